#!/usr/bin/env python3
"""The reference's grid -- 5 folds x {SM-T1w_sMRI, SM-T2w_sMRI, SM-fMRI, UCA-gPoE}: 15 one-modality and 5 four-modality models
(commands_list_deviation.sh:13-23) -- on one device, trained

  --form grouped   one JobSet per shape, the sets trained in turn (what sweep.run_cells and bench.py --scaling strong do
                   for shapes that cannot share a launch; only API every version of the package has),
  --form one       ONE mixed JobSet, train(n, rowsplit=k) with k = rowsplit_k(mixed=True) (nm_launch_rowsplit_mixed),
  --form both      grouped / one alternating, --repeats times each, in one process.

Per repeat: one pass of --steps steps for every model after a --warmup pass; no retries; assert_finite and
check_split_errors(block=True) after each form.  One JSON line: every repeat (seconds and grid steps/s), k, helpers and
workgroups per launch, kernel_src_sha16 (bench.py's)."""
import argparse, json, sys, time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import torch
import multi_modal_normative_modeling_amd as nm
from multi_modal_normative_modeling_amd import prep, sweep, workload
from bench import kernel_src_sha16

PROCS = ["SM-T1w_sMRI", "SM-T2w_sMRI", "SM-fMRI", "UCA-gPoE"]


def build_grid(cohort, dev, n_folds=5):
    """One Job per cell, as bench.py's strong-scaling leg builds them; a fresh list per call (fresh weights and moments)."""
    cells = sweep.plan_cells(PROCS, n_folds, 1, cohort.resource)
    folds = prep.kfold_indices(len(cohort.iid), n_folds, 42)
    tables, jobs = {}, []
    for c in cells:
        mods, combine = workload.procedure_modalities(c.procedure, cohort.resource)
        key = (c.fold, tuple(mods))
        if key not in tables:
            xs, cc = prep.fold_train_tables(cohort, mods, folds[c.fold][0])
            tables[key] = [nm.Table(x, cc, dev) for x in xs]
        spec = nm.ModelSpec([t.D for t in tables[key]], list(workload.HIDDEN), workload.LATENT, workload.C_DIM)
        jobs.append(nm.Job(spec, tables[key], combine=combine, seed=1000 * c.fold + c.job_id, init_seed=42 + c.job_id, loss_cap=64))
    return jobs


def wgs(js, k):
    groups = (sum(len(j.kmods) for j in js.jobs) + 7) // 8 * 8
    return groups * (k + js.rowsplit_helpers(k)) if k > 1 else len(js.jobs)


class Grouped:
    def __init__(self, jobs):
        by_shape = {}
        for j in jobs:
            by_shape.setdefault(tuple(j.spec.input_dims), []).append(j)
        self.sets = [nm.JobSet(v) for v in by_shape.values()]
        ks = [js.rowsplit_k() for js in self.sets]
        self.record = {"launches_per_pass": len(self.sets), "k": ks, "helpers": [js.rowsplit_helpers(k) if k > 1 else 0 for js, k in zip(self.sets, ks)],
                       "workgroups": [wgs(js, k) for js, k in zip(self.sets, ks)], "models": [len(js.jobs) for js in self.sets]}

    def train(self, n):
        for js in self.sets:
            js.train(n)


class One:
    def __init__(self, jobs):
        js = nm.JobSet(jobs)
        self.sets, self.k = [js], js.rowsplit_k(mixed=True)
        if self.k <= 1:
            raise SystemExit("the grid does not fit one row-split launch on this device (rowsplit_k(mixed=True) == 1)")
        self.record = {"launches_per_pass": 1, "k": [self.k], "helpers": [js.rowsplit_helpers(self.k)], "workgroups": [wgs(js, self.k)],
                       "models": [len(jobs)]}

    def train(self, n):
        self.sets[0].train(n, rowsplit=self.k)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--form", choices=("grouped", "one", "both"), default="both")
    ap.add_argument("--steps", type=int, default=128)
    ap.add_argument("--warmup", type=int, default=32)
    ap.add_argument("--repeats", type=int, default=4)
    ap.add_argument("--subjects", type=int, default=1280)
    ap.add_argument("--tag", default="")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    cohort = prep.synthetic_cohort(n=a.subjects, d=379)
    forms = {"grouped": Grouped, "one": One}
    order = ["grouped", "one"] if a.form == "both" else [a.form]
    runs = {f: forms[f](build_grid(cohort, dev)) for f in order}
    n_models = sum(runs[order[0]].record["models"])
    out = {"tool": "bench_grid", "tag": a.tag, "form": a.form, "models": n_models, "steps": a.steps, "warmup": a.warmup,
           "repeats": a.repeats, "kernel_src_sha16": kernel_src_sha16(), "cus": torch.cuda.get_device_properties(dev).multi_processor_count}
    for f in order:
        out[f] = dict(runs[f].record, seconds=[], grid_steps_per_s=[])
        runs[f].train(a.warmup)
        torch.cuda.synchronize(dev)
    for _ in range(a.repeats):                    # (alternating: clock drift falls on both forms alike)
        for f in order:
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            runs[f].train(a.steps)
            torch.cuda.synchronize(dev)
            dt = time.perf_counter() - t0
            out[f]["seconds"].append(round(dt, 6))
            out[f]["grid_steps_per_s"].append(round(n_models * a.steps / dt, 1))
    for f in order:
        for js in runs[f].sets:
            js.check_split_errors(block=True)
            js.assert_finite()
        v = sorted(out[f]["grid_steps_per_s"])
        out[f]["median_steps_per_s"] = round((v[(len(v) - 1) // 2] + v[len(v) // 2]) / 2, 1)
        out[f]["spread_steps_per_s"] = round(v[-1] - v[0], 1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
