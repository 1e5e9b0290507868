#!/usr/bin/env python3
"""Small sweeps of head models -- a k-fold run of cVAE_multimodal_regression (3 x 379 ROI, H = [110, 110], Z = 10, two raw
covariates, gPoE) or of cVAE_multimodal_endtoend (config 5: Z = 64, 29 covariates, classifier [128, 64, 32]) -- trained in
the persistent launch

  whole   one workgroup per model            (nm_train_steps_head),
  split   one workgroup per decoder: 3 / 6   (nm_train_steps_head_split),

for 1, 5 and 20 models, the forms alternating, --repeats timed windows of --steps steps each after a --warmup window, every
window closed by a device synchronise; in-kernel draws; assert_finite and check_split_errors(block=True) at the end of
every set.  --forms whole runs on a tree without the split form as well (the record of the commit before it).
--parent-json: such a record, taken in the same session, is folded in and the three comparisons of the record are made:
split against the parent's whole form (slowest split repeat against fastest parent repeat), and this tree's whole form
against the parent's.  One JSON document, to --out if given, else to stdout."""
import argparse, json, os, sys, time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import torch
import multi_modal_normative_modeling_amd as nm
from bench import kernel_src_sha16

DIMS, HIDDEN = [379, 379, 379], [110, 110]


def make_job(kind, i, rows, dev):
    g = torch.Generator().manual_seed(1000 + i)
    xes = [torch.randn(rows, d, generator=g) for d in DIMS]
    if kind == "regression":
        c = torch.rand(rows, 2, generator=g)
        spec = nm.ModelSpec(DIMS, HIDDEN, 10, 2, True, "regression")
        job = nm.Job(spec, [nm.Table(x, c, dev) for x in xes], combine="gpoe", seed=1000 * i, init_seed=42 + i, loss_cap=8)
        job.set_fi(torch.randn(rows, generator=g) * 0.5 + 1.0)
        return job
    c = torch.zeros(rows, 29)
    c[torch.arange(rows), torch.randint(0, 29, (rows,), generator=g)] = 1.0
    spec = nm.ModelSpec(DIMS, HIDDEN, 64, 29, True, "endtoend", (128, 64, 32), 2)
    job = nm.Job(spec, [nm.Table(x, c, dev) for x in xes], combine="poe", kl_weight=0.1, ll_weight=0.1, seed=1000 * i,
                 init_seed=42 + i, loss_cap=8, single_bypass=False)
    job.cls_dropout, job.cls_margin, job.cls_w_contrast = 0.5, 1.0, 0.1
    job.set_labels((torch.rand(rows, generator=g) < 0.4).long())
    return job


def train(js, kind, form, n):
    fn = js.train_regression if kind == "regression" else js.train_endtoend
    if form == "split":
        fn(n, split=True)
    else:                                   # (the switch every version of the package reads; no keyword the older ones lack)
        old = os.environ.get("NMHIP_SPLIT")
        os.environ["NMHIP_SPLIT"] = "0"
        try:
            fn(n)
        finally:
            if old is None:
                del os.environ["NMHIP_SPLIT"]
            else:
                os.environ["NMHIP_SPLIT"] = old


def stats(v):
    s = sorted(v)
    return {"median": round((s[(len(s) - 1) // 2] + s[len(s) // 2]) / 2, 2), "min": s[0], "max": s[-1],
            "spread": round(s[-1] - s[0], 2)}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--forms", nargs="+", choices=("whole", "split"), default=["whole", "split"])
    ap.add_argument("--kinds", nargs="+", choices=("regression", "endtoend"), default=["regression", "endtoend"])
    ap.add_argument("--models", nargs="+", type=int, default=[1, 5, 20])
    ap.add_argument("--steps", type=int, default=384)
    ap.add_argument("--warmup", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--rows", type=int, default=1024, help="rows of every training table (1280 subjects, 5 folds: 1024)")
    ap.add_argument("--tag", default="")
    ap.add_argument("--parent-json", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.repeats < 3:
        raise SystemExit("at least three repeats per form: the spread of the repeats is the record's only noise figure")
    dev = torch.device("cuda:0")
    out = {"tool": "bench_heads", "tag": a.tag, "forms": a.forms, "steps": a.steps, "warmup": a.warmup, "repeats": a.repeats,
           "rows": a.rows, "kernel_src_sha16": kernel_src_sha16(), "device": torch.cuda.get_device_name(dev),
           "cus": torch.cuda.get_device_properties(dev).multi_processor_count, "unit": "microseconds per sweep step "
           "(one step of every model of the set) and model steps per second", "sets": {}}
    for kind in a.kinds:
        for n in a.models:
            sets = {f: nm.JobSet([make_job(kind, i, a.rows, dev) for i in range(n)]) for f in a.forms}   # (fresh weights per form)
            rec = {f: {"seconds": [], "us_per_sweep_step": [], "model_steps_per_s": []} for f in a.forms}
            for f in a.forms:
                train(sets[f], kind, f, a.warmup)
                torch.cuda.synchronize(dev)
            for _ in range(a.repeats):            # (alternating: clock drift falls on both forms alike)
                for f in a.forms:
                    torch.cuda.synchronize(dev)
                    t0 = time.perf_counter()
                    train(sets[f], kind, f, a.steps)
                    torch.cuda.synchronize(dev)
                    dt = time.perf_counter() - t0
                    rec[f]["seconds"].append(round(dt, 6))
                    rec[f]["us_per_sweep_step"].append(round(dt / a.steps * 1e6, 2))
                    rec[f]["model_steps_per_s"].append(round(n * a.steps / dt, 1))
            for f in a.forms:
                sets[f].check_split_errors(block=True)
                sets[f].assert_finite()
                rec[f]["us"] = stats(rec[f]["us_per_sweep_step"])
                if f == "split":
                    rec[f]["parts"] = len(sets[f].jobs[0].kmods)
                    rec[f]["workgroups"] = (n + 7) // 8 * 8 * rec[f]["parts"]
            if "whole" in rec and "split" in rec:
                rec["ratio_whole_over_split_median"] = round(rec["whole"]["us"]["median"] / rec["split"]["us"]["median"], 3)
            out["sets"][f"{kind}_{n}"] = rec
            del sets
    if a.parent_json:
        par = json.loads(Path(a.parent_json).read_text())
        out["parent"] = {"kernel_src_sha16": par["kernel_src_sha16"], "sets": {k: v["whole"] for k, v in par["sets"].items()}}
        cmp = {}
        for key, rec in out["sets"].items():
            pw = out["parent"]["sets"].get(key)
            if pw is None:
                continue
            c = {"parent_whole_us": pw["us"]}
            if "split" in rec:
                c["split_us"] = rec["split"]["us"]
                c["ratio_parent_whole_over_split_median"] = round(pw["us"]["median"] / rec["split"]["us"]["median"], 3)
                c["slowest_split_beats_fastest_parent_whole"] = rec["split"]["us"]["max"] < pw["us"]["min"]
            if "whole" in rec:
                c["whole_us"] = rec["whole"]["us"]
                d = abs(rec["whole"]["us"]["median"] - pw["us"]["median"])
                c["whole_minus_parent_whole_median_us"] = round(rec["whole"]["us"]["median"] - pw["us"]["median"], 2)
                c["whole_within_spread_of_parent_whole"] = d <= max(rec["whole"]["us"]["spread"], pw["us"]["spread"])
            cmp[key] = c
        out["against_parent"] = cmp
    text = json.dumps(out, indent=1)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(text + "\n")
    print(json.dumps(out.get("against_parent", {k: v.get("ratio_whole_over_split_median") for k, v in out["sets"].items()})))


if __name__ == "__main__":
    main()
