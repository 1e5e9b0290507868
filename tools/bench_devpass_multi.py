#!/usr/bin/env python3
"""The multi-expert reconstruction / deviation pass (pred_recon with the joint latent, then the per-subject deviations:
multimodal_kfold_test_cvae_supervised.py:112-113) timed on its two kernels in one session:

  general   nm_forward        one workgroup per 256-row tile, 159 KB of LDS   (JobSet.forward(loss=True))
  compact   nm_devpass_multi  one workgroup per 128-row tile, two per CU      (JobSet.forward(loss=False))

for the SE shape (3 x 379 ROI) and the UCA shape (379, 379, 379 and their 1137-column early fusion), H = [110, 110], Z = 10,
29 covariates, gPoE, 1064 subjects, with 1, 5, 20 and 256 models (shared tables, the exports test_fold asks for: x_hat and
the per-subject deviation), in-kernel draws.  The legs alternate, --repeats timed windows of --iters passes each after a
warm-up pass, every window closed by a device synchronise.  Every repeat is recorded, with min / median / max per leg, each
also as a fraction of 8 N sum(D) bytes at 8 TB/s (tools/bench_deviation.py's yardstick), and the verdict of the rule the
automatic pick follows: the compact kernel stays the pick for a shape class only if its SLOWEST repeat beats the general
kernel's FASTEST one.

Second part: `sweep test`'s pass for the K = 10 folds of a 1064-subject synthetic cohort (SE-gPoE), fold by fold
(sweep.test_fold, one launch of one ~107-row job per fold) against sweep.test_folds (one launch, one job per fold): the
whole call (tables, scaler, launch, read-back) and the launches alone.

One JSON document, to --out (default profiles/devpass_multi.json)."""
import argparse, json, sys, time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import numpy as np
import torch
import multi_modal_normative_modeling_amd as nm
from multi_modal_normative_modeling_amd import prep, sweep
from bench import kernel_src_sha16

SHAPES = {"SE-3": [379, 379, 379], "UCA-4": [379, 379, 379, 1137]}
HIDDEN, Z, CDIM, N = [110, 110], 10, 29, 1064


def stats(v):
    s = sorted(v)
    return {"min": s[0], "median": round((s[(len(s) - 1) // 2] + s[len(s) // 2]) / 2, 2), "max": s[-1]}


def make_set(dims, n_models, dev):
    g = torch.Generator().manual_seed(77)
    c = torch.zeros(N, CDIM)
    c[torch.arange(N), torch.randint(0, CDIM, (N,), generator=g)] = 1.0
    tables = [nm.Table(torch.randn(N, d, generator=g), c, dev) for d in dims]
    jobs = []
    for i in range(n_models):
        job = nm.Job(nm.ModelSpec(dims, HIDDEN, Z, CDIM), tables, combine="gpoe", seed=1000 * i, init_seed=42 + i,
                     n_tiles_ws=tables[0].n_tiles)
        job.enable_exports(loc=True, sqerr=False, rowdev=True, latent=False)
        jobs.append(job)
    return nm.JobSet(jobs)


def time_legs(js, repeats, iters, dev):
    assert js.devpass_multi_ok()
    legs = {"general": True, "compact": False}      # (loss=False with compact=True: nm_devpass_multi whatever the gate says)
    rec = {k: [] for k in legs}
    for loss in legs.values():                      # warm-up: descriptors up, shadow images built, code loaded
        js.forward(loss=loss, compact=not loss or None)
    torch.cuda.synchronize(dev)
    for _ in range(repeats):                        # (alternating: clock drift falls on both legs alike)
        for name, loss in legs.items():
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            for _ in range(iters):
                js.forward(loss=loss, compact=not loss or None)
            torch.cuda.synchronize(dev)
            rec[name].append(round((time.perf_counter() - t0) / iters * 1e6, 2))
    return rec


def fold_part(repeats, dev):
    K = 10
    cohort = prep.synthetic_cohort(n=N, d=379)
    folds = prep.kfold_indices(N, K, 42)
    mods = list(prep.HCP_MODALITIES)
    spec = nm.ModelSpec([379] * 3, HIDDEN, Z, CDIM)
    jobs = []
    for k, (tr, _) in enumerate(folds):
        xs, cov = prep.fold_train_tables(cohort, mods, tr)
        jobs.append(nm.Job(spec, [nm.Table(x, cov, dev) for x in xs], combine="gpoe", seed=1000 * k, init_seed=42 + k))
    rec = {"whole_call_ms": {"fold_by_fold": [], "one_launch": []}, "launches_only_us": {"fold_by_fold": [], "one_launch": []}}
    run = {"fold_by_fold": lambda: [sweep.test_fold(jobs[k], cohort, tr, te, mods, "gpoe", dev) for k, (tr, te) in enumerate(folds)],
           "one_launch": lambda: sweep.test_folds(jobs, cohort, folds, mods, "gpoe", dev)}
    for fn in run.values():
        fn()
    for _ in range(repeats):
        for name, fn in run.items():
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize(dev)
            rec["whole_call_ms"][name].append(round((time.perf_counter() - t0) * 1e3, 3))
    evs = [sweep._fold_eval_job(jobs[k], cohort, tr, te, mods, "gpoe", dev)[0] for k, (tr, te) in enumerate(folds)]
    singles, together = [nm.JobSet([ev]) for ev in evs], nm.JobSet(evs)
    launch = {"fold_by_fold": lambda: [s.forward(loss=False) for s in singles], "one_launch": lambda: together.forward(loss=False)}
    for fn in launch.values():
        fn()
    for _ in range(repeats):
        for name, fn in launch.items():
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            for _ in range(8):
                fn()
            torch.cuda.synchronize(dev)
            rec["launches_only_us"][name].append(round((time.perf_counter() - t0) / 8 * 1e6, 2))
    for part in rec.values():
        for name in list(part):
            part[name] = {"repeats": part[name], **stats(part[name])}
    rec["folds"], rec["subjects"], rec["test_rows_per_fold"] = K, N, [int(len(te)) for _, te in folds]
    return rec


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--models", nargs="+", type=int, default=[1, 5, 20, 256])
    ap.add_argument("--shapes", nargs="+", choices=tuple(SHAPES), default=list(SHAPES))
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--iters", type=int, default=8)
    ap.add_argument("--no-folds", action="store_true")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "devpass_multi.json"))
    a = ap.parse_args()
    if a.repeats < 3:
        raise SystemExit("at least three repeats per leg: the spread of the repeats is the record's only noise figure")
    dev = torch.device("cuda:0")
    out = {"tool": "bench_devpass_multi", "kernel_src_sha16": kernel_src_sha16(), "device": torch.cuda.get_device_name(dev),
           "cus": torch.cuda.get_device_properties(dev).multi_processor_count, "subjects": N, "hidden": HIDDEN, "latent": Z,
           "repeats": a.repeats, "iters": a.iters, "unit": "microseconds per pass (all models of the set); frac = 8 N sum(D) "
           "bytes per model / time / 8 TB/s", "sets": {}}
    for shape in a.shapes:
        dims = SHAPES[shape]
        for n in a.models:
            js = make_set(dims, n, dev)
            rec = time_legs(js, a.repeats, a.iters, dev)
            byt = 8.0 * N * sum(dims) * n
            entry = {}
            for leg, v in rec.items():
                st = stats(v)
                entry[leg] = {"us": v, **st, "frac_8NsumD": {k: round(byt / st[k] / 8e6, 4) for k in ("min", "median", "max")}}
            entry["speedup_median"] = round(entry["general"]["median"] / entry["compact"]["median"], 3)
            entry["slowest_compact_beats_fastest_general"] = entry["compact"]["max"] < entry["general"]["min"]
            out["sets"][f"{shape}_{n}"] = entry
            print(f"{shape} x {n}: general {entry['general']['median']} us, compact {entry['compact']['median']} us, "
                  f"x{entry['speedup_median']}, rule {entry['slowest_compact_beats_fastest_general']}", flush=True)
            del js
    if not a.no_folds:
        out["sweep_test_folds"] = fold_part(a.repeats, dev)
        print("folds:", json.dumps(out["sweep_test_folds"]["launches_only_us"]), flush=True)
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
