#!/usr/bin/env python3
"""The joint-latent pass (what pred_latent returns: out_mu / out_logvar of every subject, cVAE.py:539-545) timed on its two
kernels in one session, one process:

  general   nm_forward      one workgroup per 256-row tile, 159 KB of LDS, decoders and export epilogue included
                            (JobSet.forward() with the latent exports on: the only way to these arrays before nm_latent_pass)
  compact   nm_latent_pass  one workgroup per 128-row tile, two per CU, encoders and fusion only (JobSet.latent(compact=True))

for the SM shape (1 x 379 ROI), the SE shape (3 x 379; also 2 x 379, so that every expert count has a record) and the UCA shape (379, 379, 379 and their 1137-column early fusion),
H = [110, 110], Z = 10, 29 covariates, gPoE, 1064 subjects, with 1, 20 and 256 models (shared tables, latent exports only).
The legs alternate, --repeats timed windows of --iters passes each after a warm-up pass, every window closed by a device
synchronise.  Every repeat is recorded, with min / median / max per leg, and the verdict of the rule the automatic pick
follows (engine.LATENT_AUTO): nm_latent_pass is the pick for a shape class only if its SLOWEST repeat beats the general
kernel's FASTEST one at every set size.

Second part: sweep.latent_folds for the K = 10 folds of a 1064-subject synthetic cohort (SE-gPoE) -- two latent launches, one
statistics and one score launch for all folds -- against the same call with the general kernel (NMHIP_LATENT=0): the whole
call (tables, scaler, launches, read-back).

One JSON document, to --out (default profiles/latent_pass.json), with the clocks record of bench.py --full."""
import argparse, json, os, sys, time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import torch
import multi_modal_normative_modeling_amd as nm
from multi_modal_normative_modeling_amd import prep, sweep
from bench import device_record, kernel_src_sha16

SHAPES = {"SM-1": [379], "SE-2": [379, 379], "SE-3": [379, 379, 379], "UCA-4": [379, 379, 379, 1137]}
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
        job.enable_exports(loc=False, sqerr=False, rowdev=False, latent=True)
        jobs.append(job)
    return nm.JobSet(jobs)


def time_legs(js, repeats, iters, dev):
    assert js.latent_ok()
    legs = {"general": js.forward, "compact": lambda: js.latent(compact=True)}
    rec = {k: [] for k in legs}
    for fn in legs.values():                        # warm-up: descriptors up, shadow images built, code loaded
        fn()
    torch.cuda.synchronize(dev)
    for _ in range(repeats):                        # (alternating: clock drift falls on both legs alike)
        for name, fn in legs.items():
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            for _ in range(iters):
                fn()
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

    def call(env):
        old = os.environ.get("NMHIP_LATENT")
        os.environ["NMHIP_LATENT"] = env
        try:
            return sweep.latent_folds(jobs, cohort, folds, mods, "gpoe", dev)
        finally:
            if old is None:
                del os.environ["NMHIP_LATENT"]
            else:
                os.environ["NMHIP_LATENT"] = old
    run = {"general_kernel": lambda: call("0"), "latent_pass": lambda: call("1")}
    rec = {"whole_call_ms": {k: [] for k in run}}
    for fn in run.values():
        fn()
    for _ in range(repeats):
        for name, fn in run.items():
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize(dev)
            rec["whole_call_ms"][name].append(round((time.perf_counter() - t0) * 1e3, 3))
    for name in list(rec["whole_call_ms"]):
        v = rec["whole_call_ms"][name]
        rec["whole_call_ms"][name] = {"repeats": v, **stats(v)}
    rec["folds"], rec["subjects"] = K, N
    rec["train_rows_per_fold"], rec["test_rows_per_fold"] = [int(len(tr)) for tr, _ in folds], [int(len(te)) for _, te in folds]
    return rec


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--models", nargs="+", type=int, default=[1, 20, 256])
    ap.add_argument("--shapes", nargs="+", choices=tuple(SHAPES), default=list(SHAPES))
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--iters", type=int, default=32)
    ap.add_argument("--no-folds", action="store_true")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "latent_pass.json"))
    a = ap.parse_args()
    if a.repeats < 3:
        raise SystemExit("at least three repeats per leg: the spread of the repeats is the record's only noise figure")
    dev = torch.device("cuda:0")
    out = {"tool": "bench_latent", "kernel_src_sha16": kernel_src_sha16(), "device": torch.cuda.get_device_name(dev),
           "cus": torch.cuda.get_device_properties(dev).multi_processor_count, "subjects": N, "hidden": HIDDEN, "latent": Z,
           "repeats": a.repeats, "iters": a.iters, "unit": "microseconds per pass (all models of the set)", "sets": {}}
    verdict = {}
    for shape in a.shapes:
        dims = SHAPES[shape]
        for n in a.models:
            js = make_set(dims, n, dev)
            rec = time_legs(js, a.repeats, a.iters, dev)
            entry = {leg: {"us": v, **stats(v)} for leg, v in rec.items()}
            entry["speedup_median"] = round(entry["general"]["median"] / entry["compact"]["median"], 3)
            entry["slowest_compact_beats_fastest_general"] = entry["compact"]["max"] < entry["general"]["min"]
            out["sets"][f"{shape}_{n}"] = entry
            verdict[shape] = verdict.get(shape, True) and entry["slowest_compact_beats_fastest_general"]
            print(f"{shape} x {n}: general {entry['general']['median']} us, compact {entry['compact']['median']} us, "
                  f"x{entry['speedup_median']}, rule {entry['slowest_compact_beats_fastest_general']}", flush=True)
            del js
    out["auto_pick_by_experts"] = {str(len(SHAPES[s])): v for s, v in verdict.items()}
    if not a.no_folds:
        out["sweep_latent_folds"] = fold_part(a.repeats, dev)
        print("folds:", json.dumps(out["sweep_latent_folds"]["whole_call_ms"]), flush=True)
    # the clocks this run saw (bench.py --full's record), from a short traced train launch of a small set
    js = make_set(SHAPES["SE-3"], 1, dev)
    out["clocks"] = device_record(torch, nm, js, dev)
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
