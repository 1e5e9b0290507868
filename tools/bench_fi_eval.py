#!/usr/bin/env python3
"""The FI evaluation of the regression model (cVAE_multimodal_regression: joint posterior, S latent draws, every decoder, the
regressor on the residuals, the per-subject row table) timed on its two routes in one session, one process:

  two_launch  per draw the general forward kernel with exports + nm_head_regression, as run_regression_folds runs them (the
              residual images go to memory and come back), then the row table folded from the S predictions with torch
              operations: JobSet.forward_fi(compact=False) -- for S = 32 that is 32 launch pairs plus the fold
  driver      S = 1 only: JobSet.forward() + JobSet.head_regression() on the set's standing descriptors, the job's own draw, no
              row table -- the two launches exactly as run_regression_folds issued them for fold_k_pred.npy
  compact     nm_fi_pass, one launch, one workgroup per 128-row tile, the residuals in LDS (JobSet.forward_fi(compact=True))

for the UCA shape (3 x 379 ROI, H = [110, 110], Z = 10, two raw covariates) at 1064 subjects with 1, 5, 20 and 256 models
(shared tables), at S = 1 and S = 32 draws.  And the five 213-row held-out folds of a 1064-subject cohort as ONE set in one
launch against five one-job sets, one after the other, as the fold driver ran them.
The legs alternate, --repeats timed windows after a warm-up pass, every window closed by a device synchronise.  Every repeat
is recorded, with min / median / max per leg, and the verdict of the rule the automatic pick follows (engine.FI_AUTO):
nm_fi_pass is the pick for a class of sets only if its SLOWEST repeat beats the other route's FASTEST one at every set size.
Losing legs are recorded like winning ones.

One JSON document, to --out (default profiles/fi_eval.json), with the clocks record of bench.py --full.  --headline FILE ...:
bench.py result lines (of this tree and of its parent, measured in the same session) copied into the record."""
import argparse, json, sys, time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import torch
import multi_modal_normative_modeling_amd as nm
from multi_modal_normative_modeling_amd.engine import draw_seeds
from bench import device_record, kernel_src_sha16

DIMS, HIDDEN, Z, CDIM, N = [379, 379, 379], [110, 110], 10, 2, 1064
ITERS = {1: 8, 5: 4, 20: 2, 256: 1}


def stats(v):
    s = sorted(v)
    return {"min": s[0], "median": round((s[(len(s) - 1) // 2] + s[len(s) // 2]) / 2, 2), "max": s[-1]}


def make_jobs(n_models, rows, dev, seed=77):
    g = torch.Generator().manual_seed(seed)
    c = torch.rand(rows, CDIM, generator=g)
    tables = [nm.Table(torch.randn(rows, d, generator=g), c, dev) for d in DIMS]
    jobs = []
    for i in range(n_models):
        job = nm.Job(nm.ModelSpec(DIMS, HIDDEN, Z, CDIM, True, "regression"), tables, combine="gpoe", seed=1000 * i,
                     init_seed=42 + i, n_tiles_ws=tables[0].n_tiles)
        job.set_fi(torch.rand(rows, generator=g))
        job.enable_fi_exports(rows=True, draws=False, loc=False, sqerr=False, rowdev=True, latent=True)
        jobs.append(job)
    return jobs


def time_legs(legs, repeats, iters, dev):
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


def entry_of(rec):
    e = {leg: {"us": v, **stats(v)} for leg, v in rec.items()}
    # the rule's baseline: the fastest repeat of whichever old leg is faster (the driver leg builds no row table and does no
    # per-draw descriptor upload, so at S = 1 it is the one that decides wherever the host work dominates)
    old = min((k for k in e if k in ("two_launch", "driver")), key=lambda k: e[k]["min"])
    e["median_ratio_two_launch_over_compact"] = round(e["two_launch"]["median"] / e["compact"]["median"], 3)
    if "driver" in e:
        e["median_ratio_driver_over_compact"] = round(e["driver"]["median"] / e["compact"]["median"], 3)
    e["rule_baseline"] = old
    e["slowest_compact_beats_fastest_old"] = e["compact"]["max"] < e[old]["min"]
    return e


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--models", nargs="+", type=int, default=[1, 5, 20, 256])
    ap.add_argument("--draws", nargs="+", type=int, default=[1, 32])
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--no-folds", action="store_true")
    ap.add_argument("--headline", nargs="*", default=[], help="files holding bench.py result lines, recorded as given: NAME=FILE")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "fi_eval.json"))
    a = ap.parse_args()
    if a.repeats < 3:
        raise SystemExit("at least three repeats per leg: the spread of the repeats is the record's only noise figure")
    dev = torch.device("cuda:0")
    out = {"tool": "bench_fi_eval", "kernel_src_sha16": kernel_src_sha16(), "device": torch.cuda.get_device_name(dev),
           "cus": torch.cuda.get_device_properties(dev).multi_processor_count, "subjects": N, "dims": DIMS, "hidden": HIDDEN,
           "latent": Z, "repeats": a.repeats, "iters_by_models": ITERS, "unit": "microseconds per evaluation (all models of the set)",
           "sets": {}}
    verdict = True
    for S in a.draws:
        keys = draw_seeds(7, S)
        for n in a.models:
            js = nm.JobSet(make_jobs(n, N, dev))
            assert js.fi_ok()
            legs = {"two_launch": lambda: js.forward_fi(n_draws=S, seeds=keys, compact=False),
                    "compact": lambda: js.forward_fi(n_draws=S, seeds=keys, compact=True)}
            if S == 1:
                nt = max(j.tables[0].n_tiles for j in js.jobs)

                def driver(js=js, nt=nt):
                    js.forward(n_tiles=nt)
                    js.head_regression(backward=False, tile0=0, n_tiles=nt)
                legs = {"driver": driver, **legs}
            iters = max(1, ITERS.get(n, 1) // (4 if S > 1 else 1))
            e = entry_of(time_legs(legs, a.repeats, iters, dev))
            out["sets"][f"s{S}_{n}"] = e
            verdict = verdict and e["slowest_compact_beats_fastest_old"]
            print(f"S {S} x {n}: driver {e.get('driver', {}).get('median')} us, two_launch {e['two_launch']['median']} us, compact {e['compact']['median']} us, "
                  f"x{e['median_ratio_two_launch_over_compact']}, rule {e['slowest_compact_beats_fastest_old']}", flush=True)
            del js
    out["auto_pick_by_experts"] = {"3": verdict}
    if not a.no_folds:
        out["folds"] = {}
        for S in a.draws:
            keys = draw_seeds(7, S)
            per_fold = [make_jobs(1, 213, dev, seed=100 + k)[0] for k in range(5)]
            one, singles = nm.JobSet(per_fold), [nm.JobSet([j]) for j in per_fold]

            def pairs():
                for s in singles:
                    s.forward_fi(n_draws=S, seeds=keys, compact=False)
            legs = {"two_launch": pairs, "compact": lambda: one.forward_fi(n_draws=S, seeds=keys, compact=True)}
            if S == 1:
                def driver():
                    for s in singles:
                        s.forward(n_tiles=1)
                        s.head_regression(backward=False, tile0=0, n_tiles=1)
                legs = {"driver": driver, **legs}
            e = entry_of(time_legs(legs, a.repeats, 2 if S > 1 else 8, dev))
            out["folds"][f"s{S}_five_213_row_folds"] = e
            print(f"folds S {S}: driver {e.get('driver', {}).get('median')} us, five sets of launch pairs {e['two_launch']['median']} us, one launch {e['compact']['median']} us, "
                  f"x{e['median_ratio_two_launch_over_compact']}, rule {e['slowest_compact_beats_fastest_old']}", flush=True)
    out["bench_headline"] = {}
    for item in a.headline:
        name, _, path = item.partition("=")
        lines = [l for l in Path(path).read_text().splitlines() if l.startswith("{")]
        out["bench_headline"][name] = [json.loads(l) for l in lines]
    # the clocks this run saw (bench.py --full's record), from a short traced train launch of a small set
    g = torch.Generator().manual_seed(1)
    c = torch.zeros(N, 29)
    c[:, 0] = 1.0
    tabs = [nm.Table(torch.randn(N, d, generator=g), c, dev) for d in DIMS]
    js = nm.JobSet([nm.Job(nm.ModelSpec(DIMS, HIDDEN, 10, 29), tabs, combine="gpoe")])
    out["clocks"] = device_record(torch, nm, js, dev)
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
