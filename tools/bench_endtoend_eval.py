#!/usr/bin/env python3
"""The evaluation of the end-to-end model (cVAE_multimodal_endtoend: joint posterior, eval-mode classifier, both decoder
banks, the per-subject row table) timed on its two routes in one session, one process:

  two_launch  nm_forward + nm_head_classifier as run_endtoend_folds has always run them: the exports enabled once, the
              descriptors kept on the device from pass to pass, JobSet.forward() then JobSet.head_classifier(); for "table" the
              row table folded from the exports with torch operations (engine._endtoend_row_fold) after them
  fallback    JobSet.forward_endtoend(compact=False): the same two launches behind the new entry point, which for
              latent="mean" installs an all-zero draw per call (a descriptor upload per job; recorded, not part of the rule)
  compact     nm_e2e_pass, one launch, one workgroup per 128-row tile (JobSet.forward_endtoend(compact=True))

for BASELINE config 5's shape (3 x 379 ROI, H = [110, 110], 29 covariates, classifier [128, 64, 32]) at 1064 subjects with 1, 5,
20 and 256 models (shared tables), at Z = 64 and at Z = 10; each with the row table and out_rowdev on ("table") and with the
logits alone ("logits": no row table, no decoder export -- the compact pass then skips the decoders).  And the five 213-row
held-out folds of a 1064-subject cohort as ONE set in one launch against five one-job sets, one after the other.
The legs alternate, --repeats timed windows after a warm-up pass, every window closed by a device synchronise.  Every repeat
is recorded, with min / median / max per leg, and the verdict of the rule the automatic pick follows (engine.E2E_AUTO):
nm_e2e_pass is the pick for a class of sets only if its SLOWEST repeat beats the other route's FASTEST one at every set
size.  Losing legs are recorded like winning ones.

One JSON document, to --out (default profiles/endtoend_eval.json), with the clocks record of bench.py --full."""
import argparse, json, sys, time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import torch
import multi_modal_normative_modeling_amd as nm
from bench import device_record, kernel_src_sha16

DIMS, HIDDEN, CDIM, LAYERS, N = [379, 379, 379], [110, 110], 29, (128, 64, 32), 1064
ITERS = {1: 16, 5: 8, 20: 4, 256: 1}


def stats(v):
    s = sorted(v)
    return {"min": s[0], "median": round((s[(len(s) - 1) // 2] + s[len(s) // 2]) / 2, 2), "max": s[-1]}


def make_jobs(Z, n_models, rows, table, dev, seed=77):
    g = torch.Generator().manual_seed(seed)
    c = torch.zeros(rows, CDIM)
    c[torch.arange(rows), torch.randint(0, CDIM, (rows,), generator=g)] = 1.0
    tables = [nm.Table(torch.randn(rows, d, generator=g), c, dev) for d in DIMS]
    jobs = []
    for i in range(n_models):
        job = nm.Job(nm.ModelSpec(DIMS, HIDDEN, Z, CDIM, True, "endtoend", LAYERS, 2), tables, combine="poe", seed=1000 * i,
                     init_seed=42 + i, single_bypass=False, n_tiles_ws=tables[0].n_tiles)
        job.cls_train, job.cls_use_mu = False, True       # model.eval(); predict(): classifier(mu)
        job.enable_endtoend_exports(rows=table, loc=False, sqerr=False, rowdev=table)
        jobs.append(job)
    return jobs


def parent_route(js, table):
    """forward() + head_classifier() on the set's standing descriptors (+ the torch fold of the row table)."""
    from multi_modal_normative_modeling_amd.engine import _endtoend_row_fold
    nt = max(j.tables[0].n_tiles for j in js.jobs)

    def run():
        js.forward(n_tiles=nt)
        js.head_classifier(backward=False, tile0=0, n_tiles=nt)
        if table:
            for j in js.jobs:
                _endtoend_row_fold(j, 0, j.tables[0].rows_alloc)
    return run


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
    e["speedup_median"] = round(e["two_launch"]["median"] / e["compact"]["median"], 3)
    e["slowest_compact_beats_fastest_two_launch"] = e["compact"]["max"] < e["two_launch"]["min"]
    return e


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--models", nargs="+", type=int, default=[1, 5, 20, 256])
    ap.add_argument("--latents", nargs="+", type=int, default=[64, 10])
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--no-folds", action="store_true")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "endtoend_eval.json"))
    a = ap.parse_args()
    if a.repeats < 3:
        raise SystemExit("at least three repeats per leg: the spread of the repeats is the record's only noise figure")
    dev = torch.device("cuda:0")
    out = {"tool": "bench_endtoend_eval", "kernel_src_sha16": kernel_src_sha16(), "device": torch.cuda.get_device_name(dev),
           "cus": torch.cuda.get_device_properties(dev).multi_processor_count, "subjects": N, "dims": DIMS, "hidden": HIDDEN,
           "classifier": list(LAYERS), "repeats": a.repeats, "iters_by_models": ITERS,
           "unit": "microseconds per pass (all models of the set)", "sets": {}}
    verdict = True
    for Z in a.latents:
        for n in a.models:
            for what in ("table", "logits"):
                js = nm.JobSet(make_jobs(Z, n, N, what == "table", dev))
                assert js.e2e_ok()
                legs = {"two_launch": parent_route(js, what == "table"), "fallback": lambda: js.forward_endtoend(compact=False),
                        "compact": lambda: js.forward_endtoend(compact=True)}
                e = entry_of(time_legs(legs, a.repeats, ITERS.get(n, 1), dev))
                out["sets"][f"z{Z}_{n}_{what}"] = e
                verdict = verdict and e["slowest_compact_beats_fastest_two_launch"]
                print(f"Z {Z} x {n} {what}: two_launch {e['two_launch']['median']} us, compact {e['compact']['median']} us, "
                      f"x{e['speedup_median']}, rule {e['slowest_compact_beats_fastest_two_launch']}", flush=True)
                del js
    out["auto_pick_by_experts"] = {"3": verdict}
    if not a.no_folds:
        out["folds"] = {}
        for Z in a.latents:
            per_fold = [make_jobs(Z, 1, 213, True, dev, seed=100 + k)[0] for k in range(5)]
            one, singles = nm.JobSet(per_fold), [nm.JobSet([j]) for j in per_fold]

            routes = [parent_route(s, True) for s in singles]

            def pairs():
                for r in routes:
                    r()
            legs = {"two_launch": pairs, "compact": lambda: one.forward_endtoend(compact=True)}
            e = entry_of(time_legs(legs, a.repeats, 8, dev))
            out["folds"][f"z{Z}_five_213_row_folds"] = e
            print(f"folds Z {Z}: five launch pairs {e['two_launch']['median']} us, one launch {e['compact']['median']} us, "
                  f"x{e['speedup_median']}, rule {e['slowest_compact_beats_fastest_two_launch']}", flush=True)
    # the clocks this run saw (bench.py --full's record), from a short traced train launch of a small set
    g = torch.Generator().manual_seed(1)
    c = torch.zeros(N, CDIM)
    c[:, 0] = 1.0
    tabs = [nm.Table(torch.randn(N, d, generator=g), c, dev) for d in DIMS]
    js = nm.JobSet([nm.Job(nm.ModelSpec(DIMS, HIDDEN, 10, CDIM), tabs, combine="gpoe")])
    out["clocks"] = device_record(torch, nm, js, dev)
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
