#!/usr/bin/env python3
"""The modality-subset pass timed against the floor of every one-launch-per-subset design, in one session:

  subsets   nm_devpass_subsets  ONE launch: every expert's encoder once per tile, then the S subsets fused and decoded
                                (JobSet.forward_subsets)
  launches  nm_devpass_multi    S back-to-back launches of the full pass on the same set (JobSet.forward(loss=False,
                                compact=True)): the same decoder work, S times the encoder work, S launches

for the SE shape (3 x 379 ROI, its 7 subsets) and the UCA shape (379, 379, 379 and their 1137-column early fusion, its 15),
H = [110, 110], Z = 10, 29 covariates, gPoE, 1064 subjects, with 1, 20 and 256 models on shared tables, in-kernel draws.
Exports: the per-subject deviation alone ("rowdev", what `analysis --given` scores) and, for sets of at most --loc-max
models, the reconstruction as well ("loc", what sweep.test_folds(given=...) reads: S x M tables of [N, D] per model).
The legs alternate; --windows timed windows of --iters calls each after a warm-up call, every window closed by a device
synchronise; every window is recorded, the median of the windows is the figure, in milliseconds per call (all models, all
subsets).  No ratio is fixed in advance: the record is the deliverable.

One JSON document, to --out (default profiles/devpass_subsets.json)."""
import argparse, json, sys, time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import torch
import multi_modal_normative_modeling_amd as nm
from bench import kernel_src_sha16

SHAPES = {"SE-3": [379, 379, 379], "UCA-4": [379, 379, 379, 1137]}
HIDDEN, Z, CDIM, N = [110, 110], 10, 29, 1064


def stats(v):
    s = sorted(v)
    return {"min": s[0], "median": round((s[(len(s) - 1) // 2] + s[len(s) // 2]) / 2, 4), "max": s[-1]}


def all_subsets(M):
    return [tuple(i for i in range(M) if (mask >> i) & 1) for mask in range(1, 1 << M)]


def make_set(dims, n_models, loc, dev):
    g = torch.Generator().manual_seed(77)
    c = torch.zeros(N, CDIM)
    c[torch.arange(N), torch.randint(0, CDIM, (N,), generator=g)] = 1.0
    tables = [nm.Table(torch.randn(N, d, generator=g), c, dev) for d in dims]
    jobs = []
    for i in range(n_models):
        job = nm.Job(nm.ModelSpec(dims, HIDDEN, Z, CDIM), tables, combine="gpoe", seed=1000 * i, init_seed=42 + i,
                     n_tiles_ws=tables[0].n_tiles)
        job.enable_exports(loc=loc, sqerr=False, rowdev=True, latent=False)
        job.enable_subset_exports(all_subsets(len(dims)), loc=loc, sqerr=False, rowdev=True)
        jobs.append(job)
    return nm.JobSet(jobs)


def time_legs(js, S, windows, iters, dev):
    assert js.devpass_multi_ok()

    def launches():
        for _ in range(S):
            js.forward(loss=False, compact=True)

    legs = {"subsets": js.forward_subsets, "launches": launches}
    rec = {k: [] for k in legs}
    for fn in legs.values():                        # warm-up: descriptors and the subset table up, shadow images built, code loaded
        fn()                                        # (twice: the first call sizes the workspace, which re-uploads descriptors
        fn()                                        #  and table once more on the second)
    torch.cuda.synchronize(dev)
    for _ in range(windows):                        # (alternating: clock drift falls on both legs alike)
        for name, fn in legs.items():
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            for _ in range(iters):
                fn()
            torch.cuda.synchronize(dev)
            rec[name].append(round((time.perf_counter() - t0) / iters * 1e3, 4))
    return rec


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--models", nargs="+", type=int, default=[1, 20, 256])
    ap.add_argument("--shapes", nargs="+", choices=tuple(SHAPES), default=list(SHAPES))
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--iters", type=int, default=4)
    ap.add_argument("--loc-max", dest="loc_max", type=int, default=20, help="the largest set that also exports the reconstruction")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "devpass_subsets.json"))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    out = {"tool": "bench_subsets", "kernel_src_sha16": kernel_src_sha16(), "device": torch.cuda.get_device_name(dev),
           "cus": torch.cuda.get_device_properties(dev).multi_processor_count, "subjects": N, "hidden": HIDDEN, "latent": Z,
           "windows": a.windows, "iters": a.iters,
           "unit": "milliseconds per call (all models of the set, all S subsets); launches = S back-to-back nm_devpass_multi passes",
           "sets": {}}
    for shape in a.shapes:
        dims = SHAPES[shape]
        S = (1 << len(dims)) - 1
        for n in a.models:
            for exports in ("rowdev", "loc"):
                if exports == "loc" and n > a.loc_max:
                    continue
                js = make_set(dims, n, exports == "loc", dev)
                rec = time_legs(js, S, a.windows, a.iters, dev)
                entry = {"subsets_per_model": S, "exports": "out_rowdev" if exports == "rowdev" else "out_loc + out_rowdev"}
                for leg, v in rec.items():
                    entry[leg] = {"ms": v, **stats(v)}
                entry["launches_over_subsets_median"] = round(entry["launches"]["median"] / entry["subsets"]["median"], 3)
                entry["slowest_subsets_beats_fastest_launches"] = entry["subsets"]["max"] < entry["launches"]["min"]
                out["sets"][f"{shape}_{n}_{exports}"] = entry
                print(f"{shape} x {n} ({exports}): subsets {entry['subsets']['median']} ms, {S} launches {entry['launches']['median']} ms, "
                      f"x{entry['launches_over_subsets_median']}", flush=True)
                del js
                torch.cuda.empty_cache()
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
