#!/usr/bin/env python3
"""The posterior-predictive pass timed against the only way to get its outputs without it, in one session:

  draws     nm_devpass_draws   ONE launch: every expert's encoder once per tile, then S draws fused, decoded and folded in the
                               kernel into mean / variance / mean squared error / z per ROI and the two row means
                               (JobSet.forward_draws)
  launches  the existing pass  S back-to-back launches of the full single-draw pass on the same set
                               (JobSet.forward(loss=False): nm_devpass_multi, or nm_devpass for one expert) and, after each,
                               the same fold as fp32 torch operations on the device over the out_loc tables of ALL models at
                               once (they are views of one buffer per modality), then the derived exports: S times the
                               encoder work, S launches, 2 S table reads

for the SE shape (3 x 379 ROI), the UCA shape (379, 379, 379 and their 1137-column early fusion) and the SM shape (1 x 379),
H = [110, 110], Z = 10, 29 covariates, gPoE, 1064 subjects, S = 8 and 32, with 1, 20 and 256 models on shared tables,
in-kernel draws.  (The launches leg keeps one seed for its S launches: a new seed per launch would add a descriptor upload
per launch to that leg; its arithmetic does not depend on the seed.)
The legs alternate; --windows timed windows of --iters calls each after a warm-up call, every window closed by a device
synchronise; every window is recorded, the median of the windows is the figure, in milliseconds per call (all models, all
S draws).  No ratio is fixed in advance: the record is the deliverable.

One JSON document, to --out (default profiles/devpass_draws.json)."""
import argparse, json, sys, time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import torch
import multi_modal_normative_modeling_amd as nm
from bench import kernel_src_sha16

SHAPES = {"SE-3": [379, 379, 379], "UCA-4": [379, 379, 379, 1137], "SM-1": [379]}
HIDDEN, Z, CDIM, N = [110, 110], 10, 29, 1064


def stats(v):
    s = sorted(v)
    return {"min": s[0], "median": round((s[(len(s) - 1) // 2] + s[len(s) // 2]) / 2, 4), "max": s[-1]}


def make_set(dims, n_models, S, dev):
    g = torch.Generator().manual_seed(77)
    c = torch.zeros(N, CDIM)
    c[torch.arange(N), torch.randint(0, CDIM, (N,), generator=g)] = 1.0
    tables = [nm.Table(torch.randn(N, d, generator=g), c, dev) for d in dims]
    ra = tables[0].rows_alloc
    # the single-draw pass's reconstructions of all models as one buffer per modality: the torch fold reads them in one go
    locs = [torch.zeros(n_models, ra, t.x_pitch, device=dev) for t in tables]
    jobs = []
    for i in range(n_models):
        job = nm.Job(nm.ModelSpec(dims, HIDDEN, Z, CDIM), tables, combine="gpoe", seed=1000 * i, init_seed=42 + i,
                     n_tiles_ws=tables[0].n_tiles)
        job.enable_exports(loc=True, sqerr=False, rowdev=False, latent=False)
        for m, t in enumerate(tables):
            job.out_loc[m] = locs[m][i][:, :t.D]
        job.touch()
        job.enable_predictive_exports(S)
        jobs.append(job)
    return nm.JobSet(jobs), tables, locs


def time_legs(js, tables, locs, S, windows, iters, dev):
    xs = [t.x_f32 for t in tables]                  # [rows_alloc, x_pitch]: broadcasts over the models
    nvs = [torch.full((l.shape[2],), 0.05, device=dev) for l in locs]
    keep = {}

    def launches():
        v = 1.0 / (S - 1) if S > 1 else 0.0
        cf = (S - 1) / S
        for m, loc in enumerate(locs):
            keep[m] = [torch.empty_like(loc), torch.zeros_like(loc)]
        for s in range(S):
            js.forward(loss=False)
            for m, loc in enumerate(locs):
                mean, m2 = keep[m]
                if s == 0:
                    mean.copy_(loc)
                else:
                    d = loc - mean
                    mean.add_(d, alpha=1.0 / (s + 1))
                    m2.addcmul_(d, loc - mean)
        for m, loc in enumerate(locs):
            mean, m2 = keep[m]
            var = m2 * v
            e = xs[m] - mean
            msq = e * e + var * cf
            z = e / torch.sqrt(nvs[m] + var)
            keep[m] += [var, msq, z, msq.sum(2) / tables[m].D, (z * z).sum(2) / tables[m].D]

    legs = {"draws": js.forward_draws, "launches": launches}
    rec = {k: [] for k in legs}
    for fn in legs.values():                        # warm-up: descriptors and tables up, shadow images built, code loaded
        fn()                                        # (twice: the first call sizes the workspace, which re-uploads descriptors)
        fn()
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
    ap.add_argument("--draws", nargs="+", type=int, default=[8, 32])
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--iters", type=int, default=2)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "devpass_draws.json"))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    out = {"tool": "bench_draws", "kernel_src_sha16": kernel_src_sha16(), "device": torch.cuda.get_device_name(dev),
           "cus": torch.cuda.get_device_properties(dev).multi_processor_count, "subjects": N, "hidden": HIDDEN, "latent": Z,
           "windows": a.windows, "iters": a.iters,
           "unit": "milliseconds per call (all models of the set, all S draws); launches = S back-to-back single-draw passes "
                   "plus the fold and the derived exports as fp32 torch operations on the device",
           "sets": {}}
    for shape in a.shapes:
        dims = SHAPES[shape]
        for n in a.models:
            for S in a.draws:
                js, tables, locs = make_set(dims, n, S, dev)
                rec = time_legs(js, tables, locs, S, a.windows, a.iters, dev)
                entry = {"draws_per_row": S}
                for leg, v in rec.items():
                    entry[leg] = {"ms": v, **stats(v)}
                entry["launches_over_draws_median"] = round(entry["launches"]["median"] / entry["draws"]["median"], 3)
                entry["slowest_draws_beats_fastest_launches"] = entry["draws"]["max"] < entry["launches"]["min"]
                out["sets"][f"{shape}_{n}_S{S}"] = entry
                print(f"{shape} x {n}, S = {S}: draws {entry['draws']['median']} ms, {S} launches + fold "
                      f"{entry['launches']['median']} ms, x{entry['launches_over_draws_median']}", flush=True)
                del js, tables, locs
                torch.cuda.empty_cache()
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
