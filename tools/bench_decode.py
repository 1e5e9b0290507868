#!/usr/bin/env python3
"""The decoder pass over a covariate grid (nm_decode_pass: every decoder of every model under G cells in ONE launch) timed
against the two other routes to the same numbers, in one session, one process:

  pass     nm_decode_pass   one workgroup per 128-row tile, two per CU, decoders only, the loop over the cells inside
                            (JobSet.decode() on requests of R rows x G cells)
  zgiven   nm_forward       today's route, what the classes' decode(z, c, m) does: per cell and modality a one-modality model
                            on the general kernel with NM_F_ZGIVEN (its encoder runs on an all-zero x).  ONE cell is timed --
                            a launch per modality over all models -- and multiplied by G: the cells' launches cost the same
  torch    fp32 torch.nn.functional.linear chains on the same device, the cells stacked into the batch ([G * R, Z + C] per
                            model and modality: the form most favourable to it)

for the SM shape (1 x 379 ROI), the SE shape (3 x 379) and the UCA shape (379, 379, 379, 1137), H = [110, 110], Z = 10, 29
covariates, with 1, 20 and 256 models, G = 54 cells x S = 256 prior rows (the normative trajectory) and G = 54 x 1064 subject
rows (counterfactual reconstructions of a cohort).  The legs alternate, --repeats timed windows after a warm-up pass, every
window closed by a device synchronise; every repeat is recorded, with min / median / max per leg, and whether on this GRID
workload the pass's SLOWEST repeat beats the FASTEST extrapolated zgiven figure at every set size of a shape class
(grid_rule_by_decoders; the routing of single decode() calls, engine.DECODE_AUTO, needs a record of its own).  A set whose exports would not fit --max-gb is recorded as skipped.

One JSON document, to --out (default profiles/decode_pass.json), with the clocks record of bench.py --full."""
import argparse, json, sys, time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import torch
import multi_modal_normative_modeling_amd as nm
from multi_modal_normative_modeling_amd import _lib
from bench import device_record, kernel_src_sha16

SHAPES = {"SM-1": [379], "SE-3": [379, 379, 379], "UCA-4": [379, 379, 379, 1137]}
HIDDEN, Z, CDIM, G = [110, 110], 10, 29, 54
ROWS = {"prior_256": 256, "subjects_1064": 1064}


def stats(v):
    s = sorted(v)
    return {"min": s[0], "median": round((s[(len(s) - 1) // 2] + s[len(s) // 2]) / 2, 4), "max": s[-1]}


def grid():
    g = torch.zeros(G, CDIM)
    for cell in range(G):                            # 27 age bins x 2 sexes, one-hot pair
        g[cell, cell // 2], g[cell, 27 + cell % 2] = 1.0, 1.0
    return g


def export_gb(dims, n_models, R):
    ra = (R + 255) // 256 * 256
    return sum(G * ra * ((d + 3) // 4 * 4) * 4 for d in dims) * n_models / 2 ** 30


def make_pass(dims, n_models, R, dev):
    place = [nm.Table(torch.zeros(1, d), torch.zeros(1, CDIM), dev) for d in dims]
    z = torch.randn(R, Z, generator=torch.Generator().manual_seed(5))
    jobs = []
    for i in range(n_models):
        job = nm.Job(nm.ModelSpec(dims, HIDDEN, Z, CDIM), place, combine="gpoe", seed=1000 * i, init_seed=42 + i)
        job.enable_decode_exports(R, G)
        job.set_decode_inputs(z, c_grid=grid(), x=None)
        jobs.append(job)
    js = nm.JobSet(jobs)
    assert js.decode_ok()
    return js, js.decode


def make_zgiven(dims, n_models, R, dev):
    """Per modality a set of one-modality models on tables of R rows carrying one cell's covariates; the pass of ONE cell."""
    z = torch.randn(R, Z, generator=torch.Generator().manual_seed(5))
    nt = (R + 255) // 256
    eps = torch.zeros(nt * 256, Z)
    eps[:R] = z
    c = grid()[:1].repeat(R, 1)
    sets = []
    for d in dims:
        tab = [nm.Table(torch.zeros(R, d), c, dev)]
        jobs = []
        for i in range(n_models):
            job = nm.Job(nm.ModelSpec([d], HIDDEN, Z, CDIM), tab, combine="poe", seed=1000 * i, init_seed=42 + i, n_tiles_ws=nt)
            job.set_eps(eps.view(nt, 256, Z))
            job.enable_exports(loc=True, sqerr=False, rowdev=False, latent=True)
            jobs.append(job)
        sets.append(nm.JobSet(jobs))

    def one_cell():
        for js in sets:
            js._launch(0, 1, nt, _lib.NM_F_EXPORT | _lib.NM_F_ZGIVEN)
    return sets, one_cell


def make_torch(dims, n_models, R, dev):
    gen = torch.Generator().manual_seed(9)
    inp = torch.cat([torch.randn(R, Z, generator=gen).repeat(G, 1), grid().repeat_interleave(R, 0)], 1).to(dev)
    widths = [Z + CDIM] + HIDDEN[::-1]
    models = []
    for _ in range(n_models):
        per_mod = []
        for d in dims:
            ws = [(torch.randn(o, i, generator=gen).to(dev) * 0.05, torch.zeros(o, device=dev)) for i, o in zip(widths, widths[1:] + [d])]
            per_mod.append(ws)
        models.append(per_mod)

    def chain():
        out = None
        for per_mod in models:
            for ws in per_mod:
                h = inp
                for w, b in ws[:-1]:
                    h = torch.nn.functional.leaky_relu(torch.nn.functional.linear(h, w, b), 0.01)
                out = torch.nn.functional.linear(h, ws[-1][0], ws[-1][1])
        return out
    return models, chain


def time_legs(legs, repeats, dev):
    rec = {k: [] for k in legs}
    for fn, _, _ in legs.values():                   # warm-up: descriptors up, shadow images built, code loaded
        fn()
    torch.cuda.synchronize(dev)
    for _ in range(repeats):                         # (alternating: clock drift falls on all legs alike)
        for name, (fn, iters, scale) in legs.items():
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            for _ in range(iters):
                fn()
            torch.cuda.synchronize(dev)
            rec[name].append(round((time.perf_counter() - t0) / iters * 1e3 * scale, 4))
    return rec


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--models", nargs="+", type=int, default=[1, 20, 256])
    ap.add_argument("--shapes", nargs="+", choices=tuple(SHAPES), default=list(SHAPES))
    ap.add_argument("--rows", nargs="+", choices=tuple(ROWS), default=list(ROWS))
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--max-gb", type=float, default=48.0, help="skip a set whose decode exports would be larger")
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "decode_pass.json"))
    a = ap.parse_args()
    if a.repeats < 3:
        raise SystemExit("at least three repeats per leg: the spread of the repeats is the record's only noise figure")
    dev = torch.device("cuda:0")
    out = {"tool": "bench_decode", "kernel_src_sha16": kernel_src_sha16(), "device": torch.cuda.get_device_name(dev),
           "cus": torch.cuda.get_device_properties(dev).multi_processor_count, "cells": G, "hidden": HIDDEN, "latent": Z,
           "repeats": a.repeats, "unit": "milliseconds per call (all cells, all decoders, all models of the set)",
           "zgiven_note": "EXTRAPOLATED: one cell timed (a launch per modality over all models), times the number of cells", "sets": {}}
    verdict = {}
    for shape in a.shapes:
        dims = SHAPES[shape]
        for rows_name in a.rows:
            R = ROWS[rows_name]
            for n in a.models:
                key = f"{shape}_{rows_name}_{n}"
                gb = export_gb(dims, n, R)
                if gb > a.max_gb:
                    out["sets"][key] = {"skipped": f"the exports of the pass would take {gb:.1f} GB (--max-gb {a.max_gb:g})"}
                    print(f"{key}: skipped, {gb:.1f} GB of exports", flush=True)
                    continue
                work = n * len(dims) * G * R                  # decoded rows per call: the iteration counts follow it
                it = max(1, min(16, int(4e6 // work)))
                keep_p, fp = make_pass(dims, n, R, dev)
                keep_z, fz = make_zgiven(dims, n, R, dev)
                legs = {"pass": (fp, it, 1.0), "zgiven": (fz, max(2, min(16, it * 8)), float(G))}
                if not a.no_torch:
                    keep_t, ft = make_torch(dims, n, R, dev)
                    legs["torch"] = (ft, it, 1.0)
                rec = time_legs(legs, a.repeats, dev)
                entry = {leg: {"ms": v, **stats(v)} for leg, v in rec.items()}
                entry["export_gb"] = round(gb, 3)
                entry["speedup_median_vs_zgiven"] = round(entry["zgiven"]["median"] / entry["pass"]["median"], 3)
                if "torch" in entry:
                    entry["speedup_median_vs_torch"] = round(entry["torch"]["median"] / entry["pass"]["median"], 3)
                entry["slowest_pass_beats_fastest_zgiven"] = entry["pass"]["max"] < entry["zgiven"]["min"]
                out["sets"][key] = entry
                verdict[shape] = verdict.get(shape, True) and entry["slowest_pass_beats_fastest_zgiven"]
                print(f"{key}: " + ", ".join(f"{leg} {entry[leg]['median']} ms" for leg in rec) +
                      f", rule {entry['slowest_pass_beats_fastest_zgiven']}", flush=True)
                del keep_p, keep_z, legs, fp, fz
                if not a.no_torch:
                    del keep_t, ft
                torch.cuda.empty_cache()
    # (the rule on the GRID workload, per number of decoders; it does not govern the classes' decode(): engine.DECODE_AUTO follows
    #  a record of single calls, which this tool does not make)
    out["grid_rule_by_decoders"] = {str(len(SHAPES[s])): v for s, v in verdict.items()}
    out["grid_rule_note"] = ("slowest pass repeat below the fastest extrapolated zgiven figure at every set of the class, on the "
                             "54-cell grid workload; engine.DECODE_AUTO (the routing of single decode() calls) is not set from it")
    place = [nm.Table(torch.zeros(256, d), torch.zeros(256, CDIM), dev) for d in SHAPES["SE-3"]]
    js = nm.JobSet([nm.Job(nm.ModelSpec(SHAPES["SE-3"], HIDDEN, Z, CDIM), place, combine="gpoe")])
    out["clocks"] = device_record(torch, nm, js, dev)
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
