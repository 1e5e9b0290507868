#!/usr/bin/env python3
"""The likelihood pass timed against the only way to get its outputs without it, and against the posterior-predictive pass
at the same number of draws, in one session:

  iw        nm_devpass_iw      ONE launch: every expert's encoder once per tile, then S draws fused and decoded, the
                               importance weights folded per subject in registers -- eight values per row and one per
                               decoder out, no [N, D] traffic (JobSet.forward_loglik)
  launches  today's route      S back-to-back launches of the general kernel with the loc and latent exports on
                               (JobSet.forward(loss=False)) and, after each, the same fold as fp32 torch operations on the
                               device over the out_loc / out_mu / out_logvar / out_z tables of ALL models at once (views of
                               one buffer each): the Gaussian log-likelihood per decoder, the latent term with eps recovered
                               from z, the online log-sum-exp and the running sums; then the eight columns
  draws     nm_devpass_draws   the posterior-predictive pass at the same S (S <= 64 only): the same encoders, draws and
                               decoders with the per-element accumulators in HBM -- what dropping them buys

for the SE shape (3 x 379 ROI), the UCA shape (379, 379, 379 and their 1137-column early fusion) and the SM shape (1 x 379),
H = [110, 110], Z = 10, 29 covariates, gPoE, 1064 subjects, S = 8, 32 and 256, with 1, 20 and 256 models on shared tables,
in-kernel draws.  (The launches leg keeps one seed for its S launches: a new seed per launch would add a descriptor upload
per launch to that leg; its arithmetic does not depend on the seed.)
The legs alternate; --windows timed windows of --iters calls each after a warm-up call, every window closed by a device
synchronise; every window is recorded, the median of the windows is the figure, in milliseconds per call (all models, all
S draws).  The pass has no other form, so there is no pick per size, and no ratio is fixed in advance: the record is the
deliverable.

One JSON document, to --out (default profiles/devpass_iw.json)."""
import argparse, json, math, sys, time
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
    """-> (the likelihood set, the general-kernel set with its exports as views of one buffer per kind, the draws set or None)."""
    g = torch.Generator().manual_seed(77)
    c = torch.zeros(N, CDIM)
    c[torch.arange(N), torch.randint(0, CDIM, (N,), generator=g)] = 1.0
    tables = [nm.Table(torch.randn(N, d, generator=g), c, dev) for d in dims]
    ra = tables[0].rows_alloc
    locs = [torch.zeros(n_models, ra, t.x_pitch, device=dev) for t in tables]
    lat = [torch.zeros(n_models, ra, Z, device=dev) for _ in range(3)]          # out_mu, out_logvar, out_z of all models
    spec = nm.ModelSpec(dims, HIDDEN, Z, CDIM)
    mk = lambda i: nm.Job(spec, tables, combine="gpoe", seed=1000 * i, init_seed=42 + i, n_tiles_ws=tables[0].n_tiles)
    iw, gen, drw = [], [], []
    for i in range(n_models):
        job = mk(i)
        job.enable_likelihood_exports(S, per_modality=True)
        iw.append(job)
        job = mk(i)
        job.enable_exports(loc=True, sqerr=False, rowdev=False, latent=True)
        for m, t in enumerate(tables):
            job.out_loc[m] = locs[m][i][:, :t.D]
        job.out_mu, job.out_logvar, job.out_z = lat[0][i], lat[1][i], lat[2][i]
        job.touch()
        gen.append(job)
        if S <= nm._lib.NM_MAX_DRAWS:
            job = mk(i)
            job.enable_predictive_exports(S)
            drw.append(job)
    return nm.JobSet(iw), nm.JobSet(gen), (nm.JobSet(drw) if drw else None), tables, locs, lat


def time_legs(js_iw, js_gen, js_drw, tables, locs, lat, S, windows, iters, dev):
    xs = [t.x_f32 for t in tables]                  # [rows_alloc, x_pitch]: broadcasts over the models
    j0 = js_gen.jobs[0]
    # (one model's observation variance for all: the fold's cost does not depend on the values)
    lvo = [j0.layout.get(j0.params, f"{dp}logvar_out").reshape(-1) for _, _, dp in j0.kmods]
    nvs, cst = [], []
    for m, l in enumerate(locs):
        nv = torch.ones(l.shape[2], device=dev)
        nv[: lvo[m].numel()] = torch.exp(lvo[m])
        nvs.append(nv)
        cst.append(float(-0.5 * (lvo[m].double() + math.log(2 * math.pi)).sum()))
    keep = {}

    def launches():
        mu, lv, z = lat
        for s in range(S):
            js_gen.forward(loss=False)
            rec = None
            for m, loc in enumerate(locs):
                e = (xs[m] - loc)[:, :, : tables[m].D]
                ll = cst[m] - 0.5 * (e * e / nvs[m][: tables[m].D]).sum(2)
                keep[("ll", m)] = ll if s == 0 else keep[("ll", m)] + ll
                rec = ll if rec is None else rec + ll
            eps = (z - mu) * torch.exp(-0.5 * lv)
            a = -0.5 * (z * z - eps * eps - lv).sum(2)
            lw = rec + a
            if s == 0:
                mx, s1, s2 = lw, torch.ones_like(lw), torch.ones_like(lw)
                sums = [lw.clone(), a.clone(), rec.clone(), lw, lw]
            else:
                new = torch.maximum(mx, lw)
                sc, e1 = torch.exp(mx - new), torch.exp(lw - new)
                s1, s2, mx = s1 * sc + e1, s2 * sc * sc + e1 * e1, new
                sums = [sums[0] + lw, sums[1] + a, sums[2] + rec, torch.maximum(sums[3], lw), torch.minimum(sums[4], lw)]
        kl = 0.5 * (mu * mu + torch.exp(lv) - 1.0 - lv).sum(2)
        keep["row"] = torch.stack([mx + torch.log(s1) - math.log(S), sums[0] / S, s1 * s1 / s2, -sums[1] / S, kl, sums[2] / S,
                                   sums[3], sums[4]], dim=2)

    legs = {"iw": js_iw.forward_loglik, "launches": launches}
    if js_drw is not None:
        legs["draws"] = js_drw.forward_draws
    rec = {k: [] for k in legs}
    for fn in legs.values():                        # warm-up: descriptors and tables up, shadow images built, code loaded
        fn()                                        # (twice: the first call sizes the workspace, which re-uploads descriptors)
        fn()
    torch.cuda.synchronize(dev)
    for _ in range(windows):                        # (alternating: clock drift falls on every leg alike)
        for name, fn in legs.items():
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            for _ in range(iters):
                fn()
            torch.cuda.synchronize(dev)
            rec[name].append(round((time.perf_counter() - t0) / iters * 1e3, 4))
    # the two routes give the same table (draws differ only in the launches leg's single seed): the first column's scale
    rec["_log_px_mean"] = [round(float(js_iw.jobs[0].iw_row[:N, 0].mean()), 3), round(float(keep["row"][0, :N, 0].mean()), 3)]
    return rec


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--models", nargs="+", type=int, default=[1, 20, 256])
    ap.add_argument("--shapes", nargs="+", choices=tuple(SHAPES), default=list(SHAPES))
    ap.add_argument("--draws", nargs="+", type=int, default=[8, 32, 256])
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--iters", type=int, default=2)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "devpass_iw.json"))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    out = {"tool": "bench_loglik", "kernel_src_sha16": kernel_src_sha16(), "device": torch.cuda.get_device_name(dev),
           "cus": torch.cuda.get_device_properties(dev).multi_processor_count, "subjects": N, "hidden": HIDDEN, "latent": Z,
           "windows": a.windows, "iters": a.iters,
           "unit": "milliseconds per call (all models of the set, all S draws); launches = S back-to-back general-kernel passes "
                   "with the loc and latent exports on plus the fold as fp32 torch operations on the device; draws = the "
                   "posterior-predictive pass at the same S (S <= 64)",
           "sets": {}}
    for shape in a.shapes:
        dims = SHAPES[shape]
        for n in a.models:
            for S in a.draws:
                js_iw, js_gen, js_drw, tables, locs, lat = make_set(dims, n, S, dev)
                rec = time_legs(js_iw, js_gen, js_drw, tables, locs, lat, S, a.windows, a.iters, dev)
                entry = {"draws_per_row": S, "log_px_mean_of_model_0": {"iw": rec["_log_px_mean"][0], "launches": rec["_log_px_mean"][1]}}
                for leg, v in rec.items():
                    if not leg.startswith("_"):
                        entry[leg] = {"ms": v, **stats(v)}
                entry["launches_over_iw_median"] = round(entry["launches"]["median"] / entry["iw"]["median"], 3)
                entry["slowest_iw_beats_fastest_launches"] = entry["iw"]["max"] < entry["launches"]["min"]
                line = (f"{shape} x {n}, S = {S}: iw {entry['iw']['median']} ms, {S} launches + fold "
                        f"{entry['launches']['median']} ms, x{entry['launches_over_iw_median']}")
                if "draws" in entry:
                    entry["draws_over_iw_median"] = round(entry["draws"]["median"] / entry["iw"]["median"], 3)
                    line += f"; draws {entry['draws']['median']} ms, x{entry['draws_over_iw_median']}"
                out["sets"][f"{shape}_{n}_S{S}"] = entry
                print(line, flush=True)
                del js_iw, js_gen, js_drw, tables, locs, lat
                torch.cuda.empty_cache()
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
