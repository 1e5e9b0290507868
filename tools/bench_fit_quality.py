#!/usr/bin/env python3
"""Model fit per ROI (metrics.fit_quality -> nm_fit_quality / nm_fit_rank) timed in one session, one process, three ways on the
same data:

  kernel   one launch for all sets per entry point (pointer table, the three tables read where they lie)
  torch    the same quantities as fp64 torch expressions on the same device, the sets one after another: Pearson's rho, SMSE,
           EXPV, MSLL, RMSE, bias, MAE, the moments of z and its coverage; Spearman's rho from mid-ranks by two searchsorted
           calls per column on the sorted column
  host     scipy.stats (pearsonr, spearmanr, skew, kurtosis) and sklearn.metrics (r2_score, explained_variance_score) column
           by column on one set, on copies made beforehand -- what a user without this package would call

for 1064 evaluated subjects, D = 379 (one modality) and D = 1137 (the early-fusion table), with 1, 20 and 256 sets (every set
three tables of its own, a per-column variance and a trivial model).  Each leg: a warm-up call, then --repeats timed windows
of some calls each, every window closed by a device synchronise; every repeat is recorded, with min / median / max.  Before the
timing the kernel's first and last set are compared with the yardstick of the tests (tests/fit_quality_ref.py).  The quality
pass is also given as the fraction of the time 24 N D bytes per set take at 8 TB/s (it reads its three tables twice), next to
metrics.cohort_moments on the x tables of the same session against its 8 N D.  No ratio is a target: all legs are recorded as
they come.

One JSON document, to --out (default profiles/fit_quality.json), with the clocks record of bench.py --full."""
import argparse, json, sys, time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))
import numpy as np
import torch
import multi_modal_normative_modeling_amd as nm
from multi_modal_normative_modeling_amd import metrics
from bench import device_record, kernel_src_sha16
from bench_roi_effect import stats, timed
from tests import fit_quality_ref as R

N = 1064
THR = 1.96
HBM_BYTES_PER_S = 8e12


def make_sets(D, n_sets, dev):
    g = torch.Generator(device=dev).manual_seed(1000 * D + n_sets)
    pitch = (D + 3) // 4 * 4                                      # the evaluation jobs' table pitch
    xs, locs, vs, cvs = [], [], [], []
    for _ in range(n_sets):
        sig = torch.randn(N, pitch, device=dev, generator=g)
        xs.append((0.8 * sig + 0.6 * torch.randn(N, pitch, device=dev, generator=g))[:, :D])
        locs.append((0.75 * sig)[:, :D])
        vs.append((0.05 + 0.1 * torch.rand(N, pitch, device=dev, generator=g))[:, :D])
        cvs.append(0.3 + 0.1 * torch.rand(D, device=dev, generator=g))
    group = torch.zeros(N, dtype=torch.int32)                     # every row a hold-out control
    mom = metrics.cohort_moments(xs, [group] * n_sets, ddof=0, device=dev)
    return xs, locs, vs, cvs, [group] * n_sets, mom


def torch_quality(xs, locs, vs, cvs, mom):
    keep = None
    for k, (x, f, v, c) in enumerate(zip(xs, locs, vs, cvs)):
        y, f = x.double(), f.double()
        s2 = v.double() + c.double()
        e = y - f
        n = y.shape[0]
        dy, df, de = y - y.mean(0), f - f.mean(0), e - e.mean(0)
        syy, sff, syf, see, sse = (dy * dy).sum(0), (df * df).sum(0), (dy * df).sum(0), (de * de).sum(0), (e * e).sum(0)
        z = e / s2.sqrt()
        dz = z - z.mean(0)
        m2, m3, m4 = (dz ** 2).mean(0), (dz ** 3).mean(0), (dz ** 4).mean(0)
        m_t, v_t = mom[k, :, 0], mom[k, :, 2]
        msll = (0.5 * torch.log(2 * np.pi * s2) + e * e / (2 * s2)).mean(0) - (0.5 * torch.log(2 * np.pi * v_t) + ((y - m_t) ** 2).sum(0) / (2 * v_t * n))
        keep = (syf / (syy * sff).sqrt(), sse / syy, 1 - see / syy, msll, (sse / n).sqrt(), e.mean(0), e.abs().mean(0), z.mean(0),
                m2.sqrt(), m3 / m2 ** 1.5, m4 / m2 ** 2 - 3, (z.abs() <= THR).double().mean(0))
    return keep


def torch_rank(xs, locs):
    keep = None
    for x, f in zip(xs, locs):
        ks = []
        for v in (x, f):
            vt = v.T.contiguous()
            s = vt.sort(dim=1).values
            ks.append((torch.searchsorted(s, vt, right=False) + torch.searchsorted(s, vt, right=True)).double())
        a, b = ks[0] - ks[0].mean(1, keepdim=True), ks[1] - ks[1].mean(1, keepdim=True)
        keep = (a * b).sum(1) / ((a * a).sum(1) * (b * b).sum(1)).sqrt()
    return keep


def host_leg(x, f, v, c):
    from scipy import stats as st
    from sklearn import metrics as skm
    y, f = x.astype(np.float64), f.astype(np.float64)
    z = (y - f) / np.sqrt(v.astype(np.float64) + c.astype(np.float64))
    for d in range(y.shape[1]):
        st.pearsonr(y[:, d], f[:, d]), st.spearmanr(y[:, d], f[:, d]), st.skew(z[:, d]), st.kurtosis(z[:, d])
        skm.r2_score(y[:, d], f[:, d]), skm.explained_variance_score(y[:, d], f[:, d])


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--widths", nargs="+", type=int, default=[379, 1137])
    ap.add_argument("--sets", nargs="+", type=int, default=[1, 20, 256])
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "fit_quality.json"))
    a = ap.parse_args()
    if a.repeats < 3:
        raise SystemExit("at least three repeats per leg: the spread of the repeats is the record's only noise figure")
    dev = torch.device("cuda:0")
    out = {"tool": "bench_fit_quality", "kernel_src_sha16": kernel_src_sha16(), "device": torch.cuda.get_device_name(dev),
           "cus": torch.cuda.get_device_properties(dev).multi_processor_count, "subjects": N, "thr": THR, "repeats": a.repeats,
           "unit": "milliseconds per call (all sets)", "hbm_bytes_per_s_assumed": HBM_BYTES_PER_S, "fit": {}}
    for D in a.widths:
        for n_sets in a.sets:
            xs, locs, vs, cvs, groups, mom = make_sets(D, n_sets, dev)
            kw = dict(var=vs, col_var=cvs, moments=mom, thr=THR, device=dev)
            fit, cal, rk = metrics.fit_quality(xs, locs, groups, rank=True, **kw)
            for k in sorted({0, n_sets - 1}):                     # the timed kernels compute what the yardstick computes
                h = [t[k].cpu().numpy() for t in (xs, locs, vs, cvs)]
                rf, rc = R.quality(h[0], h[1], groups[k].numpy(), h[2], h[3], mom[k].cpu().numpy(), thr=THR)
                worst = max(R.close(fit[k].cpu().numpy(), rf, "fit"), R.close(cal[k].cpu().numpy(), rc, "cal"),
                            R.close(rk[k].cpu().numpy(), R.rank(h[0], h[1], groups[k].numpy()), "rank"))
                if not worst <= 1.0:
                    raise SystemExit(f"D={D}, {n_sets} sets: set {k} differs from the yardstick ({worst} x the bound)")
            floor_ms = 24.0 * N * D * n_sets / HBM_BYTES_PER_S * 1e3
            entry = {"bytes_24ND": 24 * N * D * n_sets, "floor_ms_at_8TBps": round(floor_ms, 5)}
            iters = max(1, min(50, 2000 // n_sets))
            v = timed(lambda: metrics.fit_quality(xs, locs, groups, **kw), a.repeats, iters, dev)
            entry["quality"] = {"ms": v, "calls_per_window": iters, **stats(v), "fraction_of_24ND_at_8TBps": round(floor_ms / stats(v)["median"], 4)}
            v2 = timed(lambda: metrics.fit_quality(xs, locs, groups, rank=True, **kw), a.repeats, iters, dev)
            entry["quality_and_rank"] = {"ms": v2, "calls_per_window": iters, **stats(v2)}
            vm = timed(lambda: metrics.cohort_moments(xs, groups, ddof=0, device=dev), a.repeats, iters, dev)
            entry["cohort_moments_same_session"] = {"ms": vm, "calls_per_window": iters, **stats(vm),
                                                    "fraction_of_8ND_at_8TBps": round(floor_ms / 3.0 / stats(vm)["median"], 4)}
            iters_t = max(1, min(10, 40 // n_sets))
            vt = timed(lambda: torch_quality(xs, locs, vs, cvs, mom), a.repeats, iters_t, dev)
            entry["torch_fp64_quality"] = {"ms": vt, "calls_per_window": iters_t, **stats(vt)}
            vr = timed(lambda: torch_rank(xs, locs), a.repeats, iters_t, dev)
            entry["torch_fp64_rank"] = {"ms": vr, "calls_per_window": iters_t, **stats(vr)}
            if n_sets == a.sets[0]:                               # (the host leg is per set: measured once per width)
                h = [t[0].cpu().numpy() for t in (xs, locs, vs, cvs)]
                vh = []
                for _ in range(3):
                    t0 = time.perf_counter()
                    host_leg(*h)
                    vh.append(round((time.perf_counter() - t0) * 1e3, 2))
                entry["host_scipy_sklearn_one_set"] = {"ms": vh, **stats(vh)}
            out["fit"][f"D{D}_{n_sets}"] = entry
            print(f"D={D} x {n_sets} sets: quality {entry['quality']['median']} ms ({entry['quality']['fraction_of_24ND_at_8TBps']} of "
                  f"24ND at 8 TB/s), with rank {entry['quality_and_rank']['median']} ms, cohort_moments {entry['cohort_moments_same_session']['median']} "
                  f"ms ({entry['cohort_moments_same_session']['fraction_of_8ND_at_8TBps']} of 8ND), torch quality "
                  f"{entry['torch_fp64_quality']['median']} ms, torch rank {entry['torch_fp64_rank']['median']} ms"
                  + (f", host one set {entry['host_scipy_sklearn_one_set']['median']} ms" if "host_scipy_sklearn_one_set" in entry else ""),
                  flush=True)
            del xs, locs, vs, cvs, mom
            torch.cuda.empty_cache()
    # the clocks this run saw (bench.py --full's record), from a short traced train launch of a small set
    from bench_latent import make_set, SHAPES
    out["clocks"] = device_record(torch, nm, make_set(SHAPES["SE-3"], 1, dev), dev)
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
