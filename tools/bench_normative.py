#!/usr/bin/env python3
"""Normative z-maps (metrics.cohort_moments / normative_z -> nm_cohort_moments / nm_normative_z) and the latent Mahalanobis
distance (metrics.cohort_cov / mahalanobis -> nm_cohort_cov / nm_mahalanobis) timed in one session, one process, three ways on
the same data:

  kernel   one launch for all sets per entry point (pointer table, tables read where they lie)
  torch    the same quantities as fp64 torch expressions on the same device, the sets one after another: mean / var of the
           controls, (x - mean) / sd, the counts beyond the threshold per row and per column and group; torch.cov,
           torch.linalg.cholesky and solve_triangular for the distance
  numpy    the yardstick of the tests (tests/normative_ref.py) on the host, on copies made beforehand

for 1064 subjects, 532 controls against 532 patients, D = 379 (one modality) and D = 1137 (the early-fusion table) for the
z-map, Z = 10 and 64 for the distance, with 1, 20 and 256 sets (every set a table of its own).  Each leg: a warm-up call, then
--repeats timed windows of some calls each, every window closed by a device synchronise; every repeat is recorded, with min /
median / max.  Before the timing the kernel's first and last set are compared with the yardstick's.  The moments and the z pass
are also given as the fraction of the time 8 N D bytes per set take at 8 TB/s (the moments pass reads its 4 N D bytes twice,
the z pass reads them in both of its kernels, or once and writes 4 N D).  No ratio is a target: all legs are recorded as they come.

One JSON document, to --out (default profiles/normative.json), with the clocks record of bench.py --full."""
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
from tests import normative_ref as R

N = 1064
THR = 1.96
HBM_BYTES_PER_S = 8e12


def make_sets(D, n_sets, dev):
    g = torch.Generator(device=dev).manual_seed(1000 * D + n_sets)
    pitch = (D + 3) // 4 * 4                                      # the evaluation jobs' out_sqerr pitch
    bufs = [torch.randn(N, pitch, device=dev, generator=g) ** 2 for _ in range(n_sets)]
    group = (torch.arange(N) % 2).to(torch.int32)               # 532 controls, 532 patients, interleaved
    return [b[:, :D] for b in bufs], [group] * n_sets


def torch_zmap(mats, group, dev):
    ref, pat = (group == 0).to(dev), (group == 1).to(dev)
    keep = None
    for m in mats:
        v = m.double()
        mean, sd = v[ref].mean(0), v[ref].std(0, unbiased=True)
        z = (v - mean) / sd
        hi, lo = z > THR, z < -THR
        keep = (z.float(), hi.sum(1), lo.sum(1), z.mean(1), z.abs().mean(1), z.max(1), hi[pat].sum(0), lo[pat].sum(0), hi[ref].sum(0),
                lo[ref].sum(0), z[pat].mean(0), z[ref].mean(0))
    return keep


def torch_maha(mats, group, dev):
    ref = (group == 0).to(dev)
    keep = None
    for m in mats:
        v = m.double()
        mean = v[ref].mean(0)
        L = torch.linalg.cholesky(torch.atleast_2d(torch.cov(v[ref].T)))
        y = torch.linalg.solve_triangular(L, (v - mean).T, upper=False)
        keep = (y * y).sum(0).sqrt()
    return keep


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--widths", nargs="+", type=int, default=[379, 1137])
    ap.add_argument("--latents", nargs="+", type=int, default=[10, 64])
    ap.add_argument("--sets", nargs="+", type=int, default=[1, 20, 256])
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "normative.json"))
    a = ap.parse_args()
    if a.repeats < 3:
        raise SystemExit("at least three repeats per leg: the spread of the repeats is the record's only noise figure")
    dev = torch.device("cuda:0")
    out = {"tool": "bench_normative", "kernel_src_sha16": kernel_src_sha16(), "device": torch.cuda.get_device_name(dev),
           "cus": torch.cuda.get_device_properties(dev).multi_processor_count, "subjects": N, "n_ref": N - N // 2, "n_patients": N // 2,
           "thr": THR, "repeats": a.repeats, "unit": "milliseconds per call (all sets)", "hbm_bytes_per_s_assumed": HBM_BYTES_PER_S,
           "zmap": {}, "mahalanobis": {}}
    for D in a.widths:
        for n_sets in a.sets:
            mats, groups = make_sets(D, n_sets, dev)
            mom = metrics.cohort_moments(mats, groups, device=dev)
            z, rows, cols = metrics.normative_z(mats, groups, mom, thr=THR, device=dev)
            rows_k = torch.split(rows, [N] * n_sets)
            for k in sorted({0, n_sets - 1}):                     # the timed kernels compute what the yardstick computes
                x, g = mats[k].cpu().numpy(), groups[k].numpy()
                rm = R.moments(x, g)
                rz = R.z_table(x, rm)
                worst = max(R.close(mom[k].cpu().numpy(), rm, "moments"), R.close(z[k].cpu().numpy(), rz, "z32"),
                            R.close(rows_k[k].cpu().numpy(), R.row_summary(rz, THR), "rows"),
                            R.close(cols[k].cpu().numpy(), R.col_summary(rz, g, rm, THR), "cols"))
                if not worst <= 1.0:
                    raise SystemExit(f"D={D}, {n_sets} sets: set {k} differs from the yardstick ({worst} x the bound)")
            floor_ms = 8.0 * N * D * n_sets / HBM_BYTES_PER_S * 1e3
            entry = {"bytes_8ND": 8 * N * D * n_sets, "floor_ms_at_8TBps": round(floor_ms, 5)}
            iters = max(1, min(50, 2000 // n_sets))
            for name, fn in (("moments", lambda: metrics.cohort_moments(mats, groups, device=dev)),
                             ("z_with_table", lambda: metrics.normative_z(mats, groups, mom, thr=THR, device=dev)),
                             ("z_without_table", lambda: metrics.normative_z(mats, groups, mom, thr=THR, return_z=False, device=dev))):
                v = timed(fn, a.repeats, iters, dev)
                entry[name] = {"ms": v, "calls_per_window": iters, **stats(v),
                               "fraction_of_8ND_at_8TBps": round(floor_ms / stats(v)["median"], 4)}
            iters_t = max(1, min(10, 40 // n_sets))
            v = timed(lambda: torch_zmap(mats, groups[0], dev), a.repeats, iters_t, dev)
            entry["torch_fp64"] = {"ms": v, "calls_per_window": iters_t, **stats(v)}
            host = [(m.cpu().numpy(), g.numpy()) for m, g in zip(mats, groups)]
            v = []
            for _ in range(a.repeats if n_sets <= 20 else 1):    # (256 sets: one pass, it takes the longest by far)
                t0 = time.perf_counter()
                for x, g in host:
                    rm = R.moments(x, g)
                    rz = R.z_table(x, rm)
                    R.row_summary(rz, THR), R.col_summary(rz, g, rm, THR)
                v.append(round((time.perf_counter() - t0) * 1e3, 2))
            entry["numpy_host"] = {"ms": v, **stats(v)}
            out["zmap"][f"D{D}_{n_sets}"] = entry
            print(f"D={D} x {n_sets} sets: moments {entry['moments']['median']} ms, z {entry['z_with_table']['median']} ms "
                  f"(no table {entry['z_without_table']['median']} ms), torch {entry['torch_fp64']['median']} ms, numpy "
                  f"{entry['numpy_host']['median']} ms; floor {floor_ms:.4f} ms", flush=True)
            del mats, host, z
            torch.cuda.empty_cache()
    for Z in a.latents:
        for n_sets in a.sets:
            g = torch.Generator(device=dev).manual_seed(77 * Z + n_sets)
            mats = [torch.randn(N, Z, device=dev, generator=g) for _ in range(n_sets)]
            group = (torch.arange(N) % 2).to(torch.int32)
            groups = [group] * n_sets
            mean, chol, st = metrics.cohort_cov(mats, groups, device=dev)
            d = metrics.mahalanobis(mats, mean, chol, st, device=dev)
            for k in sorted({0, n_sets - 1}):
                x = mats[k].cpu().numpy()
                want = np.sqrt(R.mahalanobis(x, *R.cov_chol(x, group.numpy())))
                if not R.close(d[k].cpu().numpy(), want, "rel") <= 1.0:
                    raise SystemExit(f"Z={Z}, {n_sets} sets: set {k} differs from the yardstick")
            entry = {}
            iters = max(1, min(50, 2000 // n_sets))
            for name, fn in (("cov", lambda: metrics.cohort_cov(mats, groups, device=dev)),
                             ("distance", lambda: metrics.mahalanobis(mats, mean, chol, st, device=dev))):
                v = timed(fn, a.repeats, iters, dev)
                entry[name] = {"ms": v, "calls_per_window": iters, **stats(v)}
            iters_t = max(1, min(10, 40 // n_sets))
            v = timed(lambda: torch_maha(mats, group, dev), a.repeats, iters_t, dev)
            entry["torch_fp64"] = {"ms": v, "calls_per_window": iters_t, **stats(v)}
            host = [m.cpu().numpy() for m in mats]
            v = []
            for _ in range(a.repeats if n_sets <= 20 else 1):
                t0 = time.perf_counter()
                for x in host:
                    R.mahalanobis(x, *R.cov_chol(x, group.numpy()))
                v.append(round((time.perf_counter() - t0) * 1e3, 2))
            entry["numpy_host"] = {"ms": v, **stats(v)}
            out["mahalanobis"][f"Z{Z}_{n_sets}"] = entry
            print(f"Z={Z} x {n_sets} sets: cov {entry['cov']['median']} ms, distance {entry['distance']['median']} ms, torch "
                  f"{entry['torch_fp64']['median']} ms, numpy {entry['numpy_host']['median']} ms", flush=True)
            del mats, host
            torch.cuda.empty_cache()
    # the clocks this run saw (bench.py --full's record), from a short traced train launch of a small set
    from bench_latent import make_set, SHAPES
    out["clocks"] = device_record(torch, nm, make_set(SHAPES["SE-3"], 1, dev), dev)
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
