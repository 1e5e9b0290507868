#!/usr/bin/env python3
"""ROI-wise significance (metrics.roi_significance -> nm_roi_significance: Mann-Whitney p, Benjamini-Hochberg q, max-statistic
label permutations) timed in one session, one process, in three legs on the same data:

  n_perm = 0        the asymptotic pass alone (rank pass, z / p, the BH sort)
  n_perm = 1000     ... and the label, sum and closing passes
  n_perm = 10000

against two yardsticks:

  scipy   scipy.stats.mannwhitneyu(X, Y, axis=0, method='asymptotic') + false_discovery_control on the host, on copies made
          beforehand, for the first leg
  matmul  for the other two, on the same device: per set  labels (fp64 [n_perm, n]) @ r2 (fp64 [n, D])  - n_x (n + 1), then
          the two comparisons (|S*| >= |S| summed over permutations; the row maximum of |S*| >= |S|).  Exact: the sums stay
          below 2^53.  The labels and r2 are the yardstick's (tests/roi_significance_ref.py), uploaded beforehand, so the
          matmul leg pays for neither the ranks nor the permutations -- the kernel's time includes both.

for 1064 subjects split 532 / 532, D = 379 (one modality) and D = 1137 (the early-fusion table), with 1 and 20 sets (every set
a table of its own: squares of values quantised to 1/4, as the tests use).  Each leg: a warm-up call, then --repeats timed
windows of some calls each, every window closed by a device synchronise; every repeat is recorded, with min / median / max.
Before the timing the kernel's table is compared with the yardstick's (n_perm = 0: first and last set) and its permutation
counts with the matmul leg's (every set).  No ratio is a target: everything is recorded as it comes.

One JSON document, to --out (default profiles/roi_significance.json), with the clocks record of bench.py --full."""
import argparse, json, sys, time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))
import numpy as np
import scipy.stats
import torch
import multi_modal_normative_modeling_amd as nm
from multi_modal_normative_modeling_amd import metrics
from bench import device_record, kernel_src_sha16
from bench_roi_effect import N, make_sets, stats
from tests import roi_significance_ref as R

SEED = 2024


def timed(fn, repeats, dev, window_s=0.25):
    """A warm-up call (timed on its own to size the windows), then `repeats` windows closed by a synchronise."""
    fn()
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize(dev)
    iters = int(max(1, min(50, window_s / max(time.perf_counter() - t0, 1e-6))))
    out = []
    for _ in range(repeats):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        for _ in range(iters):
            fn()
        torch.cuda.synchronize(dev)
        out.append(round((time.perf_counter() - t0) / iters * 1e3, 4))
    return out, iters


def matmul_leg(labels, r2, absS, center):
    """Per set the two permutation counts [D] from the fp64 product; returns them stacked [n_sets, 2, D]."""
    res = []
    for lab, r, a in zip(labels, r2, absS):
        sp = (lab @ r - center).abs()
        res.append(torch.stack([(sp >= a).sum(0), (sp.max(1).values[:, None] >= a).sum(0)]))
    return torch.stack(res)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--widths", nargs="+", type=int, default=[379, 1137])
    ap.add_argument("--sets", nargs="+", type=int, default=[1, 20])
    ap.add_argument("--perms", nargs="+", type=int, default=[0, 1000, 10000])
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "roi_significance.json"))
    a = ap.parse_args()
    if a.repeats < 3:
        raise SystemExit("at least three repeats per leg: the spread of the repeats is the record's only noise figure")
    dev = torch.device("cuda:0")
    n_x = N // 2
    out = {"tool": "bench_roi_significance", "kernel_src_sha16": kernel_src_sha16(), "device": torch.cuda.get_device_name(dev),
           "cus": torch.cuda.get_device_properties(dev).multi_processor_count, "subjects": N, "n_x": n_x, "n_y": N - n_x,
           "perm_chunk": nm._lib.NM_ROI_PERM_CHUNK, "row_chunk": nm._lib.NM_ROI_ROW_CHUNK, "seed": SEED, "repeats": a.repeats,
           "unit": "milliseconds per call (all sets)", "shapes": {}}
    # the permutations of set k do not depend on the table: the yardstick's labels once, for the most sets and permutations
    pmax, smax = max(a.perms), max(a.sets)
    lab_host = [R.labels(N, n_x, pmax, SEED, k).astype(np.int8) for k in range(smax)] if pmax else []
    for D in a.widths:
        for n_sets in a.sets:
            mats, groups = make_sets(D, n_sets, dev)
            host = [(m.cpu().numpy(), g.numpy()) for m, g in zip(mats, groups)]
            parts = [R.parts(x, g) for x, g in host]
            entry = {}
            for n_perm in a.perms:
                call = lambda: metrics.roi_significance(mats, groups, n_perm=n_perm, seed=SEED, device=dev)
                got = call().cpu().numpy()
                leg = {"rank_sums": n_perm * N * D * n_sets,
                       "workspace_mib": round(nm._lib.load().nm_roi_significance_workspace(n_sets, D, N, n_perm) / 2 ** 20, 1)}
                if n_perm == 0:
                    for k in sorted({0, n_sets - 1}):             # the timed kernel computes what the yardstick computes
                        ref = R.table(*host[k])
                        if not (np.array_equal(got[k][:, :3], ref[:, :3]) and np.allclose(got[k][:, 3:5], ref[:, 3:5], rtol=1e-12, atol=0)):
                            raise SystemExit(f"D={D}, {n_sets} sets: set {k} differs from the yardstick")
                    v = []
                    for _ in range(a.repeats):
                        t0 = time.perf_counter()
                        for x, g in host:
                            p = scipy.stats.mannwhitneyu(x[g == 1], x[g == 0], alternative="two-sided", method="asymptotic", axis=0).pvalue
                            scipy.stats.false_discovery_control(p, method="bh")
                        v.append(round((time.perf_counter() - t0) * 1e3, 2))
                    leg["scipy_host"] = {"ms": v, **stats(v)}
                else:
                    labels = [torch.as_tensor(lab_host[k][:n_perm], dtype=torch.float64).to(dev) for k in range(n_sets)]
                    r2 = [torch.as_tensor(P["r2"], dtype=torch.float64).to(dev) for P in parts]
                    absS = [torch.as_tensor(np.abs(P["S"]), dtype=torch.float64).to(dev) for P in parts]
                    mm = lambda: matmul_leg(labels, r2, absS, float(n_x * (N + 1)))
                    cnt = mm().cpu().numpy()
                    if not (np.array_equal(got[:, :, 5], (1 + cnt[:, 0]) / (1 + n_perm)) and np.array_equal(got[:, :, 6], (1 + cnt[:, 1]) / (1 + n_perm))):
                        raise SystemExit(f"D={D}, {n_sets} sets, {n_perm} permutations: the kernel's counts differ from the matmul leg's")
                    v, iters = timed(mm, a.repeats, dev)
                    leg["matmul_fp64_device"] = {"ms": v, "calls_per_window": iters, **stats(v)}
                    del labels, r2, absS
                v, iters = timed(call, a.repeats, dev)
                leg["kernel"] = {"ms": v, "calls_per_window": iters, **stats(v)}
                if n_perm:
                    leg["kernel"]["rank_sums_per_s_median"] = round(leg["rank_sums"] / (stats(v)["median"] * 1e-3), 0)
                entry[f"perm{n_perm}"] = leg
                other = leg.get("scipy_host", leg.get("matmul_fp64_device"))
                print(f"D={D} x {n_sets} sets, n_perm {n_perm}: kernel {leg['kernel']['median']} ms, "
                      f"{'scipy (host)' if n_perm == 0 else 'fp64 matmul (device)'} {other['median']} ms", flush=True)
                torch.cuda.empty_cache()
            out["shapes"][f"D{D}_{n_sets}"] = entry
            del mats, host, parts
    # the clocks this run saw (bench.py --full's record), from a short traced train launch of a small set
    from bench_latent import make_set, SHAPES
    out["clocks"] = device_record(torch, nm, make_set(SHAPES["SE-3"], 1, dev), dev)
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
