#!/usr/bin/env python3
"""The AUC bootstrap (metrics.auc_bootstrap -> nm_auc_bootstrap: stratified resamples of the per-subject ROC-AUC, percentile
interval, mean and standard error) timed in one session, one process, in three legs:

  kernel  metrics.auc_bootstrap on the sets as they lie on the device: the uploads of its arguments, the three launches, the
          [n_sets, 8] table left on the device
  torch   the same quantity on the same device in torch: per resample the drawn negatives sorted (one batched torch.sort),
          torch.searchsorted of the drawn positives from the left and from the right, A2* = the sum of both; then the sort of
          the A2* per set for the two order statistics, their mean and standard deviation.  All sets at once, the resamples in
          slices that keep a temporary below 2^25 elements.  The draws come from torch.randint (the same distribution, not the
          kernel's hash: torch has no unsigned 64-bit arithmetic), so this leg is timed, not compared bit by bit; its A2*
          expression is checked beforehand against the yardstick's on the yardstick's own draws.
  numpy   the yardstick tests/auc_bootstrap_ref.py on the host (uint64 hashing, np.sort + np.searchsorted per resample), one
          pass.  Up to --host-resamples resamples in all it runs in full; beyond that it is timed on that many resamples of
          the first set and recorded per resample with the product as `extrapolated_ms`, marked as such.

Shapes: 1064 subjects split 532 / 532 (scores quantised to 1/16, the patients shifted up), 1 / 20 / 256 sets, n_boot 2000 and
10000.  Kernel and torch legs: a warm-up call, then --repeats timed windows closed by a device synchronise; every repeat is
recorded, with min / median / max.  Before the timing the kernel's rows of the first and last set are compared with the
yardstick's at 130 resamples.  No ratio is a target: everything is recorded as it comes.

One JSON document, to --out (default profiles/auc_bootstrap.json), with the clocks record of bench.py --full."""
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
from bench_roi_effect import N, stats
from bench_roi_significance import timed
from tests import auc_bootstrap_ref as R

SEED, CI = 2024, 0.95
SLICE = 1 << 25                                                    # elements of one temporary of the torch leg


def make_sets(n_sets):
    rng = np.random.default_rng(7)
    lab = (np.arange(N) % 2).astype(np.int32)                      # 532 patients, 532 controls, interleaved
    return [((np.round((rng.standard_normal(N) + 0.5 * lab) * 16) / 16).astype(np.float32), lab) for _ in range(n_sets)]


def torch_a2(pv, qv):
    """A2 of the drawn positives pv [..., n_pos] against the drawn negatives qv [..., n_neg]: int64 [...]."""
    qs = torch.sort(qv, dim=-1).values
    return (torch.searchsorted(qs, pv, right=False) + torch.searchsorted(qs, pv, right=True)).sum(-1)


def torch_leg(P, Q, n_boot, lo, hi):
    """[n_sets, 5]: ci_lo, ci_hi, mean, se (over the denominator) and the observed AUC, from P [S, n_pos], Q [S, n_neg]."""
    S, n_pos, n_neg = P.shape[0], P.shape[1], Q.shape[1]
    per = max(1, SLICE // (S * max(n_pos, n_neg)))
    a2 = torch.empty(S, n_boot, dtype=torch.int64, device=P.device)
    for b0 in range(0, n_boot, per):
        b = min(per, n_boot - b0)
        ip = torch.randint(n_pos, (S, b, n_pos), device=P.device)
        iq = torch.randint(n_neg, (S, b, n_neg), device=P.device)
        pv = torch.gather(P[:, None, :].expand(S, b, n_pos), 2, ip)
        qv = torch.gather(Q[:, None, :].expand(S, b, n_neg), 2, iq)
        a2[:, b0:b0 + b] = torch_a2(pv, qv)
    den = float(2 * n_pos * n_neg)
    srt = torch.sort(a2, dim=1).values.to(torch.float64)
    f = a2.to(torch.float64)
    return torch.stack([srt[:, lo], srt[:, hi], f.mean(1), f.std(1), torch_a2(P, Q).to(torch.float64)], 1) / den


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sets", nargs="+", type=int, default=[1, 20, 256])
    ap.add_argument("--boots", nargs="+", type=int, default=[2000, 10000])
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--host-resamples", type=int, default=40000, help="the most resamples the numpy leg runs in full")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "auc_bootstrap.json"))
    a = ap.parse_args()
    if a.repeats < 3:
        raise SystemExit("at least three repeats per leg: the spread of the repeats is the record's only noise figure")
    dev = torch.device("cuda:0")
    out = {"tool": "bench_auc_bootstrap", "kernel_src_sha16": kernel_src_sha16(), "device": torch.cuda.get_device_name(dev),
           "cus": torch.cuda.get_device_properties(dev).multi_processor_count, "subjects": N, "n_pos": N // 2, "n_neg": N - N // 2,
           "boot_chunk": nm._lib.NM_BOOT_CHUNK, "seed": SEED, "ci": CI, "repeats": a.repeats,
           "unit": "milliseconds per call (all sets)", "shapes": {}}
    # the torch leg's expression against the yardstick's on the yardstick's own draws
    s0, l0 = make_sets(1)[0]
    p0, q0 = R.split(s0, l0)
    ip, iq = R.draws(len(p0), len(q0), np.arange(1, 9), SEED, 0)
    mine = torch_a2(torch.as_tensor(p0[ip]).to(dev), torch.as_tensor(q0[iq]).to(dev)).cpu().numpy()
    if not np.array_equal(mine, R.boot(s0, l0, 8, SEED, 0)):
        raise SystemExit("the torch leg's A2* differs from the yardstick's on the same draws")
    for n_sets in a.sets:
        sets = make_sets(n_sets)
        sc = [torch.as_tensor(s).to(dev) for s, _ in sets]
        lb = [torch.as_tensor(l).to(dev) for _, l in sets]
        lo, hi = R.boot_indices(130, CI)
        got = metrics.auc_bootstrap(sc, lb, n_boot=130, ci=CI, seed=SEED, device=dev).cpu().numpy()
        for k in sorted({0, n_sets - 1}):                          # the timed kernel computes what the yardstick computes
            ref = R.set_row(*sets[k], 130, lo, hi, SEED, k)
            if not (np.array_equal(got[k][[0, 1, 2, 5, 6, 7]], ref[[0, 1, 2, 5, 6, 7]]) and np.allclose(got[k][3:5], ref[3:5], rtol=1e-12, atol=0)):
                raise SystemExit(f"{n_sets} sets: set {k} differs from the yardstick")
        den_ref = 2 * (N // 2) * (N - N // 2)
        auc_ref = np.array([R.a2(*R.split(s, l)) / den_ref for s, l in sets])
        P = torch.stack([s[l != 0] for s, l in zip(sc, lb)])               # fp32, as the kernel reads them
        Q = torch.stack([s[l == 0] for s, l in zip(sc, lb)])
        for n_boot in a.boots:
            lo, hi = R.boot_indices(n_boot, CI)
            leg = {"resamples": n_sets * n_boot,
                   "workspace_mib": round(nm._lib.load().nm_auc_bootstrap_workspace(n_sets, N, n_boot, 0) / 2 ** 20, 2)}
            call = lambda: metrics.auc_bootstrap(sc, lb, n_boot=n_boot, ci=CI, seed=SEED, device=dev)
            v, iters = timed(call, a.repeats, dev)
            leg["kernel"] = {"ms": v, "calls_per_window": iters, **stats(v),
                             "resamples_per_s_median": round(leg["resamples"] / (stats(v)["median"] * 1e-3), 0)}
            tl = lambda: torch_leg(P, Q, n_boot, lo, hi)
            kt, tt = call().cpu().numpy(), tl().cpu().numpy()
            # every set's observed AUC against the yardstick's: the kernel's bits; the torch leg's A2 (torch divides by a
            # scalar through its reciprocal on the device, so its quotient may be an ulp off)
            for name, bad in (("kernel", kt[:, 0] != auc_ref), ("torch leg", np.rint(tt[:, 4] * den_ref) != np.rint(auc_ref * den_ref))):
                if bad.any():
                    raise SystemExit(f"{n_sets} sets x {n_boot}: the {name}'s observed AUC differs from the yardstick's in sets "
                                     f"{np.flatnonzero(bad)[:8].tolist()}")
            leg["interval_width_kernel_over_torch_median"] = round(float(np.median((kt[:, 2] - kt[:, 1]) / (tt[:, 1] - tt[:, 0]))), 4)
            v, iters = timed(tl, a.repeats, dev)
            leg["torch_device"] = {"ms": v, "calls_per_window": iters, **stats(v)}
            total = n_sets * n_boot
            t0 = time.perf_counter()
            if total <= a.host_resamples:
                for k, (s, l) in enumerate(sets):
                    R.set_row(s, l, n_boot, lo, hi, SEED, k)
                ms = (time.perf_counter() - t0) * 1e3
                leg["numpy_host"] = {"ms": round(ms, 1), "ms_per_resample": round(ms / total, 4), "extrapolated": False}
            else:
                nb = min(n_boot, a.host_resamples)
                R.set_row(*sets[0], nb, *R.boot_indices(nb, CI), SEED, 0)
                per = (time.perf_counter() - t0) * 1e3 / nb
                leg["numpy_host"] = {"timed_resamples": nb, "ms_per_resample": round(per, 4), "extrapolated_ms": round(per * total, 0),
                                     "extrapolated": True}
            out["shapes"][f"sets{n_sets}_boot{n_boot}"] = leg
            host = leg["numpy_host"]
            print(f"{n_sets} sets x {n_boot} resamples: kernel {leg['kernel']['median']} ms, torch (device) {leg['torch_device']['median']} ms, "
                  f"numpy (host) {host.get('ms', host.get('extrapolated_ms'))} ms{' (extrapolated)' if host['extrapolated'] else ''}", flush=True)
            torch.cuda.empty_cache()
    # the clocks this run saw (bench.py --full's record), from a short traced train launch of a small set
    from bench_latent import make_set, SHAPES
    out["clocks"] = device_record(torch, nm, make_set(SHAPES["SE-3"], 1, dev), dev)
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
