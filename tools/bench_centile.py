#!/usr/bin/env python3
"""Normative centiles (metrics.cohort_quantiles / normative_centile -> nm_cohort_quantiles / nm_normative_centile) timed in one
session, one process, three ways on the same data:

  kernel   one call for all sets per entry point (pointer table, tables read where they lie)
  torch    the same quantities as fp64 torch expressions on the same device, the sets one after another: torch.sort of the
           controls' columns, torch.quantile and the medians for the curve, torch.searchsorted (left and right) of every row
           for the percentile rank, the counts in the tails per row and per column and group
  numpy    the yardstick of the tests (tests/centile_ref.py) on the host, on copies made beforehand

for 1064 subjects, 532 controls against 532 patients, D = 379 (one modality) and D = 1137 (the early-fusion table), with 1, 20
and 256 sets (every set a table of its own).  Each leg: a warm-up call, then --repeats timed windows of some calls each, every
window closed by a device synchronise; every repeat is recorded, with min / median / max.  Before the timing the kernel's first
and last set are compared with the yardstick's, bit for bit.  The numpy leg runs up to --numpy-max-sets sets (a pass over 256
sets takes minutes); a leg that was not run is recorded as "not measured".  No ratio is a target: all legs are recorded as
they come.

One JSON document, to --out (default profiles/normative_centile.json), with the clocks record of bench.py --full."""
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
from bench_normative import make_sets
from tests import centile_ref as R
from tests.table_stats_util import same_bits

N = 1064
TAIL = 2.5
PROBS = (0.05, 0.25, 0.5, 0.75, 0.95)


def torch_centile(mats, group, dev):
    ref, pat = (group == 0).to(dev), (group == 1).to(dev)
    probs = torch.tensor(PROBS, dtype=torch.float64, device=dev)
    keep = None
    for m in mats:
        v = m.double()
        a = torch.sort(v[ref], dim=0).values                       # [n, D]
        n = a.shape[0]
        q = torch.quantile(a, probs, dim=0)
        med = a.median(0).values
        mad = (v[ref] - med).abs().median(0).values
        at, vt = a.T.contiguous(), v.T.contiguous()                # searchsorted works along the last axis
        k2 = torch.searchsorted(at, vt, right=False) + torch.searchsorted(at, vt, right=True)
        pct = (k2.double() * (50.0 / n)).T
        hi, lo = pct > 100.0 - TAIL, pct < TAIL
        keep = (q, med, mad, pct.float(), hi.sum(1), lo.sum(1), pct.mean(1), (pct - 50.0).abs().mean(1), pct.max(1), hi[pat].sum(0),
                lo[pat].sum(0), hi[ref].sum(0), lo[ref].sum(0), pct[pat].mean(0), pct[ref].mean(0))
    return keep


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--widths", nargs="+", type=int, default=[379, 1137])
    ap.add_argument("--sets", nargs="+", type=int, default=[1, 20, 256])
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--numpy-max-sets", dest="numpy_max_sets", type=int, default=20)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "normative_centile.json"))
    a = ap.parse_args()
    if a.repeats < 3:
        raise SystemExit("at least three repeats per leg: the spread of the repeats is the record's only noise figure")
    dev = torch.device("cuda:0")
    out = {"tool": "bench_centile", "kernel_src_sha16": kernel_src_sha16(), "device": torch.cuda.get_device_name(dev),
           "cus": torch.cuda.get_device_properties(dev).multi_processor_count, "subjects": N, "n_ref": N - N // 2, "n_patients": N // 2,
           "tail": TAIL, "probs": list(PROBS), "repeats": a.repeats, "unit": "milliseconds per call (all sets)", "centile": {}}
    for D in a.widths:
        for n_sets in a.sets:
            mats, groups = make_sets(D, n_sets, dev)
            q, st = metrics.cohort_quantiles(mats, groups, PROBS, device=dev)
            pct, rows, cols = metrics.normative_centile(mats, groups, tail=TAIL, device=dev)
            rows_k = torch.split(rows, [N] * n_sets)
            for k in sorted({0, n_sets - 1}):                     # the timed kernels compute what the yardstick computes
                x, g = mats[k].cpu().numpy(), groups[k].numpy()
                wq, wst = R.cohort_quantiles(x, g, PROBS)
                wpct, wrows, wcols = R.normative_centile([(x, g, None)], None, TAIL, False)[0]
                if not (same_bits(q[k].cpu().numpy(), wq) and same_bits(st[k].cpu().numpy(), wst) and
                        same_bits(pct[k].cpu().numpy(), wpct) and same_bits(rows_k[k].cpu().numpy(), wrows) and
                        same_bits(cols[k].cpu().numpy(), wcols)):
                    raise SystemExit(f"D={D}, {n_sets} sets: set {k} differs from the yardstick")
            entry = {}
            iters = max(1, min(50, 2000 // n_sets))
            for name, fn in (("quantiles", lambda: metrics.cohort_quantiles(mats, groups, PROBS, device=dev)),
                             ("centile_with_table", lambda: metrics.normative_centile(mats, groups, tail=TAIL, device=dev)),
                             ("centile_without_table", lambda: metrics.normative_centile(mats, groups, tail=TAIL, return_table=False, device=dev)),
                             ("centile_loo", lambda: metrics.normative_centile(mats, groups, tail=TAIL, loo=True, device=dev))):
                v = timed(fn, a.repeats, iters, dev)
                entry[name] = {"ms": v, "calls_per_window": iters, **stats(v)}
            iters_t = max(1, min(10, 40 // n_sets))
            v = timed(lambda: torch_centile(mats, groups[0], dev), a.repeats, iters_t, dev)
            entry["torch_fp64"] = {"ms": v, "calls_per_window": iters_t, **stats(v)}
            if n_sets <= a.numpy_max_sets:
                host = [(m.cpu().numpy(), g.numpy()) for m, g in zip(mats, groups)]
                v = []
                for _ in range(a.repeats if n_sets == 1 else 1):
                    t0 = time.perf_counter()
                    for x, g in host:
                        R.cohort_quantiles(x, g, PROBS)
                        R.normative_centile([(x, g, None)], None, TAIL, False)
                    v.append(round((time.perf_counter() - t0) * 1e3, 2))
                entry["numpy_host"] = {"ms": v, **stats(v)}
                del host
            else:
                entry["numpy_host"] = "not measured"
            out["centile"][f"D{D}_{n_sets}"] = entry
            np_ms = entry["numpy_host"]["median"] if isinstance(entry["numpy_host"], dict) else "not measured"
            print(f"D={D} x {n_sets} sets: quantiles {entry['quantiles']['median']} ms, centile {entry['centile_with_table']['median']} ms "
                  f"(no table {entry['centile_without_table']['median']} ms, loo {entry['centile_loo']['median']} ms), torch "
                  f"{entry['torch_fp64']['median']} ms, numpy {np_ms} ms", flush=True)
            del mats, pct
            torch.cuda.empty_cache()
    # the clocks this run saw (bench.py --full's record), from a short traced train launch of a small set
    from bench_latent import make_set, SHAPES
    out["clocks"] = device_record(torch, nm, make_set(SHAPES["SE-3"], 1, dev), dev)
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
