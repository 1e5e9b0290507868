#!/usr/bin/env python3
"""ROI-wise group effect sizes (Cliff's delta / ROC-AUC per ROI, metrics.roi_effect -> nm_roi_effect) timed in one session,
one process, three ways on the same data:

  kernel   metrics.roi_effect: one launch for all sets (pointer table, tables read where they lie)
  torch    the broadcast expression on the same device, per set and per direction
               (x[:, None, :] > y[None, :, :]).sum((0, 1))   and the same with <
           -- its boolean temporary has n_x n_y D bytes; the leg runs only where that fits (--torch-temp-limit), the sets one
           after another so that one temporary is alive at a time
  numpy    the yardstick of the tests (tests/roi_effect_ref.py, the sort-based counts) on the host, on copies made beforehand

for 1064 subjects split evenly into patients and controls, D = 379 (one modality) and D = 1137 (the early-fusion table), with
1, 20 and 256 sets (every set a table of its own: squares of values quantised to 1/4, as the tests use).  Each leg: a
warm-up call, then --repeats timed windows of some calls each, every window closed by a device synchronise; every repeat is
recorded, with min / median / max.  Before the timing the kernel's counts of the first and the last set are compared with the
yardstick's.  No ratio is a target: all three are recorded as they come.

One JSON document, to --out (default profiles/roi_effect.json), with the clocks record of bench.py --full."""
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
from tests import roi_effect_ref as R

N = 1064


def stats(v):
    s = sorted(v)
    return {"min": s[0], "median": round((s[(len(s) - 1) // 2] + s[len(s) // 2]) / 2, 3), "max": s[-1]}


def make_sets(D, n_sets, dev):
    g = torch.Generator(device=dev).manual_seed(1000 * D + n_sets)
    pitch = (D + 3) // 4 * 4                                      # the evaluation jobs' out_sqerr pitch
    bufs = [(torch.round(torch.randn(N, pitch, device=dev, generator=g) * 4) / 4) ** 2 for _ in range(n_sets)]
    group = (torch.arange(N) % 2).to(torch.int32)               # 532 patients, 532 controls, interleaved
    return [b[:, :D] for b in bufs], [group] * n_sets


def timed(fn, repeats, iters, dev):
    fn()
    torch.cuda.synchronize(dev)
    out = []
    for _ in range(repeats):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        for _ in range(iters):
            fn()
        torch.cuda.synchronize(dev)
        out.append(round((time.perf_counter() - t0) / iters * 1e3, 4))
    return out


def torch_leg(mats, group, dev):
    gx, gy = (group == 1).to(dev), (group == 0).to(dev)
    keep = None
    for m in mats:
        x, y = m[gx], m[gy]
        more = (x[:, None, :] > y[None, :, :]).sum((0, 1))
        less = (x[:, None, :] < y[None, :, :]).sum((0, 1))
        keep = (more, less)
    return keep


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--widths", nargs="+", type=int, default=[379, 1137])
    ap.add_argument("--sets", nargs="+", type=int, default=[1, 20, 256])
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--torch-temp-limit", type=float, default=2.0, help="GiB the broadcast expression's temporary may take")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "roi_effect.json"))
    a = ap.parse_args()
    if a.repeats < 3:
        raise SystemExit("at least three repeats per leg: the spread of the repeats is the record's only noise figure")
    dev = torch.device("cuda:0")
    out = {"tool": "bench_roi_effect", "kernel_src_sha16": kernel_src_sha16(), "device": torch.cuda.get_device_name(dev),
           "cus": torch.cuda.get_device_properties(dev).multi_processor_count, "subjects": N, "n_x": N // 2, "n_y": N - N // 2,
           "y_chunk": nm._lib.NM_ROI_Y_CHUNK, "repeats": a.repeats, "unit": "milliseconds per call (all sets)", "shapes": {}}
    for D in a.widths:
        for n_sets in a.sets:
            mats, groups = make_sets(D, n_sets, dev)
            got = metrics.roi_effect(mats, groups, device=dev).cpu().numpy()
            for k in sorted({0, n_sets - 1}):                     # the timed kernel computes what the yardstick computes
                ref = R.table(mats[k].cpu().numpy(), groups[k].numpy(), R.counts_sorted)
                if not (np.array_equal(got[k][:, 2:6], ref[:, 2:6]) and np.array_equal(got[k][:, :2], ref[:, :2])):
                    raise SystemExit(f"D={D}, {n_sets} sets: set {k} differs from the yardstick")
            pairs = (N // 2) * (N - N // 2) * D * n_sets
            entry = {"pairs": pairs}
            iters = max(1, min(50, 2000 // n_sets))
            v = timed(lambda: metrics.roi_effect(mats, groups, device=dev), a.repeats, iters, dev)
            entry["kernel"] = {"ms": v, "calls_per_window": iters, **stats(v),
                               "pairs_per_s_median": round(pairs / (stats(v)["median"] * 1e-3), 0)}
            temp_gib = (N // 2) * (N - N // 2) * D / 2 ** 30
            if temp_gib <= a.torch_temp_limit:
                iters_t = max(1, min(10, 40 // n_sets))
                v = timed(lambda: torch_leg(mats, groups[0], dev), a.repeats, iters_t, dev)
                entry["torch_broadcast"] = {"ms": v, "calls_per_window": iters_t, "temporary_gib": round(temp_gib, 3), **stats(v)}
            else:
                entry["torch_broadcast"] = {"skipped": f"temporary of {temp_gib:.2f} GiB above the limit"}
            host = [(m.cpu().numpy(), g.numpy()) for m, g in zip(mats, groups)]
            v = []
            for _ in range(a.repeats if n_sets <= 20 else 1):    # (256 sets: one pass, it takes the longest by far)
                t0 = time.perf_counter()
                for x, g in host:
                    R.table(x, g, R.counts_sorted)
                v.append(round((time.perf_counter() - t0) * 1e3, 2))
            entry["numpy_sorted_host"] = {"ms": v, **stats(v)}
            out["shapes"][f"D{D}_{n_sets}"] = entry
            tb = entry["torch_broadcast"].get("median")
            print(f"D={D} x {n_sets} sets: kernel {entry['kernel']['median']} ms, torch {tb} ms, numpy {entry['numpy_sorted_host']['median']} ms",
                  flush=True)
            del mats, host
            torch.cuda.empty_cache()
    # the clocks this run saw (bench.py --full's record), from a short traced train launch of a small set
    from bench_latent import make_set, SHAPES
    out["clocks"] = device_record(torch, nm, make_set(SHAPES["SE-3"], 1, dev), dev)
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
