#!/usr/bin/env python3
"""Operating points (metrics.operating_points -> nm_operating_points: all seven threshold rules, the summary row and the ROC
on a grid of 100 per set) timed in one session, one process, in three legs:

  kernel   metrics.operating_points on the sets as they lie on the device: the uploads of its arguments, the two launches,
           the three tables left on the device
  posthoc  metrics.posthoc_metrics on the same sets: the one rule ('roc') the device path had before, one launch
  sklearn  the reference's five rules written out over sklearn on the host (roc_curve, the f1_score loop over the 100-point
           grid, precision_recall_curve, the cost loop, the EER), average_precision_score, roc_auc_score(max_fpr=) and
           np.interp of the full curve -- after one untimed set, one pass over up to --host-sets sets, recorded per set
           with the product as `extrapolated_ms` beyond that, marked as such

Shapes: 1064 subjects split 532 / 532 (scores in (0, 1) quantised to 1/1024, the patients shifted up), 1 / 20 / 256 sets.
Kernel and posthoc legs: a warm-up call, then --repeats timed windows closed by a device synchronise; every repeat is
recorded, with min / median / max.  Before the timing the kernel's rows of the first and last set are compared with
tests/operating_point_ref.py.  No ratio is a target: everything is recorded as it comes.

One JSON document, to --out (default profiles/operating_points.json), with the clocks record of bench.py --full."""
import argparse, json, sys, time, warnings
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
from tests import operating_point_ref as R

G = 100
RULES = R.RULES


def make_sets(n_sets):
    rng = np.random.default_rng(11)
    lab = (np.arange(N) % 2).astype(np.int32)                      # 532 patients, 532 controls, interleaved
    return [((np.round(np.clip(0.4 + 0.15 * rng.standard_normal(N) + 0.1 * lab, 0.0, 1.0) * 1024) / 1024).astype(np.float32), lab)
            for _ in range(n_sets)]


def sklearn_set(s, y):
    """The reference's five rules, the two areas and the grid of one set on the host."""
    import sklearn.metrics as skm
    s = s.astype(np.float64)
    fpr, tpr, thr = skm.roc_curve(y, s)
    out = [thr[np.argmax(tpr - fpr)], thr[np.nanargmin(np.absolute((1 - tpr) - fpr))]]
    best_f1, best_cost = (0, 0), (0, np.inf)
    for v in np.linspace(0, 1, 100):
        pred = (s >= v).astype(int)
        f = skm.f1_score(y, pred)
        if f > best_f1[1]:
            best_f1 = (v, f)
        cost = np.sum((pred == 1) & (y == 0)) + np.sum((pred == 0) & (y == 1))
        if cost < best_cost[1]:
            best_cost = (v, cost)
    p, r, pthr = skm.precision_recall_curve(y, s)
    with np.errstate(invalid="ignore", divide="ignore"):
        out.append(pthr[np.argmax(2 * (p * r) / (p + r))])
    full_fpr, full_tpr, _ = skm.roc_curve(y, s, drop_intermediate=False)
    return out + [best_f1[0], best_cost[0], skm.average_precision_score(y, s), skm.roc_auc_score(y, s, max_fpr=0.1),
                  np.interp(np.linspace(0, 1, G), full_fpr, full_tpr)]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sets", nargs="+", type=int, default=[1, 20, 256])
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--host-sets", type=int, default=20, help="the most sets the sklearn leg runs in full")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "operating_points.json"))
    a = ap.parse_args()
    if a.repeats < 3:
        raise SystemExit("at least three repeats per leg: the spread of the repeats is the record's only noise figure")
    dev = torch.device("cuda:0")
    out = {"tool": "bench_operating_points", "kernel_src_sha16": kernel_src_sha16(), "device": torch.cuda.get_device_name(dev),
           "cus": torch.cuda.get_device_properties(dev).multi_processor_count, "subjects": N, "n_pos": N // 2, "n_neg": N - N // 2,
           "rules": list(RULES), "roc_grid": G, "repeats": a.repeats, "unit": "milliseconds per call (all sets)", "shapes": {}}
    for n_sets in a.sets:
        sets = make_sets(n_sets)
        sc = [torch.as_tensor(s).to(dev) for s, _ in sets]
        lb = [torch.as_tensor(l).to(dev) for _, l in sets]
        call = lambda: metrics.operating_points(sc, lb, rules=RULES, roc_grid=G, device=dev)
        got = [t.cpu().numpy() for t in call()]
        for k in sorted({0, n_sets - 1}):                          # the timed kernel computes what the restatement computes
            ref = R.operating_points([sets[k][0]], [sets[k][1]], rules=RULES, roc_grid=G)
            same = np.array_equal(got[0][k], ref[0][0], equal_nan=True) and np.allclose(got[1][k], ref[1][0], rtol=0, atol=1e-11) \
                and np.allclose(got[2][k], ref[2][0], rtol=0, atol=1e-11)
            if not same:
                raise SystemExit(f"{n_sets} sets: set {k} differs from the restatement")
        leg = {"distinct_scores_median": float(np.median(got[1][:, 5])),
               "pr_rule_on_nan": int((got[0][:, RULES.index("pr"), 7] == 1.0).sum())}
        v, iters = timed(call, a.repeats, dev)
        leg["kernel"] = {"ms": v, "calls_per_window": iters, **stats(v), "sets_per_s_median": round(n_sets / (stats(v)["median"] * 1e-3), 0)}
        v, iters = timed(lambda: metrics.posthoc_metrics(sc, lb, device=dev), a.repeats, dev)
        leg["posthoc_one_rule"] = {"ms": v, "calls_per_window": iters, **stats(v)}
        nh = min(n_sets, a.host_sets)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            sklearn_set(*sets[0])                                  # (imports and first-call set-up stay outside the window)
            t0 = time.perf_counter()
            for s, l in sets[:nh]:
                sklearn_set(s, l)
            per = (time.perf_counter() - t0) * 1e3 / nh
        leg["sklearn_host"] = {"timed_sets": nh, "ms_per_set": round(per, 2), "extrapolated": nh < n_sets,
                               ("extrapolated_ms" if nh < n_sets else "ms"): round(per * n_sets, 1)}
        out["shapes"][f"sets{n_sets}"] = leg
        print(f"{n_sets} sets: kernel (7 rules + summary + grid) {leg['kernel']['median']} ms, posthoc (1 rule) "
              f"{leg['posthoc_one_rule']['median']} ms, sklearn (host, 5 rules + areas + grid) {round(per * n_sets, 1)} ms"
              f"{' (extrapolated)' if nh < n_sets else ''}", flush=True)
    # the clocks this run saw (bench.py --full's record), from a short traced train launch of a small set
    from bench_latent import make_set, SHAPES
    out["clocks"] = device_record(torch, nm, make_set(SHAPES["SE-3"], 1, dev), dev)
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
