"""numpy restatement of nm_operating_points (include/nmhip.h has the definitions): every threshold rule, the summary row
and the ROC on a grid, in the layout metrics.operating_points returns.

The rules are those of multimodal_kfold_cvae_group_analysis_1x1.py: 'roc' :129-132, 'f1' :63-75, 'pr' :77-81, 'cost' :83-97,
'eer' :99-103, the prediction `score >= threshold` :144 and the four counts :147-153 -- restated on the counts of the
distinct-score curve (sklearn's _binary_clf_curve) instead of on calls into sklearn, so that
tests/test_operating_point_ref_cpu.py can hold this file to sklearn 1.7 and to the rules written out with sklearn's
functions, and tests/test_gpu_operating_points.py can hold the kernels to this file.  Scores are fp32 promoted to fp64; -0 and
+0 are one threshold (+0).  Counts are integers until the divisions, which are single fp64 divisions of exact integers.
"""
import math

import numpy as np

COLUMNS = ("threshold", "accuracy", "recall", "specificity", "tp", "fp", "objective", "status")
SUMMARY = ("roc_auc", "average_precision", "pauc", "sens_at_spec", "spec_at_sens", "n_thresholds", "n_pos", "n_neg")
RULES = ("roc", "f1", "pr", "cost", "eer", "f1max", "spec")
MAX_N = 8192


def as_scores(scores):
    return np.asarray(scores, dtype=np.float32).astype(np.float64).reshape(-1) + 0.0          # (-0 + 0 = +0)


def as_labels(labels):
    return (np.asarray(labels).reshape(-1) != 0)


class Curve:
    """thr[j], tps[j], fps[j], j = 0..K-1: the distinct scores from the top with the counts of `score >= thr[j]`."""

    def __init__(self, scores, labels):
        s, y = as_scores(scores), as_labels(labels)
        self.n = int(s.size)
        self.P = int(y.sum())
        self.N = self.n - self.P
        self.valid = 1 <= self.n <= MAX_N and not bool(np.isnan(s).any()) and self.P > 0 and self.N > 0
        if not self.valid:
            return
        order = np.argsort(-s, kind="stable")
        s, y = s[order], y[order]
        last = np.r_[np.nonzero(s[1:] != s[:-1])[0], s.size - 1]          # the last member of every run of equal scores
        self.thr = s[last]
        self.tps = np.cumsum(y.astype(np.int64))[last]
        self.fps = last + 1 - self.tps
        self.K = int(last.size)
        self.kept = np.ones(self.K, dtype=bool)                            # roc_curve's drop_intermediate (len > 2 only)
        if self.K > 2:
            self.kept[1:-1] = (np.diff(self.fps, 2) != 0) | (np.diff(self.tps, 2) != 0)

    def counts_at(self, theta):
        """(tp, fp) of `score >= theta` for an array of thresholds."""
        k = np.searchsorted(-self.thr, -np.asarray(theta, dtype=np.float64), side="right")   # how many thr >= theta
        tp = np.where(k > 0, self.tps[np.maximum(k, 1) - 1], 0)
        fp = np.where(k > 0, self.fps[np.maximum(k, 1) - 1], 0)
        return tp, fp


def select(c, rule, grid=(0.0, 1.0, 100), cost_fn=1.0, cost_fp=1.0, spec=0.9):
    """(threshold, objective, status) of one rule on the curve c."""
    if not c.valid:
        return math.nan, math.nan, -2.0
    P, N = float(c.P), float(c.N)
    tps, fps = c.tps.astype(np.float64), c.fps.astype(np.float64)
    if rule == "roc":
        J = np.r_[0.0, (tps / P - fps / N)[c.kept]]
        i = int(np.argmax(J))
        return (math.inf if i == 0 else float(c.thr[c.kept][i - 1])), float(J[i]), 0.0
    if rule in ("f1", "cost"):
        th = np.linspace(grid[0], grid[1], int(grid[2]))
        tp, fp = c.counts_at(th)
        if rule == "f1":
            v = (2 * tp).astype(np.float64) / (c.P + tp + fp).astype(np.float64)
            i = int(np.argmax(v))
            return (float(th[i]), float(v[i]), 0.0) if v[i] > 0.0 else (0.0, 0.0, 0.0)
        v = fp.astype(np.float64) * float(cost_fp) + (c.P - tp).astype(np.float64) * float(cost_fn)
        i = int(np.argmin(v))
        return (float(th[i]), float(v[i]), 0.0) if v[i] < math.inf else (0.0, math.inf, 0.0)
    if rule in ("pr", "f1max"):
        tp, fp, thr = tps[::-1], fps[::-1], c.thr[::-1]                     # ascending thresholds
        with np.errstate(invalid="ignore", divide="ignore"):
            p, r = tp / (tp + fp), tp / P
            f = 2 * (p * r) / (p + r)
        if rule == "f1max":
            f = np.where(tp == 0, 0.0, f)
        i = int(np.argmax(f))                                               # (the first NaN where there is one)
        return float(thr[i]), float(f[i]), (1.0 if np.isnan(f[i]) else 0.0)
    if rule == "eer":
        d = np.r_[1.0, np.abs((1.0 - tps / P) - fps / N)[c.kept]]
        i = int(np.nanargmin(d))
        return (math.inf if i == 0 else float(c.thr[c.kept][i - 1])), float(d[i]), 0.0
    if rule == "spec":
        need = math.ceil(float(spec) * N)
        ok = np.nonzero(c.N - c.fps >= need)[0]
        if ok.size == 0:
            return math.inf, 1.0, 0.0
        j = int(ok[-1])
        return float(c.thr[j]), float(c.N - c.fps[j]) / N, 0.0
    raise ValueError(rule)


def apply(threshold, objective, status, scores, labels):
    """One row of COLUMNS: the threshold scored on an evaluation set (:144-153)."""
    s, y = as_scores(scores), as_labels(labels)
    if status == -2.0 or s.size == 0:
        return np.array([math.nan] * 7 + [-2.0])
    pred = s >= threshold
    tp, fp = int((pred & y).sum()), int((pred & ~y).sum())
    P = int(y.sum())
    N = s.size - P
    tn = N - fp
    return np.array([threshold, float(tp + tn) / float(s.size), float(tp) / float(P) if P else math.nan,
                     float(tn) / float(N) if N else math.nan, float(tp), float(fp), objective, status])


def summary(c, spec=0.9, sens=0.9, max_fpr=0.1):
    """One row of SUMMARY."""
    row = np.full(8, math.nan)
    if 1 <= c.n <= MAX_N:
        row[6], row[7] = c.P, c.N
    if not c.valid:
        return row
    P, N = float(c.P), float(c.N)
    tps0, fps0 = np.r_[0, c.tps[:-1]], np.r_[0, c.fps[:-1]]
    a2 = int(((c.fps - fps0) * (c.tps + tps0)).sum())
    row[0] = float(a2) / (2.0 * P * N)
    # average_precision_score: -sum(diff(recall) * precision[:-1]) over precision_recall_curve's arrays
    precision = np.r_[(c.tps / (c.tps + c.fps))[::-1], 1.0]
    recall = np.r_[(c.tps / P)[::-1], 0.0]
    row[1] = -np.sum(np.diff(recall) * precision[:-1])
    # roc_auc_score(max_fpr=): the curve cut at max_fpr, McClish's standardisation
    fpr, tpr = np.r_[0.0, c.fps / N], np.r_[0.0, c.tps / P]
    if max_fpr == 1.0:
        row[2] = row[0]
    else:
        stop = int(np.searchsorted(fpr, max_fpr, "right"))
        y_cut = np.interp(max_fpr, fpr[stop - 1:stop + 1], tpr[stop - 1:stop + 1])
        x, y = np.r_[fpr[:stop], max_fpr], np.r_[tpr[:stop], y_cut]
        area = float(np.sum(np.diff(x) * (y[1:] + y[:-1]) / 2.0))
        lo = 0.5 * max_fpr * max_fpr
        row[2] = 0.5 * (1.0 + (area - lo) / (max_fpr - lo))
    ok = np.nonzero(c.N - c.fps >= math.ceil(float(spec) * N))[0]
    row[3] = float(c.tps[ok[-1]]) / P if ok.size else 0.0
    j = int(np.nonzero(c.tps >= math.ceil(float(sens) * P))[0][0])
    row[4] = float(c.N - c.fps[j]) / N
    row[5] = c.K
    return row


def roc_on_grid(c, G):
    """np.interp of the full curve (origin first) at linspace(0, 1, G)."""
    if not c.valid:
        return np.full(G, math.nan)
    return np.interp(np.linspace(0.0, 1.0, G), np.r_[0.0, c.fps / float(c.N)], np.r_[0.0, c.tps / float(c.P)])


def operating_points(scores, positive, rules=("roc",), select_of=None, evaluate=None, grid=(0.0, 1.0, 100), cost_fn=1.0,
                     cost_fp=1.0, spec=0.9, sens=0.9, max_fpr=0.1, roc_grid=0):
    """metrics.operating_points on the host: (points, summary) or (points, summary, grid) as numpy arrays."""
    curves = [Curve(s, l) for s, l in zip(scores, positive)]
    evaluate = list(range(len(curves))) if evaluate is None else list(evaluate)
    select_of = list(evaluate) if select_of is None else list(select_of)
    chosen = [[select(c, r, grid, cost_fn, cost_fp, spec) for r in rules] for c in curves]
    points = np.array([[apply(*chosen[ss][k], scores[es], positive[es]) for k in range(len(rules))]
                       for es, ss in zip(evaluate, select_of)]).reshape(len(evaluate), len(rules), 8)
    summ = np.array([summary(c, spec, sens, max_fpr) for c in curves])
    if roc_grid:
        return points, summ, np.array([roc_on_grid(c, roc_grid) for c in curves])
    return points, summ
