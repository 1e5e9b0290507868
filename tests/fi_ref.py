"""The row table of the regression model's evaluation pass (include/nmhip.h: nm_fi_pass, metrics.FI_ROW_COLUMNS) restated in
numpy from a pass's own exports (fi_draws, per-decoder row deviations of draw 0, mu, logvar, the target), operation by
operation in fp32.

    fi_pred  the mean of the S predictions p_s by the running fold: s = 0: mean = p_0, M2 = 0; s >= 1: d = p_s - mean,
             mean += d * (1 / (s + 1)), M2 += d * (p_s - mean), with 1 / (s + 1) rounded to fp32 first
    fi_sd    sqrt(M2 * (1 / (S - 1))); S = 1: 0
    fi_min / fi_max over the draws
    err      fi_pred - target; no target: 0 and status carries 2
    dev      (((d_0 + d_1) + ...) + d_{M-1}) / M
    kl       tests/endtoend_ref.py's (the same formula and summation order): its fp64 value and bound
    status   1 if a prediction, a deviation, mu or logvar of the row is not finite; + 2 without a target

Every column but kl holds no transcendental (sqrt is correctly rounded): an fp32 evaluation in this order gives these
bytes, whoever computes it.

Bound of the fold against the fp64 mean and standard deviation of the same S fp32 numbers (check_fold), from the
definition alone, u = 2^-24, A = max_s |p_s|:
    mean   step s forms d (one rounding, |d| <= 2 A), d * r_s (r_s itself rounded: two roundings) and the sum (one rounding
           of a value <= A (1 + 2u)): at most 4 roundings of quantities <= 2 A, i.e. 8 u A per step; an error already in the
           mean is carried with the factor (1 - r_s) <= 1, so the steps add: |mean - mean64| <= 8 u A S.  (A few ulp of the
           mean times S, as long as the predictions do not cancel; stated against A because they may.)
    sd     M2 takes per step three more roundings of products <= (2 A)^2 and inherits the mean's error times |d| <= 2 A:
           |M2 - M2_64| <= S (3 u (2 A)^2 + 2 * 2 A * 8 u A S) <= 44 u A^2 S^2; the division and the square root add two
           roundings of sd itself, and sqrt turns an absolute error e of the variance into at most sqrt(e):
           |sd - sd64| <= sqrt(44 u A^2 S^2 / (S - 1)) + 2 u sd64
"""
import numpy as np

from tests import endtoend_ref as E

COLUMNS = ("fi_pred", "fi_sd", "fi_min", "fi_max", "err", "dev", "kl", "status")
EXACT = ("fi_pred", "fi_sd", "fi_min", "fi_max", "err", "dev", "status")
f32 = np.float32
U24 = 2.0 ** -24


def head(resid, w1, b1, w2, b2, w3, b3):
    """The regressor (cVAE.py:2249-2253) on the concatenated residuals [N, sum D]: Linear(sum D, 128) - ReLU -
    Linear(128, 64) - ReLU - Linear(64, 1), fp32 -> [N] float32."""
    r = np.asarray(resid, f32)
    h1 = np.maximum((r @ np.asarray(w1, f32).T + np.asarray(b1, f32)).astype(f32), f32(0.0))
    h2 = np.maximum((h1 @ np.asarray(w2, f32).T + np.asarray(b2, f32)).astype(f32), f32(0.0))
    return (h2 @ np.asarray(w3, f32).T + np.asarray(b3, f32)).astype(f32).reshape(-1)


def fold(draws):
    """draws [N, S] fp32 -> (mean, M2, min, max), each [N] fp32, by the running fold in draw order."""
    p = np.asarray(draws, f32)
    mean, m2 = p[:, 0].copy(), np.zeros(p.shape[0], f32)
    lo, hi = p[:, 0].copy(), p[:, 0].copy()
    for s in range(1, p.shape[1]):
        rs = f32(1.0) / f32(s + 1)
        d = (p[:, s] - mean).astype(f32)
        mean = (mean + (d * rs).astype(f32)).astype(f32)
        m2 = (m2 + (d * (p[:, s] - mean).astype(f32)).astype(f32)).astype(f32)
        lo, hi = np.fmin(lo, p[:, s]), np.fmax(hi, p[:, s])
    return mean, m2, lo, hi


def row_table(draws, rowdev, mu, lv, target):
    """draws [N, S]; rowdev: M arrays [N] (draw 0); mu, lv [N, Z]; target [N] or None; all taken as fp32.
    -> dict of [N] float32 arrays under COLUMNS (kl: endtoend_ref's fp32 restatement)."""
    with np.errstate(all="ignore"):
        p = np.asarray(draws, f32)
        N, S = p.shape
        mean, m2, lo, hi = fold(p)
        sd = np.sqrt((m2 * (f32(1.0) / f32(S - 1))).astype(f32)).astype(f32) if S > 1 else np.zeros(N, f32)
        err = (mean - np.asarray(target, f32)).astype(f32) if target is not None else np.zeros(N, f32)
        dev = [np.asarray(d, f32) for d in rowdev]
        dsum = dev[0].copy()
        for d in dev[1:]:
            dsum = (dsum + d).astype(f32)
        dsum = (dsum / f32(len(dev))).astype(f32)
        # endtoend_ref.row_table wants logits and two banks: a dummy of both, its kl column alone is read
        kl = E.row_table(np.zeros((N, 2), f32), [dev[0], dev[0]], mu, lv)["kl"]
        bad = ~(np.isfinite(p).all(axis=1) & np.isfinite(np.asarray(mu, f32)).all(axis=1) & np.isfinite(np.asarray(lv, f32)).all(axis=1))
        for d in dev:
            bad |= ~np.isfinite(d)
        status = bad.astype(f32) + f32(0.0 if target is not None else 2.0)
        return {"fi_pred": mean, "fi_sd": sd, "fi_min": lo, "fi_max": hi, "err": err, "dev": dsum, "kl": kl, "status": status}


def kl_reference64(mu, lv):
    """(value, bound) of the kl column in fp64: endtoend_ref's."""
    val, bnd = E.reference64(np.zeros((np.asarray(mu).shape[0], 2), f32), mu, lv)
    return val["kl"], bnd["kl"]


def fold_bounds(draws):
    """(mean64, bound of the mean, sd64, bound of the sd) of the S fp32 predictions of every row, [N] float64 each."""
    p = np.asarray(draws, f32).astype(np.float64)
    S = p.shape[1]
    A = np.abs(p).max(axis=1)
    mean64 = p.mean(axis=1)
    sd64 = p.std(axis=1, ddof=1) if S > 1 else np.zeros(p.shape[0])
    bm = 8.0 * U24 * A * S + 1e-300
    bs = (np.sqrt(44.0 * U24 * A * A * S * S / (S - 1)) + 2.0 * U24 * sd64 if S > 1 else np.zeros(p.shape[0])) + 1e-300
    return mean64, bm, sd64, bs


def check_table(row, draws, rowdev, mu, lv, target):
    """Names of the columns of `row` [N, 8] that disagree with the restatement: the EXACT columns bit for bit (NaN equal to
    NaN), kl within its bound; and the worst share of the kl bound."""
    t = row_table(draws, rowdev, mu, lv, target)
    row = np.asarray(row, f32)
    wrong = [n for n in EXACT if not np.array_equal(row[:, COLUMNS.index(n)], t[n], equal_nan=True)]
    val, bnd = kl_reference64(mu, lv)
    share = E.worst_ratio(row[:, COLUMNS.index("kl")], val, bnd) if row.shape[0] else 0.0
    if not share <= 1.0:
        wrong.append("kl")
    return wrong, share
