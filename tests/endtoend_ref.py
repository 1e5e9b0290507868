"""The row table of the end-to-end model's evaluation pass (include/nmhip.h: nm_e2e_pass, metrics.ENDTOEND_ROW_COLUMNS)
restated in numpy from (logits, per-decoder row deviations, mu, logvar), operation by operation in fp32, with the fp64
value and the error bound of the two columns that go through exp.

    p_disease   = (sum_{k>=1} e_k) / (sum_k e_k), e_k = exp(l_k - max_k l_k), sums in index order
    pred        = first index of the maximum logit
    margin      = max_{k>=1} l_k - l_0
    dev_health  = (((d_0 + d_1) + ...) + d_{Me-1}) / Me          dev_disease: the same over decoders Me + m
    contrast    = dev_health - dev_disease
    kl          = -0.5 sum_z (((1 + lv) - mu^2) - exp(lv)): four interleaved partial sums p_i over the columns i, i + 4, ...
                  (Z a multiple of 4: over the quads 4 i .., 4 (i + 4) ..), then (p_0 + p_1) + (p_2 + p_3)
    status      = 1 if a logit, a deviation, mu or logvar of the row is not finite

pred, margin, dev_health, dev_disease, contrast and status hold no transcendental: an fp32 evaluation in this order gives
these bytes, whoever computes it.  p_disease and kl depend on the exp in use (the device's expf, torch.exp, numpy's), so
they are held to fp64 within bounds taken from the definition alone:

    exp          EXP_REL = 4 * 2^-23: the libraries' fp32 exp is good to a few ulp (tests/loglik_ref.py allows the same)
    p_disease    the final division is one fp32 rounding of a value in [0, 1]: 2^-24.  Ahead of it, a relative perturbation
                 rho_k of every e_k moves p by at most p (1 - p) max_ij |rho_i - rho_j| <= 1/4 * 2 max |rho|, and rho_k is
                 the exp's own error plus the C - 1 additions of the two sums (2^-24 each).  The rounding of the argument
                 l_k - max, relative 2^-24, changes e_k by e_k |x_k| 2^-24 <= 2^-24 / e in absolute terms against a
                 denominator >= 1: C / e * 2^-24 for all of them.
                 bound = 2^-24 + 1/2 (EXP_REL + (C - 1) 2^-24) + C / e * 2^-24                (about 4e-7 at C = 4)
    kl           a recursive fp32 sum of 4 Z addends (1, lv, mu^2, exp(lv) per column), as tests/loglik_ref.py bounds its
                 sums: (n + 8) 2^-23 sum |addends| with n = 4 Z, times the 1/2 in front.  The definition subtracts exp(lv)
                 from 1 + lv - mu^2, so near lv = 0 the bound is relative to the addends, not to the (small) result.
"""
import numpy as np

COLUMNS = ("p_disease", "pred", "margin", "dev_health", "dev_disease", "contrast", "kl", "status")
U = 2.0 ** -23
EXP_REL = 4.0 * U
f32 = np.float32


def kl_columns(Z):
    """The latent columns of the four partial sums, each in the order they are added."""
    if Z % 4 == 0:
        return [[z for q in range(i, Z // 4, 4) for z in range(4 * q, 4 * q + 4)] for i in range(4)]
    return [list(range(i, Z, 4)) for i in range(4)]


def row_table(logits, rowdev, mu, lv):
    """logits [N, C] (C = 2..4), rowdev: 2 Me arrays [N] (health bank first), mu, lv [N, Z]; all taken as fp32.
    -> dict of [N] float32 arrays under COLUMNS."""
    with np.errstate(all="ignore"):
        l = np.asarray(logits, f32)
        N, C = l.shape
        dev = [np.asarray(d, f32) for d in rowdev]
        Me = len(dev) // 2
        mu, lv = np.asarray(mu, f32), np.asarray(lv, f32)
        mx = l[:, 0].copy()
        for k in range(1, C):
            mx = np.maximum(mx, l[:, k])
        e = np.exp((l - mx[:, None]).astype(f32)).astype(f32)
        sd, sa = e[:, 1].copy(), (e[:, 0] + e[:, 1]).astype(f32)
        for k in range(2, C):
            sd, sa = (sd + e[:, k]).astype(f32), (sa + e[:, k]).astype(f32)
        pred = np.zeros(N, np.int64)
        top = l[:, 0].copy()
        mxd = l[:, 1].copy()
        for k in range(1, C):
            up = l[:, k] > top
            pred[up], top[up] = k, l[up, k]
            if k > 1:
                mxd = np.maximum(mxd, l[:, k])
        dh, dd = dev[0].copy(), dev[Me].copy()
        for m in range(1, Me):
            dh, dd = (dh + dev[m]).astype(f32), (dd + dev[Me + m]).astype(f32)
        dh, dd = (dh / f32(Me)).astype(f32), (dd / f32(Me)).astype(f32)
        t = ((((f32(1.0) + lv).astype(f32) - (mu * mu).astype(f32)).astype(f32)) - np.exp(lv).astype(f32)).astype(f32)
        parts = []
        for cols in kl_columns(mu.shape[1]):
            p = np.zeros(N, f32)
            for z in cols:
                p = (p + t[:, z]).astype(f32)
            parts.append(p)
        kl = (f32(-0.5) * ((parts[0] + parts[1]).astype(f32) + (parts[2] + parts[3]).astype(f32)).astype(f32)).astype(f32)
        bad = ~(np.isfinite(l).all(axis=1) & np.isfinite(mu).all(axis=1) & np.isfinite(lv).all(axis=1))
        for d in dev:
            bad |= ~np.isfinite(d)
        return {"p_disease": (sd / sa).astype(f32), "pred": pred.astype(f32), "margin": (mxd - l[:, 0]).astype(f32),
                "dev_health": dh, "dev_disease": dd, "contrast": (dh - dd).astype(f32), "kl": kl, "status": bad.astype(f32)}


def reference64(logits, mu, lv):
    """(values, bounds) of p_disease and kl in fp64 from the fp32 inputs: dicts of [N] float64 arrays."""
    l = np.asarray(logits, f32).astype(np.float64)
    C = l.shape[1]
    mu, lv = np.asarray(mu, f32).astype(np.float64), np.asarray(lv, f32).astype(np.float64)
    e = np.exp(l - l.max(axis=1, keepdims=True))
    p = e[:, 1:].sum(axis=1) / e.sum(axis=1)
    kl = -0.5 * (1.0 + lv - mu * mu - np.exp(lv)).sum(axis=1)
    Z = mu.shape[1]
    absum = (1.0 + np.abs(lv) + mu * mu + np.exp(lv)).sum(axis=1)
    val = {"p_disease": p, "kl": kl}
    bnd = {"p_disease": np.full(p.shape, 2.0 ** -24 + 0.5 * (EXP_REL + (C - 1) * 2.0 ** -24) + C / np.e * 2.0 ** -24),
           "kl": 0.5 * (4 * Z + 8) * U * absum}
    return val, bnd


def worst_ratio(got, val, bnd):
    """max over rows of |got - value| / bound."""
    return float((np.abs(np.asarray(got, np.float64) - val) / bnd).max())
