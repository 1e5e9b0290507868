"""Yardsticks, CPU twins, case lists and bounds for the stand-alone fusion launches (csrc/nm_fusion.hip:
nm_combine_latent, nm_total_correlation) and the latent statistics (csrc/nm_metrics.hip: nm_latent_stats, nm_latent_score).

  fuse_ref / tc_ref       the operation as the header documents it, in float64 on the fp32 inputs, with the scale each
                          error bound is stated against
  fuse_twin / tc_twin     the kernels' own order of operations in float32 (numpy, vectorised over elements / columns)
  stats_twin              nm_latent_stats' chunked two-pass sums and Chan merge in float64
  FUSE_CASES / TC_CASES / LATENT_CASES / SCORE_CASES     shared by the CPU and the GPU tests

Bounds (derived first, then the working constant measured ON THE TWIN, never on the kernel):

  nm_combine_latent   |mu - ref| <= k eps32 scale_mu,  |var - ref| <= k eps32 |ref|  (out_log: k eps32 (|ref| + 1)); no absolute
      term.  scale_mu is the condition scale of the mean: sum |mu_m| w_m / sum w_m for PoE / gPoE, mean |mu_m| for MoE, the
      (M + 1)-average of both for MoPoE.  A-priori ceiling k = 40 at M = 8 gPoE: expf 1 ulp, the division that forms the
      weight, the softmax of 8 (expf, 8-term sum, division), two 8-term serial sums, the quotient.  Working k per (combine,
      in_log, out_log): 4 x the twin's worst ratio over FUSE_CASES, floored at 8, capped at 40 -- the 4 is for the device's
      expf / logf being 1 ulp where numpy's are about half, and for FMA contraction of `Smu += mu * w`.
  nm_total_correlation   |tc - ref| <= k eps32 A,  A = sum_z mean_m |lse_mz| + Z;  k = 4 x the twin's worst ratio over TC_CASES,
      floored at 8.
  nm_latent_stats   fp64 throughout, rounded once: 1 ulp (fp32) of np.mean / np.var of the widened input.
  nm_latent_score   zsep 4 eps32 |ref| (one rounded subtraction, expf, add, sqrt, division); score (Z + 4) eps32 ref (a serial
      sum of Z non-negative terms).
"""
import itertools

import numpy as np
import torch

EPS32 = float(np.finfo(np.float32).eps)
COMBINERS = ("poe", "gpoe", "moe", "mopoe")
FUSE_MAX = 8
K_CEILING = 40.0
K_FLOOR = 8.0

# The twins' worst ratios (error / (eps32 x scale)) over the case lists below, as tests/test_fusion_ref_cpu.py re-measures
# them (a value far from these means the twin is wrong), rounded up to 0.1.  Keyed (combine, in_log, out_log) -> (ratio of
# the mean, ratio of the variance).  The working k follows from them: min(40, max(8, 4 x the larger)).
TWIN_FUSE = {
    ("poe", 0, 0): (2.9, 2.0), ("poe", 0, 1): (2.7, 1.3), ("poe", 1, 0): (2.8, 2.5), ("poe", 1, 1): (2.9, 1.6),
    ("gpoe", 0, 0): (5.4, 4.9), ("gpoe", 0, 1): (4.3, 3.5), ("gpoe", 1, 0): (4.9, 4.1), ("gpoe", 1, 1): (5.9, 4.1),
    ("moe", 0, 0): (2.1, 1.9), ("moe", 0, 1): (1.9, 1.4), ("moe", 1, 0): (2.1, 2.3), ("moe", 1, 1): (2.4, 1.5),
    ("mopoe", 0, 0): (2.2, 2.2), ("mopoe", 0, 1): (2.4, 1.7), ("mopoe", 1, 0): (2.2, 2.3), ("mopoe", 1, 1): (2.3, 1.8),
}
TWIN_TC_RATIO = 3.3
K_TC = max(K_FLOOR, 4.0 * TWIN_TC_RATIO)                                   # 13.2


def k_fuse(combine, in_log, out_log):
    return min(K_CEILING, max(K_FLOOR, 4.0 * max(TWIN_FUSE[(combine, int(bool(in_log)), int(bool(out_log)))])))


# ---- nm_combine_latent: float64 yardstick --------------------------------------------------------------------------------
def _softmax64(alpha_raw):
    a = torch.as_tensor(np.asarray(alpha_raw, np.float32)).double()
    return torch.softmax(a, 0)


def fuse_expr(mus, vin, combine, al=None, single_bypass=False, in_log=False, out_log=False, var_floor=0.0):
    """The documented operation as a torch expression in the dtype of its inputs (differentiable): mus / vin [M, ...], al the
    NORMALISED gPoE weights [M].  Returns (mu, var, scale_mu)."""
    M = int(mus.shape[0])
    var = torch.exp(vin) if in_log else vin
    if M == 1 and single_bypass:
        omu, ovar, scale = mus[0], var[0], mus[0].abs()
    elif combine == "moe":
        omu, ovar, scale = mus.sum(0) / M, var.sum(0) / M, mus.abs().sum(0) / M
    else:
        w = 1.0 / var
        if combine == "gpoe":
            w = al.reshape((M,) + (1,) * (mus.dim() - 1)) / var
        S = w.sum(0)
        omu, ovar, scale = (mus * w).sum(0) / S, 1.0 / S, (mus.abs() * w).sum(0) / S
        if combine == "mopoe":
            omu, ovar = (mus.sum(0) + omu) / (M + 1), (var.sum(0) + ovar) / (M + 1)
            scale = (mus.abs().sum(0) + scale) / (M + 1)
        elif combine not in ("poe", "gpoe"):
            raise ValueError(combine)
    if out_log:
        ovar = torch.log(ovar)
    if var_floor > 0:
        ovar = torch.clamp(ovar, min=float(np.float32(var_floor)))         # (NaN stays NaN, as torch.clamp in the reference)
    return omu, ovar, scale


def fuse_ref(mus, vin, combine, alpha_raw=None, single_bypass=False, in_log=False, out_log=False, var_floor=0.0):
    """nm_combine_latent as include/nmhip.h documents it, float64 on the fp32 inputs.  Returns numpy (mu, var, scale_mu)."""
    mu = torch.as_tensor(np.asarray(mus, np.float32)).double()
    v = torch.as_tensor(np.asarray(vin, np.float32)).double()
    al = _softmax64(alpha_raw)[:mu.shape[0]] if combine == "gpoe" else None
    with torch.no_grad():
        out = fuse_expr(mu, v, combine, al, single_bypass, in_log, out_log, var_floor)
    return tuple(o.numpy() for o in out)


# ---- nm_combine_latent: float32 twin of combine_latent_kernel ------------------------------------------------------------
def fuse_twin(mus, vin, combine, alpha_raw=None, single_bypass=False, in_log=False, out_log=False, var_floor=0.0, fault=None):
    """combine_latent_kernel's order of operations in float32: the softmax over all FUSE_MAX slots (max, expf, serial sum,
    division), then per element the serial accumulation over m of S, Smu, sm, sv.  `fault` plants one mistake: loop_bound, alpha_swap,
    mopoe_div or floor_before_log."""
    f32 = np.float32
    mus, vin = np.asarray(mus, f32), np.asarray(vin, f32)
    M = mus.shape[0]
    al = np.zeros(FUSE_MAX, f32)
    if alpha_raw is not None:
        a = np.asarray(alpha_raw, f32)[:M]
        e = np.zeros(FUSE_MAX, f32)
        e[:M] = np.exp(a - a.max())
        s = f32(0)
        for m in range(FUSE_MAX):
            s = f32(s + e[m])
        al = (e / s).astype(f32) if s > 0 else al
    with np.errstate(all="ignore"):
        if M == 1 and single_bypass:
            omu, ovar = mus[0].copy(), (np.exp(vin[0]) if in_log else vin[0].copy())
        else:
            S = np.zeros(mus.shape[1:], f32); Smu = S.copy(); sm = S.copy(); sv = S.copy()
            for m in range(M - 1 if (fault == "loop_bound" and M == FUSE_MAX) else M):
                var = np.exp(vin[m]) if in_log else vin[m]
                if combine == "gpoe":
                    w = al[m ^ 1 if fault == "alpha_swap" else m] / var
                else:
                    w = f32(1) / var
                S = S + w; Smu = Smu + mus[m] * w
                sm = sm + mus[m]; sv = sv + var
            if combine == "moe":
                omu, ovar = sm / f32(M), sv / f32(M)
            else:
                omu, ovar = Smu / S, f32(1) / S
                if combine == "mopoe":
                    d = f32(M if fault == "mopoe_div" else M + 1)
                    omu, ovar = (sm + omu) / d, (sv + ovar) / d
        fl = f32(var_floor)
        if fault == "floor_before_log" and var_floor > 0:
            ovar = np.where(ovar < fl, fl, ovar)
        if out_log:
            ovar = np.log(ovar)
        if var_floor > 0 and fault != "floor_before_log":
            ovar = np.where(ovar < fl, fl, ovar)
    return omu.astype(f32), ovar.astype(f32)



# ---- nm_total_correlation --------------------------------------------------------------------------------------------------
def tc_ref(q):
    """-sum_z mean_m logsumexp_rows(q[m, :, z]) in float64 and the scale A = sum_z mean_m |lse_mz| + Z."""
    q = np.asarray(q, np.float32).astype(np.float64)
    mx = q.max(axis=1)
    lse = mx + np.log(np.exp(q - mx[:, None, :]).sum(axis=1))              # [M, Z]
    return float(-lse.mean(axis=0).sum()), float(np.abs(lse).mean(axis=0).sum() + q.shape[2])


def tc_twin(q, fault=None):
    """total_correlation_kernel in float32: per (expert, column) 64 lane partials over the rows lane, lane + 64, ..., the
    xor-butterfly, lse = mx + logf(sx); then the serial sum over m, divided by M, subtracted serially over z."""
    f32 = np.float32
    q = np.asarray(q, f32)
    M, B, Z = q.shape
    Bk = B & ~63 if fault == "row_loop_trunc" else B
    K = (B + 63) // 64
    pad = np.full((M, K * 64, Z), -np.inf, f32)
    pad[:, :Bk] = q[:, :Bk]
    pad = pad.reshape(M, K, 64, Z)                                          # row k * 64 + lane
    lanes = np.arange(64)
    with np.errstate(all="ignore"):
        mx = np.full((M, 64, Z), 0.0 if fault == "max_init_zero" else -3.0e38, f32)
        for k in range(K):
            mx = np.maximum(mx, pad[:, k])
        mx = mx.max(axis=1, keepdims=True)                                  # (a max is the same in any order)
        sx = np.zeros((M, 64, Z), f32)
        for k in range(K):
            sx = sx + np.exp(pad[:, k] - mx)
        o = 32
        while o:
            sx = sx + sx[:, lanes ^ o]
            o >>= 1
        lse = (mx[:, 0] + np.log(sx[:, 0])).astype(f32)                     # [M, Z]
        s = np.zeros(Z, f32)
        for m in range(M):
            s = s + lse[m]
        term = s / f32(M)
        tc = f32(0)
        for z in range(Z):
            tc = f32(tc - term[z])
    return float(tc)


TC_FAULTS = ("row_loop_trunc", "max_init_zero")


# ---- nm_latent_stats: the chunked merge in float64 ---------------------------------------------------------------------------
LAT_CHUNK, LAT_THREADS = 128, 256


def stats_twin(x, fault=None):
    """latent_stats_kernel for one cohort x [n, Z]: per 128-row chunk the serial sum, its mean and the serial sum of squared
    deviations (float64), merged in row order by Chan's formula in rounds of 256 // Z chunks; rounded once to float32.
    `fault`: cnt_not_carried or merge_per_index."""
    x = np.asarray(x, np.float32).astype(np.float64)
    n, Z = x.shape
    if n == 0:
        return np.full(Z, np.nan, np.float32), np.full(Z, np.nan, np.float32)
    per = LAT_THREADS // Z
    nch = (n + LAT_CHUNK - 1) // LAT_CHUNK
    cm, q, nb = np.zeros((nch, Z)), np.zeros((nch, Z)), np.zeros(nch)
    for c in range(nch):
        blk = x[c * LAT_CHUNK:(c + 1) * LAT_CHUNK]
        s = np.zeros(Z)
        for r in range(blk.shape[0]):
            s = s + blk[r]
        cm[c] = s / blk.shape[0]
        for r in range(blk.shape[0]):
            q[c] = q[c] + (blk[r] - cm[c]) ** 2
        nb[c] = blk.shape[0]
    cnt, mean, m2 = 0.0, np.zeros(Z), np.zeros(Z)
    for c0 in range(0, nch, per):
        if fault == "cnt_not_carried":
            cnt = 0.0
        # the partials of a round as the threads leave them in LDS: slot cl * Z + z
        lds_m, lds_q = np.zeros(LAT_THREADS), np.zeros(LAT_THREADS)
        k_hi = min(per, nch - c0)
        lds_m[:k_hi * Z], lds_q[:k_hi * Z] = cm[c0:c0 + k_hi].ravel(), q[c0:c0 + k_hi].ravel()
        stride = per if fault == "merge_per_index" else Z
        for k in range(k_hi):
            idx = np.minimum(k * stride + np.arange(Z), LAT_THREADS - 1)
            delta, tot = lds_m[idx] - mean, cnt + nb[c0 + k]
            mean = mean + delta * (nb[c0 + k] / tot)
            m2 = m2 + lds_q[idx] + delta * delta * (cnt * nb[c0 + k] / tot)
            cnt = tot
    return mean.astype(np.float32), (m2 / cnt).astype(np.float32)


# ---- the cases -------------------------------------------------------------------------------------------------------------
FUSE_MS = (1, 2, 3, 8)
FUSE_NS = (1, 255, 256, 257, 4099)          # one thread; the block edge from both sides; several blocks, n % 4 != 0
FUSE_FLAGS = tuple(itertools.product((0, 1), (0, 1), (0, 1), (0.0, 1e-6)))          # (in_log, out_log, single_bypass, var_floor)
MU_SCALES = (1e-3, 1.0, 1e3)
LV_SPREADS = (0.7, 8.0)
LV_CLIP = 69.0                              # variances within [1e-30, 1e30]: every reciprocal and sum a normal fp32 number


def fuse_cases(combine):
    """Every M x n x flag combination of one combiner: (M, n, in_log, out_log, single_bypass, var_floor, seed, spread,
    extreme).  The log-variance spread follows the parity of (shape index + number of set flags), so every flag combination
    meets both spreads at every M and each (M, n) meets both under either value of every flag; a third of the gPoE cases carry the extreme weight vector (+40, -40, 0, ...)
    at the narrow spread, so that alpha_m / var stays a normal number."""
    out = []
    for i, (M, n, fl) in enumerate(itertools.product(FUSE_MS, FUSE_NS, FUSE_FLAGS)):
        extreme = combine == "gpoe" and i % 3 == 0
        spread = LV_SPREADS[0] if extreme else LV_SPREADS[(i // len(FUSE_FLAGS) + sum(bool(x) for x in fl)) % 2]
        out.append((M, n, fl[0], fl[1], fl[2], fl[3], 1000 * COMBINERS.index(combine) + i, spread, extreme))
    return out


FUSE_CASES = {c: fuse_cases(c) for c in COMBINERS}


def fuse_inputs(case):
    """(mus, vin, alpha_raw) float32 for one case: means at a scale per expert from MU_SCALES with mixed signs, log-variances
    N(0, spread), alpha_raw N(0, 3) or the extreme vector.  vin is the variance, or its logarithm with in_log."""
    M, n, in_log, _, _, _, seed, spread, extreme = case
    rng = np.random.default_rng(seed)
    scale = np.asarray(MU_SCALES)[rng.integers(0, 3, M)]
    mus = (rng.standard_normal((M, n)) * scale[:, None]).astype(np.float32)
    lv = np.clip(spread * rng.standard_normal((M, n)), -LV_CLIP, LV_CLIP).astype(np.float32)
    vin = lv if in_log else np.exp(lv.astype(np.float64)).astype(np.float32)
    alpha = (3.0 * rng.standard_normal(FUSE_MAX)).astype(np.float32)
    if extreme:
        alpha = np.array([40.0, -40.0, 0, 0, 0, 0, 0, 0], np.float32)
    return mus, vin, alpha[:M].copy()


def nonfinite_inputs(in_log):
    """M = 2, one small tensor: a zero variance beside a non-zero mean, two zero variances with opposite means, a +inf variance,
    a +inf mean, a NaN variance, and ordinary elements between them."""
    mus = np.array([[1.5, 2.0, 0.5, 0.25, -1.0, np.inf, 3.0, 0.75],
                    [-0.5, -2.0, 1.0, -4.0, 2.0, 1.0, 1.0, -0.125]], np.float32)
    var = np.array([[0.0, 0.0, 2.0, np.inf, 0.5, 1.0, np.nan, 4.0],
                    [1.0, 0.0, 0.5, 1.0, 0.25, 2.0, 1.0, 0.0625]], np.float32)
    with np.errstate(all="ignore"):
        return mus, (np.log(var) if in_log else var), np.array([0.3, -1.1], np.float32)


def fuse_errors(got_mu, got_var, ref, out_log):
    """The two error ratios (in units of eps32 x scale) over the elements where the yardstick is finite; the elements where
    it is not must carry the same kind of non-finite value.  A ratio that cannot be formed -- a NaN or an infinity where the
    yardstick is finite -- is inf, never NaN, so that no comparison or max() can lose it."""
    mu, var, scale = ref
    out = []
    with np.errstate(all="ignore"):
        for got, want, sc in ((got_mu, mu, scale), (got_var, var, np.abs(var) + (1.0 if out_log else 0.0))):
            got = np.asarray(got, np.float64)
            fin = np.isfinite(want)
            same = np.where(np.isnan(want), np.isnan(got), got == want)
            if not np.all(same[~fin]) or not np.all(np.isfinite(got[fin])):
                out.append(np.inf)
                continue
            err = np.abs(got[fin] - want[fin])
            ratio = np.where(err == 0, 0.0, err / (EPS32 * sc[fin]))
            worst = float(np.max(ratio)) if ratio.size else 0.0
            out.append(worst if np.isfinite(worst) else np.inf)
    return out[0], out[1]


def within(r, k):
    """Both ratios of fuse_errors inside k, each compared on its own (a max() over the pair could drop a NaN)."""
    return bool(r[0] <= k) and bool(r[1] <= k)


TC_MS, TC_BS, TC_ZS = (1, 3, 8), (1, 63, 64, 65, 200, 1000), (1, 6, 127, 128)
TC_KINDS = ("normal", "plus90", "minus90", "spread30")
TC_CASES = [(M, B, Z, kind, i) for i, (M, B, Z, kind) in enumerate(itertools.product(TC_MS, TC_BS, TC_ZS, TC_KINDS))]


def tc_inputs(case):
    M, B, Z, kind, seed = case
    g = np.random.default_rng(7000 + seed).standard_normal((M, B, Z))
    q = {"normal": g, "plus90": 90.0 + g, "minus90": -90.0 + 5.0 * g, "spread30": 30.0 * g}[kind]
    return q.astype(np.float32)


LATENT_CASES = [(1, 1), (127, 64), (128, 64), (129, 64), (512, 64), (513, 64), (1000, 64), (2000, 1), (700, 48), (8192, 33),
                (5376, 6), (5377, 6)]
LATENT_KINDS = ("normal", "offset1e4", "minus300")
SCORE_CASES = [(300, 6), (257, 64), (1, 64), (1000, 33)]


def latent_inputs(n, Z, kind, seed=0):
    g = np.random.default_rng(9000 + 131 * n + 7 * Z + seed).standard_normal((n, Z))
    return {"normal": g, "offset1e4": 1e4 + g, "minus300": -300.0 + 0.01 * g}[kind].astype(np.float32)


def ulps32(got, want64):
    """|got - want| in units of the fp32 spacing at want."""
    want64 = np.asarray(want64, np.float64)
    sp = np.spacing(np.abs(want64).astype(np.float32)).astype(np.float64)
    return np.abs(np.asarray(got, np.float64) - want64) / sp
