"""The yardstick of nm_auc_bootstrap (own code: uint64 hashing, searchsorted, Python integers to the end), by the definitions
of include/nmhip.h.

A set is (scores fp32, labels != 0 = positive); positives in row order are p[0..n_pos), negatives q[0..n_neg).  It is valid
if n >= 1 (and n <= max_set where one is given), n_pos >= 1, n_neg >= 1, no score is NaN and 0 <= stream id < 2^24.

    A2(P, Q)   sum over (i in P, j in Q) of 2 [s_i > s_j] + [s_i == s_j] = sum over i of #{q < s_i} + #{q <= s_i}:
               np.searchsorted left + right on the sorted negatives (float comparisons: -0 == +0, inf == inf)
    roc_auc    A2 / (2 n_pos n_neg)
    resample b = 1..n_boot, stream id sigma, draw u = 0..n-1: h = splitmix64(seed ^ 0xB0075712A9 ^ (sigma << 40) ^ (b << 16) ^ u),
               hi = h >> 32; u < n_pos draws the positive p[(hi n_pos) >> 32], u >= n_pos the negative q[(hi n_neg) >> 32]
    ci_lo/hi   sorted(A2*)[lo] / den, [hi];  boot_mean = sum A2* / (n_boot den);
    boot_se    sqrt(T / (n_boot (n_boot - 1))) / den, T = n_boot sum A2*^2 - (sum A2*)^2 as a Python integer (NaN for n_boot = 1)
    pairs      d_b = A2*_a,b - A2*_c,b; the same statistics of d; n_le0, n_ge0; p_boot = min(1, 2 (1 + min) / (1 + n_boot))

The keyword `fault` plants one named defect (the CPU tests show that each one changes the output, so the comparison with the
device can catch it): 'wrong_stratum' (draw u = 0 of every resample takes a negative in a positive's place), 'ties_as_wins'
(an equal pair counts 2), 'b_from_0' (resamples numbered from 0), 'stream_ignored' (every set hashes as stream 0)."""
import math

import numpy as np

SET_COLUMNS = ("roc_auc", "ci_lo", "ci_hi", "boot_mean", "boot_se", "n_boot", "n_pos", "n_neg")
PAIR_COLUMNS = ("delta_auc", "ci_lo", "ci_hi", "boot_mean", "boot_se", "p_boot", "n_le0", "n_ge0")
FAULTS = ("wrong_stratum", "ties_as_wins", "b_from_0", "stream_ignored")
SALT = 0xB0075712A9
M64 = (1 << 64) - 1
MAX_STREAM = (1 << 24) - 1


def splitmix64(x):
    """splitmix64 on a uint64 array (wrapping arithmetic)."""
    x = np.asarray(x, dtype=np.uint64)
    with np.errstate(over="ignore"):
        x = x + np.uint64(0x9E3779B97F4A7C15)
        x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return x ^ (x >> np.uint64(31))


def indices(hi, m):
    """The multiply-shift draw (hi * m) >> 32 of 32-bit words hi over a group of m members (uint64 arithmetic: hi m < 2^45)."""
    return ((np.asarray(hi, dtype=np.uint64) * np.uint64(m)) >> np.uint64(32)).astype(np.int64)


def draws(n_pos, n_neg, b, seed=0, sigma=0, fault=None):
    """(ip [len(b), n_pos], iq [len(b), n_neg]): the ordinals drawn by the resamples numbered b (1-based) of stream sigma."""
    b = np.asarray(b, dtype=np.uint64).reshape(-1, 1)
    if fault == "b_from_0":
        b = b - np.uint64(1)
    if fault == "stream_ignored":
        sigma = 0
    fixed = np.uint64((int(seed) ^ SALT ^ (int(sigma) << 40)) & M64)
    u = np.arange(n_pos + n_neg, dtype=np.uint64)[None, :]
    hi = splitmix64(fixed ^ (b << np.uint64(16)) ^ u) >> np.uint64(32)
    return indices(hi[:, :n_pos], n_pos), indices(hi[:, n_pos:], n_neg)


def a2(pv, qv, fault=None):
    """A2 of positives' values pv against negatives' values qv (float64 arrays without NaN), a Python integer."""
    qs = np.sort(qv)
    left, right = np.searchsorted(qs, pv, side="left"), np.searchsorted(qs, pv, side="right")
    if fault == "ties_as_wins":
        left = right
    return int(left.sum()) + int(right.sum())


def split(scores, labels, stream=0, max_set=None):
    """(p values, q values) as float64 in row order, or None where the set is not valid."""
    s = np.asarray(scores, dtype=np.float32).astype(np.float64).reshape(-1)
    pos = np.asarray(labels).reshape(-1) != 0
    if s.size != pos.size:
        raise ValueError("one label per score")
    n, n_pos = s.size, int(pos.sum())
    if n < 1 or (max_set is not None and n > max_set) or n_pos < 1 or n - n_pos < 1 or np.isnan(s).any() or not 0 <= int(stream) <= MAX_STREAM:
        return None
    return s[pos], s[~pos]


def boot(scores, labels, n_boot, seed=0, stream=0, fault=None, max_set=None):
    """[n_boot] int64: A2*_b of b = 1..n_boot (all -1 for a set that is not valid)."""
    pq = split(scores, labels, stream, max_set)
    if pq is None:
        return np.full(n_boot, -1, dtype=np.int64)
    p, q = pq
    out = np.empty(n_boot, dtype=np.int64)
    for b0 in range(1, n_boot + 1, 128):
        bs = np.arange(b0, min(b0 + 128, n_boot + 1))
        ip, iq = draws(len(p), len(q), bs, seed, stream, fault)
        for r in range(len(bs)):
            pv = p[ip[r]]
            if fault == "wrong_stratum":
                pv = pv.copy()
                pv[0] = q[iq[r][0]]
            out[b0 - 1 + r] = a2(pv, q[iq[r]], fault)
    return out


def stats(d, den, lo, hi):
    """(ci_lo, ci_hi, mean, se) of the integers d over the denominator den: integers until the last divisions."""
    d = [int(v) for v in d]
    n, srt, tot = len(d), sorted(d), sum(d)
    T = n * sum(v * v for v in d) - tot * tot
    se = math.sqrt(T / (n * (n - 1))) / den if n > 1 else float("nan")
    return srt[lo] / den, srt[hi] / den, tot / (n * den), se


def set_row(scores, labels, n_boot, lo, hi, seed=0, stream=0, fault=None, max_set=None, return_boot=False):
    """The set's [8] float64 row in the order of SET_COLUMNS (NaN where it is not valid), optionally with its A2*."""
    bt = boot(scores, labels, n_boot, seed, stream, fault, max_set)
    row = np.full(len(SET_COLUMNS), np.nan)
    pq = split(scores, labels, stream, max_set)
    if pq is not None:
        p, q = pq
        den = 2 * len(p) * len(q)
        row[0] = a2(p, q, fault) / den
        row[1:5] = stats(bt, den, lo, hi)
        row[5:] = n_boot, len(p), len(q)
    return (row, bt) if return_boot else row


def pair_row(set_a, set_c, n_boot, lo, hi, seed=0, fault=None, max_set=None):
    """The [8] float64 row in the order of PAIR_COLUMNS of two sets given as (scores, labels, stream)."""
    row = np.full(len(PAIR_COLUMNS), np.nan)
    (sa, la, ka), (sc, lc, kc) = set_a, set_c
    pa, pc = split(sa, la, ka, max_set), split(sc, lc, kc, max_set)
    la, lc = np.asarray(la).reshape(-1) != 0, np.asarray(lc).reshape(-1) != 0
    if pa is None or pc is None or int(ka) != int(kc) or la.size != lc.size or not np.array_equal(la, lc):
        return row
    den = 2 * len(pa[0]) * len(pa[1])
    d = boot(sa, la, n_boot, seed, ka, fault, max_set) - boot(sc, lc, n_boot, seed, kc, fault, max_set)
    n_le0, n_ge0 = int((d <= 0).sum()), int((d >= 0).sum())
    row[0] = (a2(*pa, fault) - a2(*pc, fault)) / den
    row[1:5] = stats(d, den, lo, hi)
    row[5] = min(1.0, (2 * (1 + min(n_le0, n_ge0))) / (1 + n_boot))
    row[6:] = n_le0, n_ge0
    return row


def boot_indices(n_boot, ci):
    """lo = floor((1 - ci) / 2 * (n_boot - 1)), hi = n_boot - 1 - lo."""
    lo = int(math.floor((1.0 - ci) / 2.0 * (n_boot - 1)))
    return lo, n_boot - 1 - lo


def moment_bound(n_boot):
    """The relative bound on boot_mean / boot_se between two correct implementations: 4 n_boot 2^-52 (fp64 summation of
    n_boot integers in any order)."""
    return 4.0 * n_boot * 2.0 ** -52
