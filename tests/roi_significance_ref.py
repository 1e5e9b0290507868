"""The yardstick of nm_roi_significance (own code, int64 / uint64 / float64), by the definitions of include/nmhip.h.

The included rows of a set are its rows with group 0 or 1, in row order, at positions i = 0..n-1; n_x have group 1 (X), n_y
group 0 (Y).  A column is valid if n_x >= 1, n_y >= 1 and no included row holds a NaN in it.

    r2[i]      twice the mid-rank of row i in its column, from np.unique's inverse and counts (-0 == +0, inf == inf)
    tie_term   sum over tie groups of t^3 - t                    S = sum_{i in X} r2[i] - n_x (n + 1)
    u_x        (S + n_x n_y) / 2
    a = n_x n_y / 12;  b = tie_term / (n (n - 1));  s = sqrt(a ((n + 1) - b));  zabs = s > 0 ? max(|S| / 2 - 1/2, 0) / s : 0
    z = copysign(zabs, S);  p_mwu = erfc(zabs / sqrt(2))         (math.erfc, one float64 operation at a time)
    q_bh       over the m valid columns, p ascending: min(1, min_{j >= i} p_(j) * (m / j))
    labels     permutation t = 1..n_perm of set k: h = splitmix64(seed ^ 0x5160C0DE ^ (k << 40) ^ (t << 16) ^ i), the sort
               key (h & ~0x1FFF) | i; the n_x positions with the smallest keys are X*
    S*         labels @ r2 - n_x (n + 1) in int64;  maxstat_t = max over valid columns of |S*_t|
    p_perm     (1 + #{t: |S*_t,c| >= |S_c|}) / (1 + n_perm);  p_maxt with maxstat_t in place of |S*_t,c|;  NaN with n_perm = 0

`table` gives the [D, 8] float64 table in the order of COLUMNS; `parts` everything in between, for the tests that look inside.
The keyword `fault` plants one named defect (the CPU tests show that each one changes the output)."""
import math

import numpy as np

COLUMNS = ("u_x", "tie_term", "z", "p_mwu", "q_bh", "p_perm", "p_maxt", "n_perm")
M64 = (1 << 64) - 1


def splitmix64(x):
    """splitmix64 on a uint64 array (wrapping arithmetic)."""
    x = np.asarray(x, dtype=np.uint64)
    with np.errstate(over="ignore"):
        x = x + np.uint64(0x9E3779B97F4A7C15)
        x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return x ^ (x >> np.uint64(31))


def labels(n, n_x, n_perm, seed, k=0):
    """[n_perm, n] int64 of 0 / 1: row t - 1 marks X* of permutation t of set k (256 permutations at a time)."""
    out = np.zeros((n_perm, n), dtype=np.int64)
    i = np.arange(n, dtype=np.uint64)[None, :]
    fixed = (int(seed) ^ 0x5160C0DE ^ (int(k) << 40)) & M64
    for t0 in range(1, n_perm + 1, 256):
        t = np.arange(t0, min(t0 + 256, n_perm + 1), dtype=np.uint64)[:, None]
        h = splitmix64(np.uint64(fixed) ^ (t << np.uint64(16)) ^ i)
        key = (h & np.uint64(M64 ^ 0x1FFF)) | i
        first = np.argsort(key, axis=1, kind="stable")[:, :n_x]
        np.put_along_axis(out[t0 - 1:t0 - 1 + len(t)], first, 1, axis=1)
    return out


def ranks2(col):
    """(twice the mid-ranks, tie term) of a 1-D float array without NaN, both int64."""
    _, inv, cnt = np.unique(col, return_inverse=True, return_counts=True)      # -0.0 == 0.0 and inf == inf: one value each
    cnt = cnt.astype(np.int64)
    end = np.cumsum(cnt)                                   # ranks end - cnt + 1 .. end: twice their mean is 2 end - cnt + 1
    return (2 * end - cnt + 1)[inv.reshape(-1)], int((cnt ** 3 - cnt).sum())


def bh(p):
    """Benjamini-Hochberg q of a 1-D float64 array: p ascending as p_(1..m), q_(i) = min(1, min_{j >= i} p_(j) * (m / j))."""
    p = np.asarray(p, dtype=np.float64)
    m = p.size
    if m == 0:
        return p.copy()
    order = np.argsort(p, kind="stable")
    v = p[order] * (np.float64(m) / np.arange(1, m + 1, dtype=np.float64))
    v = np.minimum.accumulate(v[::-1])[::-1]
    q = np.empty(m)
    q[order] = np.minimum(v, 1.0)
    return q


def z_p(n, n_x, S, tie):
    """(z, p_mwu) of one valid column, every operation on its own in float64."""
    n_y = n - n_x
    a = np.float64(n_x * n_y) / np.float64(12.0)
    b = np.float64(tie) / (np.float64(n) * np.float64(n - 1))
    s = np.sqrt(a * (np.float64(n + 1) - b))
    zabs = max(np.float64(abs(S)) * np.float64(0.5) - np.float64(0.5), np.float64(0.0)) / s if s > 0 else np.float64(0.0)
    return float(np.copysign(zabs, np.float64(S))), math.erfc(float(zabs / np.sqrt(np.float64(2.0))))


def parts(x, group, n_perm=0, seed=0, k=0, fault=None):
    """Everything the table is made of, for one set: x [rows, D], group [rows] (1 = X, 0 = Y, else left out)."""
    x = np.asarray(x, dtype=np.float64)
    group = np.asarray(group).reshape(-1)
    D = x.shape[1]
    inc = (group == 0) | (group == 1)
    xi, gi = x[inc], group[inc]
    n, n_x = int(inc.sum()), int((gi == 1).sum())
    n_y = n - n_x
    valid = np.zeros(D, dtype=bool) if (n_x < 1 or n_y < 1) else ~np.isnan(xi).any(0)
    r2 = np.zeros((n, D), dtype=np.int64)
    tie = np.zeros(D, dtype=np.int64)
    for c in np.flatnonzero(valid):
        col = xi[:, c]
        if fault == "tie_group_split" and c == 0:          # the members of the first tie group ranked one by one
            _, inv, cnt = np.unique(col, return_inverse=True, return_counts=True)
            g = int(np.flatnonzero(cnt > 1)[0])
            col = col.copy()
            col[np.flatnonzero(inv.reshape(-1) == g)[0]] = np.nextafter(col[np.flatnonzero(inv.reshape(-1) == g)[0]], -np.inf)
        r2[:, c], tie[c] = ranks2(col)
    if fault == "rank_off_by_one" and valid.any():
        r2[np.flatnonzero(gi == 1)[0], np.flatnonzero(valid)[0]] += 2
    S = (r2[gi == 1].sum(0) - n_x * (n + 1)) * valid
    lab = labels(n, n_x, n_perm, seed, k) if valid.any() else np.zeros((n_perm, n), dtype=np.int64)
    if fault == "label_flipped" and n_perm:
        lab[0, 0] ^= 1
    Sp = (lab @ r2 - n_x * (n + 1)) if n_perm else np.zeros((0, D), dtype=np.int64)
    over = valid if fault != "max_over_invalid" else np.ones(D, dtype=bool)
    maxstat = np.abs(Sp[:, over]).max(1) if over.any() and valid.any() else np.full(n_perm, -1, dtype=np.int64)
    return dict(n=n, n_x=n_x, n_y=n_y, valid=valid, r2=r2, tie=tie, S=S, labels=lab, S_perm=Sp, maxstat=maxstat.astype(np.int64))


def table(x, group, n_perm=0, seed=0, k=0, fault=None, return_parts=False):
    """[D, 8] float64 in the order of COLUMNS for set k."""
    P = parts(x, group, n_perm, seed, k, fault)
    D = P["valid"].size
    out = np.full((D, len(COLUMNS)), np.nan)
    v = np.flatnonzero(P["valid"])
    n, n_x, n_y = P["n"], P["n_x"], P["n_y"]
    for c in v:
        S = int(P["S"][c])
        z, p = z_p(n, n_x, S, int(P["tie"][c]))
        out[c, 0] = np.float64(S + n_x * n_y) * 0.5
        out[c, 1], out[c, 2], out[c, 3] = np.float64(P["tie"][c]), z, p
        if n_perm:
            out[c, 5] = np.float64(1 + int((np.abs(P["S_perm"][:, c]) >= abs(S)).sum())) / np.float64(1 + n_perm)
            out[c, 6] = np.float64(1 + int((P["maxstat"] >= abs(S)).sum())) / np.float64(1 + n_perm)
        out[c, 7] = np.float64(n_perm)
    out[v, 4] = bh(out[v, 3])
    return (out, P) if return_parts else out


def p_bound(z):
    """The relative bound on p_mwu between two correct implementations: 16 (z^2 + 4) 2^-52.  d ln erfc(a) / d ln a ~ -2 a^2
    with a^2 = z^2 / 2, and 16 units for the roundings of s, of the argument and of the two erfc implementations."""
    return 16.0 * (np.asarray(z, dtype=np.float64) ** 2 + 4.0) * 2.0 ** -52
