"""The chart pass restated in fp64 numpy (the definition in include/nmhip.h, nm_chart_t; csrc/nm_chart.inc), operation by
operation -- every numpy call below is one correctly rounded IEEE operation per element, in the kernel's order, so the
kernel's partials and chart can be held to this file bit for bit -- and an error bound of `mean` and `var_latent` against
exact arithmetic, derived from the operation counts with u = 2^-53.

Tile fold (one 128-row tile, one column; the values are the fp32 x_hat converted to fp64):
    slot r of the tile holds row r, slots from `live` on hold +0; wave w owns slots 16 w .. 16 w + 15
    wave sum      butterfly over the 16 slots: v = v + v[lane ^ k] for k = 1, 2, 4, 8 (every lane ends with the same value)
    tile sum      S = wave[0] + wave[1] + ... + wave[nw - 1], nw = ceil(live / 16), left to right
    mean_t        S / live
    M2_t          the same two reductions over d * d, d = value - mean_t (dead slots +0)
Merge (ascending tiles, n_a the rows merged so far, n_b the tile's rows):
    n = n_a + n_b; delta = mean_b - mean; mean = mean + (delta * n_b) / n; M2 = (M2 + M2_b) + ((delta * delta) * (n_a * n_b)) / n
Chart row: (mean, M2 / (n - 1), n, 0), or (NaN, NaN, n, -2) where n < 2 or the merged mean is not finite.

Bound (first order in u, the computed values standing in for the exact ones):
    tile mean     an element passes 4 butterfly additions and at most 7 wave additions, then the division:
                  |mean_t^ - mean_t| <= 12 u mean|x| =: e_t
    merged mean   a convex combination of its inputs (their errors propagate with weights that sum to 1) plus, per step,
                  the roundings of delta, the product, the quotient (3 u |delta| n_b / n) and the sum (u |mean|)
    tile M2       sum of non-negative terms: subtraction and product 3 u, 11 additions 11 u -- 14 u M2_t -- plus live e_t^2
                  for the centre (sum (x - c)^2 = M2 + live (c - mean)^2)
    merged M2     per step the term delta^2 n_a n_b / n with |delta^ - delta| <= e_a + e_b + u |delta| =: e_d:
                  ((2 |delta| + e_d) e_d + 4 u delta^2) n_a n_b / n; every piece passes at most 2 (T - 1) additions
    var_latent    bound(M2) / (n - 1) + u var
"""
import numpy as np

U = 2.0 ** -53
TILE = 128
COLUMNS = ("mean", "var_latent", "n_rows", "status")
_LANE = np.arange(16)


def _bfly(v):
    """[8, 16, D] -> [8, D]: the butterfly over the 16 row lanes of every wave."""
    for k in (1, 2, 4, 8):
        v = v + v[:, _LANE ^ k, :]
    return v[:, 0, :]


def _waves(s, nw):
    acc = s[0]
    for w in range(1, nw):
        acc = acc + s[w]
    return acc


def tile_fold(x):
    """x [live <= 128, D] float32: one tile's rows -> (mean_t [D], M2_t [D]) float64, the kernel's operations."""
    x = np.asarray(x)
    assert x.dtype == np.float32 and x.ndim == 2 and 1 <= x.shape[0] <= TILE
    live, D = x.shape
    nw = (live + 15) // 16
    with np.errstate(all="ignore"):
        v = np.zeros((TILE, D), dtype=np.float64)
        v[:live] = x.astype(np.float64)
        mean = _waves(_bfly(v.reshape(8, 16, D)), nw) / np.float64(live)
        d = v - mean
        q = d * d
        q[live:] = 0.0
        m2 = _waves(_bfly(q.reshape(8, 16, D)), nw)
    return mean, m2


def tile_rows(n_rows, t):
    """Rows of tile t of a request of n_rows rows."""
    return min(TILE, n_rows - t * TILE)


def partials(x):
    """x [n, D] float32 -> [T, D, 2] float64: (mean_t, M2_t) per 128-row tile, the layout of one cell of nm_chart_t.part."""
    x = np.asarray(x)
    n = x.shape[0]
    T = (n + TILE - 1) // TILE
    out = np.zeros((T, x.shape[1], 2), dtype=np.float64)
    for t in range(T):
        out[t, :, 0], out[t, :, 1] = tile_fold(x[t * TILE:t * TILE + tile_rows(n, t)])
    return out


def merge(part, n_rows, counts=None):
    """part [T, D, 2], the request's row count -> the chart rows [D, 4].  counts: the rows per tile (default: what n_rows
    and the tile index say -- the seeded-fault tests pass wrong ones)."""
    part = np.asarray(part, dtype=np.float64)
    T = part.shape[0]
    counts = [tile_rows(n_rows, t) for t in range(T)] if counts is None else list(counts)
    with np.errstate(all="ignore"):
        na = np.float64(counts[0])
        mean, m2 = part[0, :, 0].copy(), part[0, :, 1].copy()
        for t in range(1, T):
            nb = np.float64(counts[t])
            n = na + nb
            delta = part[t, :, 0] - mean
            mean = mean + (delta * nb) / n
            m2 = (m2 + part[t, :, 1]) + ((delta * delta) * (na * nb)) / n
            na = n
        out = np.zeros((part.shape[1], 4), dtype=np.float64)
        bad = ~np.isfinite(mean) if na >= 2 else np.ones_like(mean, dtype=bool)
        out[:, 0] = np.where(bad, np.nan, mean)
        out[:, 1] = np.where(bad, np.nan, m2 / (na - 1.0)) if na >= 2 else np.nan
        out[:, 2] = na
        out[:, 3] = np.where(bad, -2.0, 0.0)
    return out


def chart(x):
    """x [n, D] float32 (one cell's x_hat over the request's rows) -> [D, 4] float64 under COLUMNS."""
    x = np.asarray(x)
    return merge(partials(x), x.shape[0])


def bound(x):
    """x [n, D] float32, n >= 2, finite -> (b_mean [D], b_var [D]): the bound of the module's docstring for |chart - exact|."""
    x = np.asarray(x)
    n, D = x.shape
    T = (n + TILE - 1) // TILE
    x64 = x.astype(np.float64)
    part = partials(x)
    e = None
    na, mean, m2, b2 = 0.0, None, None, None
    for t in range(T):
        nb = float(tile_rows(n, t))
        rows = x64[t * TILE:t * TILE + int(nb)]
        e_t = 12.0 * U * np.abs(rows).sum(axis=0) / nb
        b_t = 14.0 * U * part[t, :, 1] + nb * e_t * e_t
        if t == 0:
            na, mean, m2, e, b2 = nb, part[0, :, 0], part[0, :, 1], e_t, b_t
            continue
        nn = na + nb
        delta = part[t, :, 0] - mean
        e_d = e + e_t + U * np.abs(delta)
        b2 = b2 + b_t + ((2.0 * np.abs(delta) + e_d) * e_d + 4.0 * U * delta * delta) * (na * nb / nn)
        new_mean = mean + (delta * nb) / nn
        e = np.maximum(e, e_t) + U * np.abs(new_mean) + 3.0 * U * np.abs(delta) * (nb / nn)
        m2 = (m2 + part[t, :, 1]) + ((delta * delta) * (na * nb)) / nn
        mean, na = new_mean, nn
    b2 = b2 + 2.0 * (T - 1) * U * m2
    var = m2 / (n - 1.0)
    return e, b2 / (n - 1.0) + U * var
