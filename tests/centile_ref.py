"""The yardstick of the normative centiles (nm_cohort_quantiles, nm_normative_centile, metrics.robust_moments): a numpy
restatement of include/nmhip.h, operation by operation in fp64, so the kernels are held to it bit for bit.
tests/test_centile_ref_cpu.py holds the restatement itself to numpy and scipy with ==."""
import numpy as np

INVALID = 0xFFFF
NAN = float("nan")


def values(x, sub=None):
    """v = (double)x - (double)sub, or x."""
    v = np.asarray(x, dtype=np.float32).astype(np.float64)
    if sub is not None:
        v = v - np.asarray(sub, dtype=np.float32).astype(np.float64)
    return v


def sorted_ref(col):
    """The reference values of one column, ascending, -0 and +0 one value (+0)."""
    return np.sort(np.asarray(col, dtype=np.float64) + 0.0)


def quantile(a, p):
    """np.quantile(method="linear") of the sorted a at p, one operation at a time."""
    n = len(a)
    top = np.float64(n - 1)
    h = top * np.float64(p)
    jf = np.floor(h)
    g = h - jf
    if h >= top:
        lo = hi = a[n - 1]
    else:
        lo, hi = a[int(jf)], a[int(jf) + 1]
    d = hi - lo
    r = lo + d * g
    if g >= 0.5:
        r = hi - d * (np.float64(1.0) - g)
    return np.float64(r)


def median(a):
    """np.median of the sorted a."""
    n = len(a)
    if n & 1:
        return np.float64(a[n >> 1])
    return np.float64((a[n // 2 - 1] + a[n // 2]) / np.float64(2.0))


def mad(a, med):
    """The same median of |v - median|, by a second sort."""
    return median(sorted_ref(np.abs(a - med)))


def cohort_quantiles(x, group, probs, sub=None):
    """(q [D, n_q], stats [D, 8]) of one set, or of a refused set with x = None."""
    probs = [float(p) for p in probs]
    if x is None:
        raise ValueError("a refused set has no table: use refused_quantiles")
    v = values(x, sub)
    g = np.asarray(group)
    D = v.shape[1]
    q = np.full((D, len(probs)), NAN)
    st = np.full((D, 8), NAN)
    ref = v[g == 0]
    n = ref.shape[0]
    with np.errstate(all="ignore"):
        for c in range(D):
            nbad = int(np.count_nonzero(~np.isfinite(ref[:, c])))
            st[c, 5], st[c, 6], st[c, 7] = n, nbad, -2.0
            if n < 1 or nbad:
                continue
            a = sorted_ref(ref[:, c])
            for k, p in enumerate(probs):
                q[c, k] = quantile(a, p)
            med = median(a)
            q1, q3 = quantile(a, 0.25), quantile(a, 0.75)
            st[c] = [med, mad(a, med), q1, q3, q3 - q1, n, 0.0, 0.0]
    return q, st


def refused_quantiles(D, n_q):
    q = np.full((D, n_q), NAN)
    st = np.full((D, 8), NAN)
    st[:, 5], st[:, 6], st[:, 7] = 0.0, 0.0, -2.0
    return q, st


def k2_table(x, group, ref_x, ref_group, sub=None, ref_sub=None, self_loo=False):
    """(k2 [rows, D] int64 with INVALID marks, n_ref): every row of the scored table ranked in the reference columns.
    self_loo: the scored set is its own reference and loo is on -- its group-0 rows are ranked among the other n - 1."""
    v = values(x, sub)
    g = np.asarray(group)
    rv = values(ref_x, ref_sub)[np.asarray(ref_group) == 0]
    n = rv.shape[0]
    k2 = np.full(v.shape, INVALID, dtype=np.int64)
    for c in range(v.shape[1]):
        if n < 1 or not np.all(np.isfinite(rv[:, c])):
            continue
        a = sorted_ref(rv[:, c])
        fin = np.isfinite(v[:, c])
        vv = np.where(fin, v[:, c], 0.0)
        k = np.searchsorted(a, vv, "left") + np.searchsorted(a, vv, "right")
        ok = fin.copy()
        if self_loo:
            own = g == 0
            k = k - own
            if n - 1 == 0:
                ok &= ~own
        k2[:, c] = np.where(ok, k, INVALID)
    return k2, n


def divisors(group, n, self_loo):
    g = np.asarray(group)
    return np.where((g == 0) & bool(self_loo), n - 1, n).astype(np.int64)


def pct_table(k2, nd):
    """fp64 pct [rows, D], NaN where invalid: (double)k2 * (50.0 / (double)n)."""
    with np.errstate(all="ignore"):
        f = np.float64(50.0) / nd.astype(np.float64)
        return np.where(k2 != INVALID, k2.astype(np.float64) * f[:, None], NAN)


def row_summary(k2, nd, tail):
    rows = k2.shape[0]
    out = np.zeros((rows, 8))
    valid = k2 != INVALID
    pct = pct_table(k2, nd)
    with np.errstate(all="ignore"):
        f = np.float64(50.0) / nd.astype(np.float64)
        nv = valid.sum(1)
        out[:, 0] = (valid & (pct > np.float64(100.0) - np.float64(tail))).sum(1)
        out[:, 1] = (valid & (pct < np.float64(tail))).sum(1)
        sk = np.where(valid, k2, 0).sum(1)
        sa = np.where(valid, np.abs(k2 - nd[:, None]), 0).sum(1)
        has = nv > 0
        out[:, 2] = np.where(has, sk.astype(np.float64) * f / nv.astype(np.float64), NAN)
        out[:, 3] = np.where(has, sa.astype(np.float64) * f / nv.astype(np.float64), NAN)
        kk = np.where(valid, k2, -1)
        am = kk.argmax(1) if k2.shape[1] else np.zeros(rows, dtype=np.int64)
        mk = kk.max(1) if k2.shape[1] else np.full(rows, -1)
        out[:, 4] = np.where(has, mk.astype(np.float64) * f, NAN)
        out[:, 5] = np.where(has, am, -1)
        out[:, 6] = nv
        out[:, 7] = np.where(has, 0.0, -2.0)
    return out


def refused_rows(rows):
    out = np.zeros((rows, 8))
    out[:, 2:5] = NAN
    out[:, 5], out[:, 7] = -1.0, -2.0
    return out


def col_summary(k2, group, n, self_loo, tail):
    g = np.asarray(group)
    D = k2.shape[1]
    out = np.zeros((D, 8))
    valid = k2 != INVALID
    with np.errstate(all="ignore"):
        for which, c_hi, c_lo, c_n, c_mean, div in ((1, 0, 1, 4, 6, n), (0, 2, 3, 5, 7, n - 1 if self_loo else n)):
            f = np.float64(50.0) / np.float64(div)
            m = valid & (g == which)[:, None]
            pct = k2.astype(np.float64) * f
            out[:, c_hi] = (m & (pct > np.float64(100.0) - np.float64(tail))).sum(0)
            out[:, c_lo] = (m & (pct < np.float64(tail))).sum(0)
            cnt = m.sum(0)
            s = np.where(m, k2, 0).sum(0)
            out[:, c_n] = cnt
            out[:, c_mean] = np.where(cnt > 0, s.astype(np.float64) * f / cnt.astype(np.float64), NAN)
    return out


def normative_centile(sets, ref_of=None, tail=2.5, loo=False, refused=()):
    """The whole entry point over a list of sets (x, group, sub or None): per set (pct32 or None, rows or None, cols).
    ref_of as the C entry point takes it (-1: a reference only; outside -1..n-1: the set's own refusal); refused: indices of
    sets whose table entry the kernel refuses (as scored sets: status rows, NaN cols; as references: every element invalid)."""
    n_sets = len(sets)
    ref = list(range(n_sets)) if ref_of is None else [int(r) for r in ref_of]
    out = []
    for s, (x, g, sub) in enumerate(sets):
        D = np.asarray(x).shape[1]
        rows = np.asarray(x).shape[0]
        if ref[s] == -1:
            out.append((None, None, np.full((D, 8), NAN)))
            continue
        if s in refused:
            out.append((None, refused_rows(rows), np.full((D, 8), NAN)))
            continue
        if not 0 <= ref[s] < n_sets or ref[s] in refused:
            out.append((np.full((rows, D), NAN, dtype=np.float32), refused_rows(rows), np.full((D, 8), NAN)))
            continue
        rx, rg, rsub = sets[ref[s]]
        self_loo = bool(loo) and ref[s] == s
        k2, n = k2_table(x, g, rx, rg, sub, rsub, self_loo)
        nd = divisors(g, n, self_loo)
        out.append((pct_table(k2, nd).astype(np.float32), row_summary(k2, nd, tail), col_summary(k2, g, n, self_loo, tail)))
    return out


def robust_moments(stats, scale=1.4826):
    st = np.asarray(stats, dtype=np.float64)
    out = np.full(st.shape, NAN)
    sd = np.float64(scale) * st[..., 1]
    out[..., 0] = st[..., 0]
    out[..., 1] = sd
    out[..., 2] = sd * sd
    out[..., 3] = st[..., 5]
    out[..., 6] = st[..., 6]
    out[..., 7] = np.where((st[..., 7] == -2.0) | (st[..., 1] == 0.0), -2.0, 0.0)
    return out
