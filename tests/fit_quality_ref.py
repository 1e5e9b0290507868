"""The numpy yardstick of the model-fit entry points (nm_fit_quality, nm_fit_rank; include/nmhip.h has the definitions): float64
throughout, vectorised over the columns, the same status rules.  The inputs are the fp32 tables the device reads.
tests/test_fit_quality_ref_cpu.py holds this file to scipy / sklearn code that shares nothing with it and measures its own
summation-order noise, which is what the tolerance of `close` rests on."""
import numpy as np
from scipy import special

STRIDE = 8
TOL = 1e-9
FIT = ("rho", "p_rho", "smse", "expv", "msll", "rmse", "n_obs", "status")
CAL = ("bias", "mae", "mean_z", "sd_z", "skew_z", "kurt_z", "coverage", "n_var")
RANK = ("spearman", "p_spearman", "t_spearman", "n_obs", "n_tied_y", "n_tied_loc", "reserved", "status")


def student_t_two_sided(t, df):
    """P(|T_df| >= |t|) = I_x(df / 2, 1 / 2) at x = df / (df + t^2); 0 at t = +-inf."""
    t = np.asarray(t, dtype=np.float64)
    with np.errstate(all="ignore"):
        p = special.betainc(0.5 * df, 0.5, df / (df + t * t))
    return np.where(np.isinf(t), 0.0, p)


def _t_and_p(r, n):
    """t = r sqrt((n - 2) / ((1 - r)(1 + r))), one operation at a time, and its p; r^2 >= 1: t = +-inf, p = 0."""
    with np.errstate(all="ignore"):
        one = r * r >= 1.0
        t = r * np.sqrt(np.float64(n - 2) / ((1.0 - r) * (1.0 + r)))
        t = np.where(one, np.where(r > 0, np.inf, -np.inf), t)
        p = np.where(one, 0.0, student_t_two_sided(np.where(one, 0.0, t), n - 2))
    return np.where(np.isnan(r), np.nan, t), np.where(np.isnan(r), np.nan, p)


def s2_table(shape, var=None, col_var=None):
    """[rows, D] float64 s2 = var + col_var, or None when neither is given."""
    if var is None and col_var is None:
        return None
    s2 = np.zeros(shape)
    if var is not None:
        s2 = s2 + np.asarray(var, dtype=np.float64)
    if col_var is not None:
        s2 = s2 + np.asarray(col_var, dtype=np.float64)[None, :]
    return s2


def quality(x, loc, group, var=None, col_var=None, trivial=None, thr=1.96, ddof=0, flip_trivial=False, swap_see=False,
            strict_cover=False):
    """(fit [D, 8], cal [D, 8]) over the rows with group == 0.  trivial: the [D, 8] row of a cohort_moments table (or None).
    ddof, flip_trivial, swap_see, strict_cover: the seeded faults of the CPU test (ddof 1 in the z moments, the trivial term
    added instead of subtracted, See and SSE swapped, coverage with < on thr)."""
    x, loc = np.asarray(x, dtype=np.float64), np.asarray(loc, dtype=np.float64)
    D = x.shape[1]
    ev = np.asarray(group) == 0
    y, f = x[ev], loc[ev]
    n = y.shape[0]
    s2 = s2_table(x.shape, var, col_var)
    s2 = None if s2 is None else s2[ev]
    fit, cal = np.full((D, STRIDE), np.nan), np.full((D, STRIDE), np.nan)
    fit[:, 6] = n
    with np.errstate(all="ignore"):
        s2ok = np.zeros((n, D), dtype=bool) if s2 is None else np.isfinite(s2) & (s2 > 0)
        cal[:, 7] = s2ok.sum(0)
        fin = (np.isfinite(y) & np.isfinite(f)).all(0) if n else np.ones(D, dtype=bool)
        ok = fin & (n >= 2)
        if n >= 2:
            ok &= np.where(fin, y.max(0) > y.min(0), False)
        fit[:, 7] = -2.0
        if not ok.any():
            return fit, cal
        e = y - f
        my, mf, me = y.mean(0), f.mean(0), e.mean(0)
        Syy, Sff, Syf = ((y - my) ** 2).sum(0), ((f - mf) ** 2).sum(0), ((y - my) * (f - mf)).sum(0)
        See, SSE = ((e - me) ** 2).sum(0), (e * e).sum(0)
        if swap_see:
            See, SSE = SSE, See
        f_const = ~(f.max(0) > f.min(0))
        rho = np.where(f_const, np.nan, Syf / np.sqrt(Syy * Sff))
        p_rho = _t_and_p(rho, n)[1] if n >= 3 else np.full(D, np.nan)
        b1 = f_const | (n < 3)
        b2 = ~s2ok.all(0) if s2 is not None else np.ones(D, dtype=bool)
        if trivial is None:
            b4, m_t, v_t = np.ones(D, dtype=bool), np.zeros(D), np.ones(D)
        else:
            trivial = np.asarray(trivial, dtype=np.float64)
            b4 = ~((trivial[:, 7] == 0) & (trivial[:, 2] > 0))
            m_t, v_t = trivial[:, 0], np.where(b4, 1.0, trivial[:, 2])
        s2s = np.where(s2ok, s2, 1.0) if s2 is not None else np.ones((n, D))
        z = e / np.sqrt(s2s)
        nll = (0.5 * np.log(2.0 * np.pi * s2s) + e * e / (2.0 * s2s)).mean(0)
        nll_t = 0.5 * np.log(2.0 * np.pi * v_t) + ((y - m_t) ** 2).sum(0) / (2.0 * v_t * n)
        msll = nll + nll_t if flip_trivial else nll - nll_t
        mz = z.mean(0)
        dz = z - mz
        m2 = (dz ** 2).sum(0) / n
        m3, m4 = (dz ** 3).mean(0), (dz ** 4).mean(0)
        sd = np.sqrt((dz ** 2).sum(0) / (n - ddof))
        cover = ((np.abs(z) < thr) if strict_cover else (np.abs(z) <= thr)).sum(0) / n
        cols_fit = [rho, p_rho, SSE / Syy, 1.0 - See / Syy, np.where(b2 | b4, np.nan, msll), np.sqrt(SSE / n)]
        for k, v in enumerate(cols_fit):
            fit[:, k] = np.where(ok, v, np.nan)
        fit[:, 7] = np.where(ok, b1 * 1.0 + b2 * 2.0 + b4 * 4.0, -2.0)
        cols_cal = [me, np.abs(e).sum(0) / n] + [np.where(b2, np.nan, v) for v in
                                                 (mz, sd, m3 / m2 ** 1.5, m4 / (m2 * m2) - 3.0, cover)]
        for k, v in enumerate(cols_cal):
            cal[:, k] = np.where(ok, v, np.nan)
    return fit, cal


def quality_raw(x, loc, group):
    """(smse, expv) by the raw form sum v^2 - (sum v)^2 / n: what the two-pass form is there to avoid."""
    ev = np.asarray(group) == 0
    y, f = np.asarray(x, dtype=np.float64)[ev], np.asarray(loc, dtype=np.float64)[ev]
    n, e = y.shape[0], y - f
    Syy = (y * y).sum(0) - y.sum(0) ** 2 / n
    See = (e * e).sum(0) - e.sum(0) ** 2 / n
    return (e * e).sum(0) / Syy, 1.0 - See / Syy


def k2(v, among=None):
    """[n, D] int64 k2 = #{a < v} + #{a <= v} per column (-0 == +0), a = the column of `among` (default: v itself)."""
    v = np.asarray(v, dtype=np.float64) + 0.0
    a = np.sort(v if among is None else np.asarray(among, dtype=np.float64) + 0.0, axis=0)
    out = np.empty(v.shape, dtype=np.int64)
    for d in range(v.shape[1]):
        out[:, d] = np.searchsorted(a[:, d], v[:, d], side="left") + np.searchsorted(a[:, d], v[:, d], side="right")
    return out


def rank(x, loc, group, cross=False):
    """[D, 8] = spearman, p_spearman, t_spearman, n_obs, n_tied_y, n_tied_loc, 0, status over the rows with group == 0; the sums
    in exact integers.  cross: the seeded fault of the CPU test (the k2 of loc taken in the sort of x)."""
    ev = np.asarray(group) == 0
    y, f = np.asarray(x, dtype=np.float32)[ev], np.asarray(loc, dtype=np.float32)[ev]
    n, D = y.shape
    out = np.full((D, STRIDE), np.nan)
    out[:, 3], out[:, 6], out[:, 7] = n, 0.0, -2.0
    ok = (np.isfinite(y) & np.isfinite(f)).all(0) & (n >= 2) if n else np.zeros(D, dtype=bool)
    if not ok.any():
        return out
    ys, fs = np.where(np.isfinite(y), y, 0.0), np.where(np.isfinite(f), f, 0.0)
    ky, kf = k2(ys), k2(fs, among=ys if cross else None)
    nn = int(n)
    for d in np.nonzero(ok)[0]:
        a, b = ky[:, d], kf[:, d]                                  # (int64 sums below 2^42, then python integers: exact)
        sab, sa, sb, saa, sbb = (int(v) for v in (np.dot(a, b), a.sum(), b.sum(), np.dot(a, a), np.dot(b, b)))
        A, B, C = nn * sab - sa * sb, nn * saa - sa * sa, nn * sbb - sb * sb
        out[d, 4], out[d, 5] = _tied(ys[:, d]), _tied(fs[:, d])
        flat = B == 0 or C == 0
        out[d, 7] = 1.0 if (flat or n < 3) else 0.0
        if flat:
            continue
        rs = np.float64(A) / np.sqrt(np.float64(B) * np.float64(C))
        out[d, 0] = rs
        if n >= 3:
            t, p = _t_and_p(np.float64(rs), n)
            out[d, 2], out[d, 1] = t, p
    return out


def _tied(col):
    _, inv, cnt = np.unique(col + 0.0, return_inverse=True, return_counts=True)
    return int((cnt[inv] > 1).sum())


def close(got, ref, kind, tol=TOL):
    """The closeness rules; returns the worst error over its bound (<= 1 passes; inf where a NaN pattern, a status word or a
    count differs).  kind:
      "fit"   n_obs, status and the NaN pattern exactly; p_rho within tol relative; the rest within tol x max(1, |ref|)
      "cal"   n_var and the NaN pattern exactly; the rest within tol x max(1, |ref|)
      "rank"  n_obs, n_tied_y, n_tied_loc, the reserved word, status and the NaN pattern exactly; spearman and t_spearman bit
              for bit (the integers are exact and the last operations are stated one by one); p_spearman within tol relative
    tol = 1e-9, the rule of tests/normative_ref.py: tests/test_fit_quality_ref_cpu.py measures this file's own summation-order
    noise (the same table with its rows permuted) at or below 1e-12 for every column, kurtosis included."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    if got.shape != ref.shape or not np.array_equal(np.isnan(got), np.isnan(ref)):
        return np.inf
    exact = {"fit": [6, 7], "cal": [7], "rank": [0, 2, 3, 4, 5, 6, 7]}[kind]
    relative = {"fit": [1], "cal": [], "rank": [1]}[kind]
    worst = 0.0
    with np.errstate(all="ignore"):
        for k in range(STRIDE):
            g, r = got[..., k], ref[..., k]
            m = ~np.isnan(r)
            if k in exact:
                if not np.array_equal(g[m].view(np.int64) if kind == "rank" and k in (0, 2) else g[m],
                                      r[m].view(np.int64) if kind == "rank" and k in (0, 2) else r[m]):
                    return np.inf
                continue
            bound = tol * (np.abs(r[m]) if k in relative else np.maximum(1.0, np.abs(r[m])))
            err = np.abs(g[m] - r[m])
            err = np.where(g[m] == r[m], 0.0, err)                  # (equal infinities)
            nz = err != 0
            if np.any(nz):
                worst = max(worst, float((err[nz] / bound[nz]).max()))
    return worst if worst == worst else np.inf


def make_case(rng, rows, D, groups=(-1, 0, 1, 2), r2=0.6):
    """A synthetic observed table, a prediction that explains about r2 of it, a per-element and a per-column variance (all
    fp32) and the group words: columns of different scales and offsets."""
    scale, off = rng.uniform(0.5, 3.0, D), rng.uniform(-5.0, 5.0, D)
    sig = rng.normal(size=(rows, D))
    x = ((np.sqrt(r2) * sig + np.sqrt(1 - r2) * rng.normal(size=(rows, D))) * scale + off).astype(np.float32)
    loc = (np.sqrt(r2) * sig * scale * rng.uniform(0.7, 1.1, D) + off + rng.uniform(-0.2, 0.2, D)).astype(np.float32)
    var = (rng.uniform(0.05, 0.4, (rows, D)) * scale ** 2).astype(np.float32)
    col_var = (rng.uniform(0.1, 0.5, D) * scale ** 2).astype(np.float32)
    g = rng.choice(np.asarray(groups), size=rows).astype(np.int32)
    return x, loc, var, col_var, g
