"""The numpy yardstick of the normative z-map entry points (nm_cohort_moments, nm_normative_z, nm_cohort_cov, nm_mahalanobis;
include/nmhip.h has the definitions): float64 throughout, vectorised, the same status rules.  The inputs are the fp32 tables
the device reads (and the optional `sub` matrix: the value is x - sub in float64).  tests/test_normative_ref_cpu.py holds this
file to scipy / numpy code that shares nothing with it."""
import numpy as np

STRIDE = 8
EPS = 2.0 ** -52


def values(x, sub=None):
    v = np.asarray(x, dtype=np.float64)
    return v if sub is None else v - np.asarray(sub, dtype=np.float64)


def moments(x, group, sub=None, ddof=1):
    """[D, 8] = mean, sd, var, n_ref, min, max, n_nonfinite, status over the rows with group == 0."""
    v = values(x, sub)
    D = v.shape[1]
    ref = v[np.asarray(group) == 0]
    n = ref.shape[0]
    out = np.full((D, STRIDE), np.nan)
    fin = np.isfinite(ref)
    out[:, 3] = n
    out[:, 6] = (~fin).sum(0)
    with np.errstate(all="ignore"):
        any_fin = fin.any(0) if n else np.zeros(D, dtype=bool)
        out[:, 4] = np.where(any_fin, np.where(fin, ref, np.inf).min(0, initial=np.inf), np.nan)
        out[:, 5] = np.where(any_fin, np.where(fin, ref, -np.inf).max(0, initial=-np.inf), np.nan)
        ok = (n > ddof) & (out[:, 6] == 0) & (out[:, 5] > out[:, 4])
        if n > ddof:
            mean = ref.mean(0)
            var = ((ref - mean) ** 2).sum(0) / (n - ddof)          # two passes
            out[:, 0] = np.where(ok, mean, np.nan)
            out[:, 1] = np.where(ok, np.sqrt(var), np.nan)
            out[:, 2] = np.where(ok, var, np.nan)
    out[:, 7] = np.where(ok, 0.0, -2.0)
    return out


def moments_raw(x, group, ddof=1):
    """(mean, var) by the raw form E[x^2] - E[x]^2: what the two-pass form is there to avoid."""
    ref = np.asarray(x, dtype=np.float64)[np.asarray(group) == 0]
    n = ref.shape[0]
    mean = ref.sum(0) / n
    return mean, ((ref * ref).sum(0) / n - mean * mean) * n / (n - ddof)


def z_table(x, mom, sub=None):
    """[rows, D] float64 z = (v - mean) / sd; NaN where v is not finite or the column's moments are not valid."""
    v = values(x, sub)
    with np.errstate(all="ignore"):
        z = (v - mom[:, 0]) / mom[:, 1]
    z[~np.isfinite(v)] = np.nan
    z[:, ~((mom[:, 7] == 0) & (mom[:, 1] > 0))] = np.nan
    return z


def row_summary(z, thr=1.96):
    """[rows, 8] = n_hi, n_lo, mean_z, mean_abs_z, max_z, argmax_z, n_valid, status over the non-NaN z of a row."""
    valid = ~np.isnan(z)
    nv = valid.sum(1)
    out = np.full((z.shape[0], STRIDE), np.nan)
    with np.errstate(all="ignore"):
        out[:, 0] = (valid & (z > thr)).sum(1)
        out[:, 1] = (valid & (z < -thr)).sum(1)
        z0 = np.where(valid, z, 0.0)
        out[:, 2] = np.where(nv > 0, z0.sum(1) / np.maximum(nv, 1), np.nan)
        out[:, 3] = np.where(nv > 0, np.abs(z0).sum(1) / np.maximum(nv, 1), np.nan)
        zm = np.where(valid, z, -np.inf)
        out[:, 4] = np.where(nv > 0, zm.max(1, initial=-np.inf), np.nan)
        out[:, 5] = np.where(nv > 0, zm.argmax(1) if z.shape[1] else -1, -1)
    out[:, 6] = nv
    out[:, 7] = np.where(nv > 0, 0.0, -2.0)
    return out


def col_summary(z, group, mom, thr=1.96):
    """[D, 8] = n_hi_x, n_lo_x, n_hi_y, n_lo_y, n_x, n_y, mean_z_x, mean_z_y; x = group 1, y = group 0, over the non-NaN z."""
    group = np.asarray(group)
    D = z.shape[1]
    out = np.zeros((D, STRIDE))
    for base, g in ((0, 1), (1, 0)):
        zz = z[group == g]
        valid = ~np.isnan(zz)
        n = valid.sum(0)
        out[:, 2 * base + 0] = (valid & (zz > thr)).sum(0)
        out[:, 2 * base + 1] = (valid & (zz < -thr)).sum(0)
        out[:, 4 + base] = n
        with np.errstate(all="ignore"):
            out[:, 6 + base] = np.where(n > 0, np.where(valid, zz, 0.0).sum(0) / np.maximum(n, 1), np.nan)
    bad = ~((mom[:, 7] == 0) & (mom[:, 1] > 0))
    out[bad, :6] = 0.0
    out[bad, 6:] = np.nan
    return out


def cov_chol(x, group, ridge=0.0, sub=None, transposed=False):
    """(mean [Z], chol [Z, Z] lower, status): the reference rows' means, the Cholesky factor of their sample covariance
    (ddof 1) + ridge I.  status -2 (a NaN factor): n_ref < 2, a non-finite value, n_ref <= Z with ridge == 0, a pivot
    <= Z 2^-52 max diag.  transposed: the seeded fault of the CPU test (the upper factor in the lower's place)."""
    v = values(x, sub)
    Z = v.shape[1]
    ref = v[np.asarray(group) == 0]
    n = ref.shape[0]
    nanL = np.full((Z, Z), np.nan)
    if n < 1 or not np.all(np.isfinite(ref)):
        return np.full(Z, np.nan), nanL, -2
    mean = ref.mean(0)
    if n < 2 or (ridge == 0.0 and n <= Z):
        return mean, nanL, -2
    c = ref - mean
    A = c.T @ c / (n - 1) + ridge * np.eye(Z)
    tol = Z * EPS * A.diagonal().max()
    L = np.zeros((Z, Z))
    for j in range(Z):                                             # column by column, the pivot rule of the header
        s = A[j:, j] - L[j:, :j] @ L[j, :j]
        if not s[0] > tol:
            return mean, nanL, -2
        L[j, j] = np.sqrt(s[0])
        L[j + 1:, j] = s[1:] / L[j, j]
    return mean, (L.T.copy() if transposed else L), 0


def mahalanobis(x, mean, L, status, sub=None):
    """[rows] d2 = |L^-1 (v - mean)|^2 by forward substitution; NaN for a row with a non-finite entry or an invalid factor."""
    v = values(x, sub)
    n, Z = v.shape
    if status != 0:
        return np.full(n, np.nan)
    bad = ~np.isfinite(v).all(1)
    c = np.where(bad[:, None], 0.0, v - mean).T                    # [Z, rows]
    y = np.zeros_like(c)
    for k in range(Z):
        y[k] = (c[k] - L[k, :k] @ y[:k]) / L[k, k]
    d2 = (y * y).sum(0)
    d2[bad] = np.nan
    return d2


def close(got, ref, kind, tol=1e-9):
    """The closeness rules; returns the worst error over its bound (<= 1 passes; inf where a NaN pattern, a status word or a
    count differs).  kind:
      "moments"  n_ref, n_nonfinite, status exactly; mean and sd within tol x max(|mean|, sd); var within 2 tol relative;
                 min and max exactly (they are input values)
      "rows"     n_hi, n_lo, argmax_z, n_valid, status exactly; mean_z, mean_abs_z, max_z within tol x max(1, |ref|)
      "cols"     the six counts exactly; the two means within tol x max(1, |ref|)
      "z32"      float32 tables: within one fp32 ulp of the yardstick's z rounded to fp32
      "rel"      plain arrays (d2, the factor, the means): within tol x |ref| (tol x the largest |ref| for the factor)"""
    got, ref = np.asarray(got), np.asarray(ref)
    if got.shape != ref.shape or not np.array_equal(np.isnan(got), np.isnan(ref)):
        return np.inf
    worst = 0.0

    def upd(err, bound):
        nonlocal worst
        err, bound = np.asarray(err, dtype=np.float64), np.asarray(bound, dtype=np.float64)
        m = ~np.isnan(err) & (err != 0)
        if np.any(m):
            with np.errstate(divide="ignore"):
                worst = max(worst, float((err[m] / np.broadcast_to(bound, err.shape)[m]).max()))

    def exact(cols):
        g, r = got[..., cols], ref[..., cols]
        return np.array_equal(np.isnan(g), np.isnan(r)) and np.array_equal(g[~np.isnan(g)], r[~np.isnan(r)])

    with np.errstate(invalid="ignore"):
        if kind == "moments":
            if not exact([3, 4, 5, 6, 7]):
                return np.inf
            scale = np.maximum(np.abs(ref[..., 0]), ref[..., 1])
            upd(np.abs(got[..., 0] - ref[..., 0]), tol * scale)
            upd(np.abs(got[..., 1] - ref[..., 1]), tol * scale)
            upd(np.abs(got[..., 2] - ref[..., 2]), 2 * tol * ref[..., 2])
        elif kind == "rows":
            if not exact([0, 1, 5, 6, 7]):
                return np.inf
            for k in (2, 3, 4):
                upd(np.abs(got[..., k] - ref[..., k]), tol * np.maximum(1.0, np.abs(ref[..., k])))
        elif kind == "cols":
            if not exact([0, 1, 2, 3, 4, 5]):
                return np.inf
            for k in (6, 7):
                upd(np.abs(got[..., k] - ref[..., k]), tol * np.maximum(1.0, np.abs(ref[..., k])))
        elif kind == "z32":
            r32 = ref.astype(np.float32)
            if got.dtype != np.float32 or not np.array_equal(np.isnan(got), np.isnan(r32)):
                return np.inf
            upd(np.abs(got.astype(np.float64) - r32.astype(np.float64)), np.spacing(np.abs(r32)).astype(np.float64))
        elif kind == "rel":
            upd(np.abs(got - ref), tol * np.abs(ref))
        elif kind == "factor":
            upd(np.abs(got - ref), tol * np.nanmax(np.abs(ref)) if np.any(~np.isnan(ref)) else 1.0)
        else:
            raise ValueError(kind)
    return worst if worst == worst else np.inf


def make_table(rng, rows, D, groups=(-1, 0, 1, 2), n_ref=None):
    """A synthetic ROI table (fp32) and its group words: columns of different scales and offsets (|mean| / sd <= 10).  n_ref:
    exactly that many rows of group 0 (None: as drawn)."""
    x = (rng.normal(size=(rows, D)) * rng.uniform(0.5, 3.0, D) + rng.uniform(-5.0, 5.0, D)).astype(np.float32)
    g = rng.choice(np.asarray(groups), size=rows).astype(np.int32)
    if n_ref is not None:
        g[g == 0] = 1
        g[rng.permutation(rows)[:n_ref]] = 0
    return x, g


def make_latent(rng, n_ref, n_other, Z, noise=0.05):
    """A latent table whose n_ref reference rows (group 0, scattered among n_other rows of groups 1 / 2 / -1) have a
    well-conditioned sample covariance: with n_ref > Z an orthonormal centred design (covariance close to the identity even at
    n_ref = Z + 1), with n_ref <= Z a centred design whose n_ref - 1 non-zero covariance eigenvalues are all 0.5 (so a ridge of
    1e-3 leaves a condition number near 500); a little noise on top.  (x fp32 [n_ref + n_other, Z], group)."""
    q = rng.normal(size=(n_ref, Z))
    q -= q.mean(0)
    if n_ref > Z:
        q = np.linalg.qr(q)[0] * np.sqrt(n_ref - 1)
        q = q + noise * rng.normal(size=(n_ref, Z))
    elif n_ref > 1:
        u, sv, vt = np.linalg.svd(q, full_matrices=False)
        sv = np.where(np.arange(len(sv)) < n_ref - 1, np.sqrt(0.5 * (n_ref - 1)), 0.0)
        q = (u * sv) @ vt
    ref = q + rng.uniform(-2.0, 2.0, Z)
    other = rng.normal(size=(n_other, Z)) * 1.5 + rng.uniform(-2.0, 2.0, Z)
    x = np.concatenate([ref, other]).astype(np.float32)
    g = np.concatenate([np.zeros(n_ref), rng.choice([1, 2, -1], size=n_other)]).astype(np.int32)
    p = rng.permutation(n_ref + n_other)
    return x[p], g[p]
