"""The yardstick of the normative z-map (tests/normative_ref.py) against code that shares nothing with it -- scipy.stats.zscore,
np.cov, np.linalg.cholesky, scipy.spatial.distance.mahalanobis with np.linalg.inv -- on the same inputs; the two-pass variance
against the raw form at an offset of 1e4; the yardstick's own summation-order noise (rows permuted), which the GPU bounds must
exceed 1000 times; and seeded faults that close() has to flag."""
import numpy as np
import pytest
import scipy.spatial.distance
import scipy.stats

from tests import normative_ref as R

GPU_TOL = 1e-9                                                     # the bound tests/test_gpu_normative.py holds the device to


def _case(seed=0, rows=300, D=37):
    rng = np.random.default_rng(seed)
    return R.make_table(rng, rows, D)


@pytest.mark.parametrize("ddof", [0, 1])
def test_moments_and_z_against_scipy(ddof):
    x, g = _case(1)
    mom = R.moments(x, g, ddof=ddof)
    ref = x[g == 0].astype(np.float64)
    assert np.all(mom[:, 7] == 0) and np.all(mom[:, 3] == len(ref)) and np.all(mom[:, 6] == 0)
    np.testing.assert_allclose(mom[:, 0], ref.mean(0), rtol=1e-13)
    np.testing.assert_allclose(mom[:, 1], ref.std(0, ddof=ddof), rtol=1e-13)
    np.testing.assert_allclose(mom[:, 2], ref.var(0, ddof=ddof), rtol=1e-13)
    assert np.array_equal(mom[:, 4], ref.min(0)) and np.array_equal(mom[:, 5], ref.max(0))
    z = R.z_table(x, mom)
    np.testing.assert_allclose(z[g == 0], scipy.stats.zscore(ref, axis=0, ddof=ddof), rtol=1e-11, atol=1e-13)
    # the signed variant: x - sub
    sub = np.random.default_rng(2).normal(size=x.shape).astype(np.float32)
    mom_s = R.moments(x, g, sub=sub, ddof=ddof)
    d = x.astype(np.float64) - sub.astype(np.float64)
    np.testing.assert_allclose(R.z_table(x, mom_s, sub=sub)[g == 0], scipy.stats.zscore(d[g == 0], axis=0, ddof=ddof),
                               rtol=1e-11, atol=1e-13)


def test_summaries_against_loops():
    x, g = _case(3, rows=90, D=23)
    x[5, 4] = np.nan
    x[g == 0, 7] = 2.5                                            # a column that is constant over the reference rows
    mom = R.moments(x, g)
    assert mom[7, 7] == -2 and np.isnan(mom[7, :3]).all() and mom[4, 7] == (-2 if g[5] == 0 else 0)
    z = R.z_table(x, mom)
    rows, cols = R.row_summary(z, 1.5), R.col_summary(z, g, mom, 1.5)
    for r in range(x.shape[0]):
        zz = [(c, z[r, c]) for c in range(x.shape[1]) if not np.isnan(z[r, c])]
        vals = np.array([v for _, v in zz])
        assert rows[r, 0] == (vals > 1.5).sum() and rows[r, 1] == (vals < -1.5).sum() and rows[r, 6] == len(vals)
        assert abs(rows[r, 2] - vals.mean()) < 1e-12 and abs(rows[r, 3] - np.abs(vals).mean()) < 1e-12
        assert rows[r, 4] == vals.max() and rows[r, 5] == zz[int(vals.argmax())][0] and rows[r, 7] == 0
    for c in range(x.shape[1]):
        if mom[c, 7] != 0:
            assert np.all(cols[c, :6] == 0) and np.isnan(cols[c, 6:]).all()
            continue
        for base, grp in ((0, 1), (1, 0)):
            vals = z[g == grp, c]
            vals = vals[~np.isnan(vals)]
            assert cols[c, 2 * base] == (vals > 1.5).sum() and cols[c, 2 * base + 1] == (vals < -1.5).sum()
            assert cols[c, 4 + base] == len(vals) and abs(cols[c, 6 + base] - vals.mean()) < 1e-12
    # the reference cohort's own mean z is zero by construction
    assert np.nanmax(np.abs(cols[:, 7])) < 1e-12


def test_status_rules():
    x, g = _case(4, rows=40, D=5)
    none = np.where(g == 0, 1, g)
    m = R.moments(x, none)
    assert np.all(m[:, 7] == -2) and np.all(m[:, 3] == 0) and np.isnan(m[:, [0, 1, 2, 4, 5]]).all()
    one = none.copy(); one[11] = 0
    assert np.all(R.moments(x, one, ddof=1)[:, 7] == -2)
    m0 = R.moments(x, one, ddof=0)                                 # one row, ddof 0: n_ref > ddof but min == max
    assert np.all(m0[:, 7] == -2) and np.all(m0[:, 3] == 1) and np.array_equal(m0[:, 4], x[11].astype(np.float64))
    z = R.z_table(x, m)
    assert np.isnan(z).all()
    rows = R.row_summary(z)
    assert np.all(rows[:, 7] == -2) and np.all(rows[:, 5] == -1) and np.all(rows[:, :2] == 0) and np.isnan(rows[:, 2:5]).all()
    xb = x.copy(); xb[np.flatnonzero(g == 0)[0], 2] = np.inf
    mb = R.moments(xb, g)
    assert mb[2, 7] == -2 and mb[2, 6] == 1 and np.isfinite(mb[2, 4:6]).all() and np.all(mb[[0, 1, 3, 4], 7] == 0)


def test_two_pass_variance_survives_an_offset_the_raw_form_loses():
    rng = np.random.default_rng(5)
    n = 1000
    base = rng.normal(size=(n, 1))
    x = (base + 1e4).astype(np.float32)
    g = np.zeros(n, dtype=np.int32)
    truth = (x.astype(np.float64) - 1e4).var(0, ddof=1)            # the offset taken off exactly
    two = R.moments(x, g)[:, 2]
    _, raw = R.moments_raw(x, g)
    e_two, e_raw = abs(two[0] - truth[0]) / truth[0], abs(raw[0] - truth[0]) / truth[0]
    print("relative variance error at offset 1e4: two-pass", e_two, "raw", e_raw)
    # (the raw form's error, 1e8 x 2^-52 ~ 2e-8, is outside the 2e-9 the device's variance is held to; the two-pass form's is not)
    assert e_two <= 1e-12 and e_raw > 5 * (2 * GPU_TOL)


def test_cov_chol_and_mahalanobis_against_numpy_and_scipy():
    rng = np.random.default_rng(6)
    for Z, n_ref in ((1, 5), (2, 9), (10, 40), (64, 65)):
        x, g = R.make_latent(rng, n_ref, 17, Z)
        mean, L, st = R.cov_chol(x, g, ridge=1e-3)
        assert st == 0
        ref = x[g == 0].astype(np.float64)
        C = np.atleast_2d(np.cov(ref, rowvar=False)) + 1e-3 * np.eye(Z)
        np.testing.assert_allclose(mean, ref.mean(0), rtol=1e-13, atol=1e-15)
        np.testing.assert_allclose(L, np.linalg.cholesky(C), rtol=1e-10, atol=1e-13)
        d2 = R.mahalanobis(x, mean, L, st)
        VI = np.linalg.inv(C)
        want = np.array([scipy.spatial.distance.mahalanobis(r, ref.mean(0), VI) ** 2 for r in x.astype(np.float64)])
        np.testing.assert_allclose(d2, want, rtol=1e-9)
    # the status rules
    x, g = R.make_latent(rng, 10, 5, 10)
    assert R.cov_chol(x, g)[2] == -2 and np.isnan(R.cov_chol(x, g)[1]).all()              # n_ref <= Z, ridge 0
    assert R.cov_chol(x, g, ridge=1e-3)[2] == 0
    assert R.cov_chol(x, np.where(g == 0, 1, g), ridge=1.0)[2] == -2                      # no reference row
    xb = x.copy(); xb[np.flatnonzero(g == 0)[3], 4] = np.nan
    assert R.cov_chol(xb, g, ridge=1.0)[2] == -2
    x2, g2 = R.make_latent(rng, 30, 5, 6)
    x2[:, 5] = x2[:, 4]                                                                   # two equal columns: a zero pivot
    assert R.cov_chol(x2, g2)[2] == -2
    xr = x.copy(); xr[2, 1] = np.inf
    mean, L, st = R.cov_chol(x, g, ridge=1e-3)
    d2 = R.mahalanobis(xr, mean, L, st)
    assert np.isnan(d2[2]) and np.isfinite(np.delete(d2, 2)).all()
    assert np.isnan(R.mahalanobis(x, mean, np.full_like(L, np.nan), -2)).all()


def _noise():
    """The yardstick against itself with the rows permuted: the largest error, in units of the GPU bounds' scales."""
    rng = np.random.default_rng(7)
    worst = {"moments": 0.0, "rows": 0.0, "cols": 0.0, "d2": 0.0}
    for trial in range(6):
        x, g = R.make_table(rng, 1064, 130)
        p = rng.permutation(len(g))
        m1, m2 = R.moments(x, g), R.moments(x[p], g[p])
        worst["moments"] = max(worst["moments"], R.close(m2, m1, "moments", tol=1.0))
        z1, z2 = R.z_table(x, m1), R.z_table(x[p], m2)
        worst["rows"] = max(worst["rows"], R.close(R.row_summary(z2), R.row_summary(z1)[p], "rows", tol=1.0))
        worst["cols"] = max(worst["cols"], R.close(R.col_summary(z2, g[p], m2), R.col_summary(z1, g, m1), "cols", tol=1.0))
        Z, n_ref = ((10, 40), (64, 65), (128, 512))[trial % 3]
        y, h = R.make_latent(rng, n_ref, 50, Z)
        q = rng.permutation(len(h))
        a = R.mahalanobis(y, *R.cov_chol(y, h))
        b = R.mahalanobis(y[q], *R.cov_chol(y[q], h[q]))
        worst["d2"] = max(worst["d2"], R.close(b, a[q], "rel", tol=1.0))
    return worst


def test_gpu_bounds_are_a_thousand_times_the_yardsticks_own_noise():
    worst = _noise()
    print("summation-order noise of the yardstick (rows permuted), relative to the bounds' scales:", worst)
    assert all(np.isfinite(v) for v in worst.values())
    for name, v in worst.items():
        assert GPU_TOL >= 1000 * v, (name, v)


def test_seeded_faults_are_flagged():
    rng = np.random.default_rng(8)
    x, g = R.make_table(rng, 400, 20)
    good = R.moments(x, g)
    assert R.close(good, good, "moments") == 0.0
    drop = np.flatnonzero(g == 0)[7]
    keep = np.arange(len(g)) != drop
    assert R.close(R.moments(x[keep], g[keep]), good, "moments") > 1.0                    # a dropped row (n_ref differs)
    wrong = g.copy(); wrong[np.flatnonzero(g == 1)[0]] = 0
    assert R.close(R.moments(x, wrong), good, "moments") > 1.0                            # a row of the wrong group counted
    off = R.moments(x, g, ddof=0)
    assert R.close(off, good, "moments") > 1e4                                            # ddof off by one: sd moves by 1 / 2n
    # the same faults with the counts patched to agree: the values alone give them away
    for bad in (R.moments(x[keep], g[keep]), R.moments(x, wrong)):
        bad = bad.copy(); bad[:, 3] = good[:, 3]; bad[:, 4:6] = good[:, 4:6]
        assert R.close(bad, good, "moments") > 1e4
    z = R.z_table(x, good)
    zo = R.z_table(x, off)
    assert R.close(R.row_summary(zo), R.row_summary(z), "rows") > 1e4
    assert R.close(zo.astype(np.float32), z, "z32") > 1.0 and R.close(z.astype(np.float32), z, "z32") == 0.0
    y, h = R.make_latent(rng, 60, 30, 10)
    mean, L, st = R.cov_chol(y, h)
    _, LT, _ = R.cov_chol(y, h, transposed=True)
    assert R.close(LT, L, "factor") > 1e4                                                 # a transposed factor
    assert R.close(R.mahalanobis(y, mean, LT, st), R.mahalanobis(y, mean, L, st), "rel") > 1e4
    dk = h.copy(); dk[np.flatnonzero(h == 0)[0]] = 1
    assert R.close(R.mahalanobis(y, *R.cov_chol(y, dk)), R.mahalanobis(y, mean, L, st), "rel") > 1e4
