"""The yardstick of the model-fit statistics (tests/fit_quality_ref.py) against code that shares nothing with it: scipy.stats'
pearsonr, spearmanr, skew and kurtosis, sklearn's r2_score and explained_variance_score, and an MSLL formed from
scipy.stats.norm.logpdf; the status rules at n = 2, 3, 4; the two-pass sums at an offset of 1e4; the yardstick's own
summation-order noise, which the 1e-9 of fit_quality_ref.close rests on; and seeded faults the comparison must flag.

Measured summation-order noise (the same 300 x 12 table with its rows permuted, 20 permutations, worst over the columns,
|a - b| / max(1, |a|); printed by test_permutation_noise_is_far_below_the_tolerance): rho 1.9e-15, smse 1.3e-15, expv 1.3e-15,
msll 3.6e-15, rmse 9.4e-16, bias 0, mae 0, mean_z 2.5e-16, sd_z 6.7e-16, skew_z 1.1e-15, kurt_z 9.3e-15, coverage 0; p_rho
9.7e-13 relative (p down to 1e-60: the noise of rho times the slope of log p).  All at or below 1e-12, so every column keeps
the bound 1e-9; the rank table is integer arithmetic and has none."""
import numpy as np
import pytest
from scipy import stats
from sklearn import metrics as skm

from tests import fit_quality_ref as R


def case(seed=0, rows=160, D=7, **kw):
    rng = np.random.default_rng(seed)
    x, loc, var, cv, g = R.make_case(rng, rows, D, **kw)
    train = (rng.normal(size=(240, D)) * 2.0 + rng.uniform(-5, 5, D)).astype(np.float32).astype(np.float64)
    triv = np.zeros((D, 8))
    triv[:, 0], triv[:, 2] = train.mean(0), train.var(0)
    triv[:, 1], triv[:, 3] = np.sqrt(triv[:, 2]), len(train)
    return x, loc, var, cv, g, triv


def test_against_scipy_and_sklearn():
    x, loc, var, cv, g, triv = case()
    fit, cal = R.quality(x, loc, g, var, cv, triv)
    ev = g == 0
    y, f = x[ev].astype(np.float64), loc[ev].astype(np.float64)
    s2 = var[ev].astype(np.float64) + cv.astype(np.float64)
    z = (y - f) / np.sqrt(s2)
    for d in range(x.shape[1]):
        r, p = stats.pearsonr(y[:, d], f[:, d])
        assert abs(fit[d, 0] - r) <= 1e-13 and abs(fit[d, 1] - p) <= 1e-9 * p
        assert abs(fit[d, 2] - (1.0 - skm.r2_score(y[:, d], f[:, d]))) <= 1e-13
        assert abs(fit[d, 3] - skm.explained_variance_score(y[:, d], f[:, d])) <= 1e-13
        msll = -stats.norm.logpdf(y[:, d], f[:, d], np.sqrt(s2[:, d])).mean() + \
            stats.norm.logpdf(y[:, d], triv[d, 0], np.sqrt(triv[d, 2])).mean()
        assert abs(fit[d, 4] - msll) <= 1e-12 * max(1.0, abs(msll))
        assert abs(fit[d, 5] - np.sqrt(skm.mean_squared_error(y[:, d], f[:, d]))) <= 1e-13
        assert abs(cal[d, 0] - (y[:, d] - f[:, d]).mean()) <= 1e-14 and abs(cal[d, 1] - skm.mean_absolute_error(y[:, d], f[:, d])) <= 1e-14
        assert abs(cal[d, 2] - z[:, d].mean()) <= 1e-14 and abs(cal[d, 3] - z[:, d].std()) <= 1e-13
        assert abs(cal[d, 4] - stats.skew(z[:, d], bias=True)) <= 1e-12
        assert abs(cal[d, 5] - stats.kurtosis(z[:, d], fisher=True, bias=True)) <= 1e-12
        assert cal[d, 6] == np.mean(np.abs(z[:, d]) <= 1.96)
    assert np.all(fit[:, 6] == ev.sum()) and np.all(cal[:, 7] == ev.sum()) and np.all(fit[:, 7] == 0)


@pytest.mark.parametrize("decimals", [None, 1, 0])
def test_spearman_in_integers_equals_scipy_with_ties(decimals):
    x, loc, _, _, g, _ = case(seed=3, rows=220, D=6)
    if decimals is not None:
        x, loc = np.round(x, decimals), np.round(loc, decimals)
    x[5, 0], x[9, 0] = 0.0, -0.0
    rk = R.rank(x, loc, g)
    ev = g == 0
    n = int(ev.sum())
    for d in range(x.shape[1]):
        ref = stats.spearmanr(x[ev, d], loc[ev, d])
        assert abs(rk[d, 0] - ref.statistic) <= 1e-15, (d, rk[d, 0], ref.statistic)
        assert abs(rk[d, 1] - ref.pvalue) <= 1e-9 * ref.pvalue
        ranks = stats.rankdata(x[ev, d])
        assert np.array_equal(R.k2(x[ev][:, d:d + 1])[:, 0], (2 * ranks - 1).astype(np.int64))
        assert R.k2(x[ev][:, d:d + 1]).sum() == n * n
        _, cnt = np.unique(x[ev, d], return_counts=True)
        assert rk[d, 4] == cnt[cnt > 1].sum()
    assert np.all(rk[:, 3] == n) and np.all(rk[:, 7] == 0) and np.all(rk[:, 6] == 0)
    if decimals is not None:
        assert rk[:, 4].min() > 0 and rk[:, 5].min() > 0


def test_small_n_and_status_rules():
    rng = np.random.default_rng(5)
    for n in (0, 1, 2, 3, 4):
        x, loc, var, cv, _ = R.make_case(rng, 6, 3)
        g = np.array([0] * n + [1] * (6 - n), dtype=np.int32)
        fit, cal = R.quality(x, loc, g, var, cv)
        rk = R.rank(x, loc, g)
        assert np.all(fit[:, 6] == n) and np.all(rk[:, 3] == n) and np.all(cal[:, 7] == n)
        if n < 2:
            assert np.all(fit[:, 7] == -2) and np.all(rk[:, 7] == -2)
            assert np.isnan(fit[:, :6]).all() and np.isnan(cal[:, :7]).all() and np.isnan(rk[:, [0, 1, 2, 4, 5]]).all()
        elif n == 2:
            assert np.all(fit[:, 7] == 1 + 4) and np.all(np.abs(fit[:, 0]) == 1.0) and np.isnan(fit[:, 1]).all()
            assert np.all(rk[:, 7] == 1) and np.all(np.abs(rk[:, 0]) == 1.0) and np.isnan(rk[:, 1:3]).all()
        else:
            assert np.all(fit[:, 7] == 4) and np.isfinite(fit[:, [0, 1, 2, 3, 5]]).all() and np.isnan(fit[:, 4]).all()
            assert np.all(rk[:, 7] == 0) and np.isfinite(rk[:, 0]).all() and not np.isnan(rk[:, 1:3]).any()
            ev = g == 0
            for d in range(3):
                ref = stats.pearsonr(x[ev, d].astype(np.float64), loc[ev, d].astype(np.float64))
                assert abs(fit[d, 1] - ref.pvalue) <= 1e-9 * ref.pvalue
    # the planted conditions, a column each
    x, loc, var, cv, g = R.make_case(rng, 40, 8, groups=(0, 0, 1))
    ev, out = np.nonzero(g == 0)[0], np.nonzero(g != 0)[0]
    triv = np.zeros((8, 8))
    triv[:, 2] = 1.0
    x[ev[3], 0] = np.nan                      # a NaN in an evaluated row
    x[out[1], 1] = np.inf                     # an inf in a left-out row
    loc[:, 2] = 0.25                          # a constant prediction
    var[ev[2], 3], cv[3] = 0.0, 0.0           # a zero s2
    var[ev[4], 4], cv[4] = -1.0, 0.5          # a negative s2
    triv[5, 7] = -2.0                         # an invalid trivial column
    x[:, 6] = 1.5                             # a constant observed column
    loc[ev[0], 7], loc[ev[1], 7] = np.float32(1e30), np.float32(-1e30)    # nothing special: finite
    fit, cal = R.quality(x, loc, g, var, cv, triv)
    assert list(fit[:, 7]) == [-2, 0, 1, 2, 2, 4, -2, 0]
    assert np.isnan(fit[0, :6]).all() and np.isnan(cal[0, :7]).all() and cal[0, 7] == len(ev)
    assert np.isnan(fit[2, :2]).all() and np.isfinite(fit[2, 2:6]).all()
    for d in (3, 4):
        assert np.isnan(fit[d, 4]) and np.isnan(cal[d, 2:7]).all() and np.isfinite(cal[d, :2]).all() and cal[d, 7] == len(ev) - 1
    assert np.isnan(fit[5, 4]) and np.isfinite(cal[5, :7]).all()
    rk = R.rank(x, loc, g)
    assert list(rk[:, 7]) == [-2, 0, 1, 0, 0, 0, 1, 0] and np.isnan(rk[2, :3]).all() and rk[2, 5] == len(ev)


def test_two_passes_hold_at_an_offset_where_the_raw_form_fails():
    rng = np.random.default_rng(11)
    sig = rng.normal(size=(400, 4))
    x = (1e4 + sig + 0.5 * rng.normal(size=(400, 4))).astype(np.float32)
    loc = (1e4 + sig).astype(np.float32)
    g = np.zeros(400, dtype=np.int32)
    fit, _ = R.quality(x, loc, g)
    y, f = x.astype(np.float64), loc.astype(np.float64)
    exact_expv = np.array([skm.explained_variance_score(y[:, d] - 1e4, f[:, d] - 1e4) for d in range(4)])
    exact_smse = np.array([1.0 - skm.r2_score(y[:, d] - 1e4, f[:, d] - 1e4) for d in range(4)])
    assert np.abs(fit[:, 3] - exact_expv).max() <= 1e-12 and np.abs(fit[:, 2] - exact_smse).max() <= 1e-12
    raw_smse, raw_expv = R.quality_raw(x, loc, g)
    assert max(np.abs(raw_smse - exact_smse).max(), np.abs(raw_expv - exact_expv).max()) > 1e-9     # the raw form fails ...
    fit_raw = fit.copy()
    fit_raw[:, 2], fit_raw[:, 3] = raw_smse, raw_expv
    assert R.close(fit_raw, fit, "fit") > 1.0                                                       # ... and the rule flags it


def test_permutation_noise_is_far_below_the_tolerance():
    x, loc, var, cv, g, triv = case(seed=21, rows=300, D=12, groups=(0,))
    fit0, cal0 = R.quality(x, loc, g, var, cv, triv)
    rk0 = R.rank(x, loc, g)
    rng = np.random.default_rng(1)
    noise = {}
    for _ in range(20):
        p = rng.permutation(len(g))
        fit, cal = R.quality(x[p], loc[p], g[p], var[p], cv, triv)
        assert np.array_equal(R.rank(x[p], loc[p], g[p]), rk0)         # integers: no noise at all
        for names, a, b in ((R.FIT[:6], fit0, fit), (R.CAL[:7], cal0, cal)):
            for k, name in enumerate(names):
                den = np.abs(a[:, k]) if name == "p_rho" else np.maximum(1.0, np.abs(a[:, k]))
                noise[name] = max(noise.get(name, 0.0), float((np.abs(a[:, k] - b[:, k]) / den).max()))
    print("summation-order noise:", ", ".join(f"{k} {v:.1e}" for k, v in noise.items()))
    for name, v in noise.items():
        assert v <= 1e-12, (name, v)                                   # the bound behind tol = 1e-9 of fit_quality_ref.close


def test_seeded_faults_are_flagged():
    x, loc, var, cv, g, triv = case(seed=8, rows=180, D=9)
    thr = 1.96
    fit, cal = R.quality(x, loc, g, var, cv, triv, thr=thr)
    rk = R.rank(np.round(x, 1), np.round(loc, 1), g)
    assert R.close(fit, fit, "fit") == 0 and R.close(cal, cal, "cal") == 0 and R.close(rk, rk, "rank") == 0
    # ddof 1 in place of 0
    assert R.close(R.quality(x, loc, g, var, cv, triv, ddof=1)[1], cal, "cal") > 1
    # MSLL with the sign of the trivial term flipped
    assert R.close(R.quality(x, loc, g, var, cv, triv, flip_trivial=True)[0], fit, "fit") > 1
    # See and SSE swapped
    assert R.close(R.quality(x, loc, g, var, cv, triv, swap_see=True)[0], fit, "fit") > 1
    # a dropped row
    g2 = g.copy()
    g2[np.nonzero(g == 0)[0][7]] = 1
    f2, c2 = R.quality(x, loc, g2, var, cv, triv)
    assert R.close(f2, fit, "fit") == np.inf and R.close(c2, cal, "cal") == np.inf
    assert R.close(R.rank(np.round(x, 1), np.round(loc, 1), g2), rk, "rank") == np.inf
    f2[:, 6], c2[:, 7] = fit[:, 6], cal[:, 7]                          # (even with the counts patched the values tell)
    assert R.close(f2, fit, "fit") > 1 and R.close(c2, cal, "cal") > 1
    # coverage with < on thr: a |z| exactly at thr
    ev = np.nonzero(g == 0)[0]
    x3, loc3 = x.copy(), loc.copy()
    var3, cv3 = np.full_like(var, 0.75), np.full_like(cv, 0.25)         # s2 = 1 exactly
    thr3 = 2.0
    x3[ev[0], :], loc3[ev[0], :] = np.float32(4.0), np.float32(2.0)     # e = 2, z = 2 = thr
    good = R.quality(x3, loc3, g, var3, cv3, triv, thr=thr3)[1]
    bad = R.quality(x3, loc3, g, var3, cv3, triv, thr=thr3, strict_cover=True)[1]
    assert R.close(bad, good, "cal") > 1
    # the k2 of one array from the other's sort
    assert R.close(R.rank(np.round(x, 1), np.round(loc, 1), g, cross=True), rk, "rank") == np.inf
    # one ulp in spearman is flagged (bit for bit), 1e-12 relative in rho is not
    r2 = rk.copy()
    r2[0, 0] = np.nextafter(r2[0, 0], 2.0)
    assert R.close(r2, rk, "rank") == np.inf
    f3 = fit.copy()
    f3[:, 0] *= 1 + 1e-12
    assert R.close(f3, fit, "fit") <= 1
