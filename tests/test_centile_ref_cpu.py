"""The centile yardstick (tests/centile_ref.py) against numpy and scipy, with == (no tolerance: every quantity is defined
operation by operation): quantiles against np.quantile(method="linear"), the median against np.median, the MAD against
scipy.stats.median_abs_deviation, pct against scipy.stats.percentileofscore(kind="mean"); leave-one-out against dropping the
row and recomputing; robust_moments against its definition.  No GPU."""
import numpy as np
import pytest
import torch
from scipy import stats as sps

from multi_modal_normative_modeling_amd import metrics
from tests import centile_ref as R

SIZES = (1, 2, 3, 255, 256, 257, 512, 513)
PROBS = (0.0, 1.0, 1.0 / 3.0, 0.025, 0.5, 0.975)


def columns(n, seed):
    """The reference columns of one size: fp32 draws, the same rounded to one decimal (ties), shifted by -1e4, and with
    -0.0 next to +0.0."""
    rng = np.random.default_rng(seed)
    base = rng.normal(size=n).astype(np.float32)
    tied = np.round(rng.normal(size=n), 1).astype(np.float32)
    zeros = tied.copy()
    zeros[::3] = -0.0
    zeros[1::3] = 0.0
    return {"plain": base, "ties": tied, "offset": (tied - np.float32(1e4)).astype(np.float32), "zeros": zeros,
            "chi2": (base * base).astype(np.float32)}


@pytest.mark.parametrize("n", SIZES)
def test_quantiles_median_and_mad_equal_numpy_and_scipy(n):
    for name, col in columns(n, 100 + n).items():
        v = col.astype(np.float64)
        a = R.sorted_ref(v)
        for p in PROBS:
            assert R.quantile(a, p) == np.quantile(v, p, method="linear"), (name, n, p)
        med = R.median(a)
        assert med == np.median(v), (name, n)
        assert R.mad(a, med) == sps.median_abs_deviation(v, scale=1.0), (name, n)
        q, st = R.cohort_quantiles(col[:, None], np.zeros(n, dtype=np.int32), PROBS)
        assert np.array_equal(q[0], np.quantile(v, PROBS, method="linear"))
        assert st[0, 0] == np.median(v) and st[0, 1] == sps.median_abs_deviation(v, scale=1.0)
        assert st[0, 2] == np.quantile(v, 0.25) and st[0, 3] == np.quantile(v, 0.75) and st[0, 4] == st[0, 3] - st[0, 2]
        assert st[0, 5] == n and st[0, 6] == 0 and st[0, 7] == 0


@pytest.mark.parametrize("n", SIZES)
def test_pct_equals_percentileofscore(n):
    rng = np.random.default_rng(7 * n)
    for name, col in columns(n, 200 + n).items():
        scored = np.concatenate([col[: min(n, 40)], np.round(rng.normal(size=25), 1).astype(np.float32) + col[0],
                                 np.array([-0.0, 0.0, 1e30, -1e30], dtype=np.float32)])
        x = np.concatenate([col, scored])[:, None]
        g = np.concatenate([np.zeros(n, dtype=np.int32), np.ones(len(scored), dtype=np.int32)])
        k2, n_ref = R.k2_table(x, g, x, g)
        assert n_ref == n and k2.min() >= 0 and k2.max() <= 2 * n
        pct = R.pct_table(k2, R.divisors(g, n_ref, False))[:, 0]
        want = np.array([sps.percentileofscore(col.astype(np.float64), float(v), kind="mean") for v in x[:, 0]])
        assert np.array_equal(pct, want), (name, n)


def test_invalid_marks():
    x = np.array([[1.0, 2.0, 3.0], [2.0, np.nan, 1.0], [3.0, 1.0, np.inf], [np.nan, 0.0, -np.inf], [0.5, 0.5, 0.5]], dtype=np.float32)
    g = np.array([0, 0, 1, 1, 2], dtype=np.int32)
    k2, n = R.k2_table(x, g, x, g)
    assert n == 2
    assert np.all(k2[:, 1] == R.INVALID)                               # a NaN in a reference row: the column
    assert k2[3, 0] == R.INVALID and k2[2, 2] == R.INVALID and k2[3, 2] == R.INVALID     # a patient's NaN / inf: the element
    assert k2[2, 0] == 4 and k2[0, 0] == 1 and k2[4, 0] == 0 and k2[0, 2] == 3
    q, st = R.cohort_quantiles(x, g, (0.5,))
    assert np.isnan(q[1, 0]) and st[1, 7] == -2 and st[1, 5] == 2 and st[1, 6] == 1 and st[0, 7] == 0
    k2, n = R.k2_table(x, np.full(5, 1), x, np.full(5, 1))             # no reference row
    assert n == 0 and np.all(k2 == R.INVALID)
    rows = R.row_summary(k2, R.divisors(np.full(5, 1), 0, False), 2.5)
    assert np.all(rows[:, 7] == -2) and np.all(rows[:, 5] == -1) and np.isnan(rows[:, 2:5]).all() and np.all(rows[:, [0, 1, 6]] == 0)


@pytest.mark.parametrize("n", (1, 2, 3, 64, 257))
def test_leave_one_out_equals_dropping_the_row(n):
    rng = np.random.default_rng(31 * n)
    x = np.round(rng.normal(size=(n + 9, 4)), 1).astype(np.float32)
    g = np.concatenate([np.zeros(n, dtype=np.int32), np.ones(9, dtype=np.int32)])
    perm = rng.permutation(n + 9)
    x, g = x[perm], g[perm]
    k2, n_ref = R.k2_table(x, g, x, g, self_loo=True)
    nd = R.divisors(g, n_ref, True)
    pct = R.pct_table(k2, nd)
    plain = R.pct_table(*[(k, R.divisors(g, m, False)) for k, m in [R.k2_table(x, g, x, g)]][0])
    for r in range(n + 9):
        if g[r] != 0:
            assert np.array_equal(pct[r], plain[r])                    # a patient: the whole reference
            continue
        keep = np.arange(n + 9) != r
        if n == 1:
            assert np.isnan(pct[r]).all() and np.all(k2[r] == R.INVALID)
            continue
        k2r, m = R.k2_table(x[r:r + 1], g[r:r + 1] + 5, x[keep], g[keep])
        assert m == n - 1 and nd[r] == n - 1
        assert np.array_equal(pct[r], R.pct_table(k2r, np.array([m]))[0]), r
        for c in range(4):
            assert pct[r, c] == sps.percentileofscore(x[keep & (g == 0), c].astype(np.float64), float(x[r, c]), kind="mean")


def test_row_and_column_summaries_against_plain_numpy():
    rng = np.random.default_rng(5)
    x = np.round(rng.normal(size=(90, 7)), 1).astype(np.float32)
    g = rng.choice([0, 1, 2], size=90, p=[0.5, 0.4, 0.1]).astype(np.int32)
    x[np.flatnonzero(g == 1)[0], 3] = np.nan
    for loo in (False, True):
        pct32, rows, cols = R.normative_centile([(x, g, None)], tail=5.0, loo=loo)[0]
        k2, n = R.k2_table(x, g, x, g, self_loo=loo)
        pct = R.pct_table(k2, R.divisors(g, n, loo))
        assert np.array_equal(pct32, pct.astype(np.float32), equal_nan=True)
        for r in range(90):
            ok = ~np.isnan(pct[r])
            assert rows[r, 0] == np.sum(pct[r, ok] > 95.0) and rows[r, 1] == np.sum(pct[r, ok] < 5.0) and rows[r, 6] == ok.sum()
            assert rows[r, 4] == pct[r, ok].max() and rows[r, 5] == np.flatnonzero(ok & (pct[r] == pct[r, ok].max()))[0]
            assert abs(rows[r, 2] - pct[r, ok].mean()) < 1e-12 * 100 and abs(rows[r, 3] - np.abs(pct[r, ok] - 50.0).mean()) < 1e-12 * 100
        for c in range(7):
            for which, base in ((1, 0), (0, 2)):
                m = (g == which) & ~np.isnan(pct[:, c])
                assert cols[c, base] == np.sum(pct[m, c] > 95.0) and cols[c, base + 1] == np.sum(pct[m, c] < 5.0)
                assert cols[c, 4 + (which == 0)] == m.sum() and abs(cols[c, 6 + (which == 0)] - pct[m, c].mean()) < 1e-10


def test_robust_moments_against_its_definition():
    rng = np.random.default_rng(3)
    x = np.round(rng.normal(size=(40, 5)), 1).astype(np.float32)
    x[:, 2] = 1.5                                                       # a constant column: mad == 0
    x[3, 4] = np.nan                                                    # an invalid column
    _, st = R.cohort_quantiles(x, np.zeros(40, dtype=np.int32), ())
    for scale in (1.4826, 1.0):
        got = metrics.robust_moments(torch.from_numpy(st[None]), scale=scale).numpy()[0]
        assert np.array_equal(got, R.robust_moments(st, scale), equal_nan=True)
        for c in range(5):
            bad = st[c, 7] == -2 or st[c, 1] == 0
            assert got[c, 7] == (-2 if bad else 0) and got[c, 3] == st[c, 5] and got[c, 6] == st[c, 6]
            assert np.isnan(got[c, 4]) and np.isnan(got[c, 5])
            if c != 4:
                assert got[c, 0] == st[c, 0] and got[c, 1] == scale * st[c, 1] and got[c, 2] == got[c, 1] * got[c, 1]
        assert got[2, 7] == -2 and got[4, 7] == -2 and np.isnan(got[4, 0]) and got[0, 7] == 0
    for bad in (dict(scale=0.0), dict(scale=float("nan")), dict(stats=torch.zeros(1, 5, 8)), dict(stats=torch.zeros(5, 8, dtype=torch.float64))):
        with pytest.raises(ValueError):
            metrics.robust_moments(**{**dict(stats=torch.from_numpy(st[None])), **bad})
