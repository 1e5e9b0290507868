"""The numpy restatement of the chart pass (tests/chart_ref.py) against exact rational arithmetic, within the bound the file
derives from its operation counts; its status rules; and seeded faults in the merge, which must be flagged.  No GPU."""
from fractions import Fraction

import numpy as np
import pytest

from tests import chart_ref as R

ROWS = (2, 16, 127, 128, 129, 257, 4096)
D = 3


def _data(n, offset, seed=0):
    rng = np.random.default_rng(1000 * seed + n)
    return (rng.standard_normal((n, D)) + offset).astype(np.float32)


def _exact(x):
    """Column means and unbiased variances of the fp32 values in exact rational arithmetic."""
    n = x.shape[0]
    means, varis = [], []
    for d in range(x.shape[1]):
        col = [Fraction(float(v)) for v in x[:, d]]
        mean = sum(col, Fraction(0)) / n
        means.append(mean)
        varis.append(sum(((v - mean) ** 2 for v in col), Fraction(0)) / (n - 1))
    return means, varis


def _shares(x):
    """|restatement - exact| / bound per column, for mean and var_latent."""
    got = R.chart(x)
    b_mean, b_var = R.bound(x)
    means, varis = _exact(x)
    s_mean = [abs(Fraction(float(got[d, 0])) - means[d]) / Fraction(float(b_mean[d])) for d in range(x.shape[1])]
    s_var = [abs(Fraction(float(got[d, 1])) - varis[d]) / Fraction(float(b_var[d])) for d in range(x.shape[1])]
    return float(max(s_mean)), float(max(s_var))


@pytest.mark.parametrize("offset", (0.0, 1e4))
@pytest.mark.parametrize("n", ROWS)
def test_restatement_meets_its_bound_against_exact_arithmetic(n, offset):
    x = _data(n, offset)
    got = R.chart(x)
    assert np.all(got[:, 2] == n) and np.all(got[:, 3] == 0)
    s_mean, s_var = _shares(x)
    print(f"n={n} offset={offset:g}: share of the bound  mean {s_mean:.3f}  var_latent {s_var:.3f}")
    assert s_mean <= 1.0 and s_var <= 1.0
    # the bound is a statement about rounding, not a loose tolerance: it stays far below the statistic's own scale
    b_mean, b_var = R.bound(x)
    assert np.all(b_mean <= 1e-10 * (np.abs(got[:, 0]) + 1.0)) and np.all(b_var <= 1e-6 * got[:, 1])


def test_partials_have_the_request_layout_and_the_tile_counts():
    x = _data(257, 0.0)
    p = R.partials(x)
    assert p.shape == (3, D, 2) and [R.tile_rows(257, t) for t in range(3)] == [128, 128, 1]
    np.testing.assert_array_equal(p[2, :, 0], x[256].astype(np.float64))      # a one-row tile: its value, M2 = 0
    np.testing.assert_array_equal(p[2, :, 1], 0.0)
    np.testing.assert_allclose(p[0, :, 0], x[:128].astype(np.float64).mean(axis=0), rtol=1e-14)


def test_one_row_gives_status_minus_two_and_nan():
    got = R.chart(_data(2, 0.0)[:1])
    assert np.all(got[:, 3] == -2) and np.all(got[:, 2] == 1) and np.isnan(got[:, :2]).all()


@pytest.mark.parametrize("bad", (np.nan, np.inf, -np.inf))
def test_a_non_finite_value_gives_status_minus_two_in_its_column_only(bad):
    x = _data(257, 0.0)
    x[200, 1] = bad
    got = R.chart(x)
    assert got[1, 3] == -2 and np.isnan(got[1, :2]).all() and got[1, 2] == 257
    assert np.all(got[[0, 2], 3] == 0) and np.isfinite(got[[0, 2], :2]).all()


@pytest.mark.parametrize("offset", (0.0, 1e4))
def test_seeded_faults_in_the_merge_are_flagged(offset):
    """A dropped tile, a tile merged twice and a wrong count on the ragged last tile each leave the bound by orders of
    magnitude: the bound is tight enough to see them."""
    n = 300                                                           # tiles of 128, 128, 44 rows
    x = _data(n, offset)
    part = R.partials(x)
    b_mean, b_var = R.bound(x)
    means, varis = _exact(x)
    want_mean, want_var = np.array([float(m) for m in means]), np.array([float(v) for v in varis])

    def off(chart):
        return np.abs(chart[:, 0] - want_mean) / b_mean, np.abs(chart[:, 1] - want_var) / b_var

    ok_mean, ok_var = off(R.merge(part, n))
    assert ok_mean.max() <= 1.5 and ok_var.max() <= 1.5               # (the exact values rounded to fp64 once more)
    faults = {
        "dropped tile": R.merge(part[[0, 2]], n, counts=[128, 44]),
        "tile merged twice": R.merge(part[[0, 1, 1, 2]], n, counts=[128, 128, 128, 44]),
        "wrong count on the ragged tile": R.merge(part, n, counts=[128, 128, 128]),
    }
    for name, chart in faults.items():
        f_mean, f_var = off(chart)
        assert max(f_mean.max(), f_var.max()) > 1e3, name
