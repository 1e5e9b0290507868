"""The yardstick of the ROI-wise effect sizes (tests/roi_effect_ref.py) against itself and against the libraries: its two ways
of counting agree, its AUC is sklearn's, its counts are Mann-Whitney's U, delta and AUC are one quantity, and the formula gives
the bits of the pair-by-pair loop.  No GPU."""
import numpy as np
import pytest

from tests import roi_effect_ref as R


def _table(seed, rows, D, nan=True):
    """Squares of values quantised to 1/4 (ties are common), a few NaN / inf entries, groups 1 / 0 / left out."""
    rng = np.random.default_rng(seed)
    x = (np.round(rng.normal(size=(rows, D)) * 4) / 4) ** 2
    group = rng.choice([1, 0, -1, 7], size=rows, p=[0.4, 0.4, 0.1, 0.1])
    if nan:
        x[rng.integers(0, rows, 5), rng.integers(0, D, 5)] = np.nan
        x[rng.integers(0, rows, 2), rng.integers(0, D, 2)] = np.inf
        x[rng.integers(0, rows, 2), rng.integers(0, D, 2)] = -np.inf
    return x.astype(np.float32), group


@pytest.mark.parametrize("seed,rows,D", [(0, 2, 1), (1, 37, 5), (2, 150, 9), (3, 301, 3)])
def test_two_forms_agree_on_counts(seed, rows, D):
    x, group = _table(seed, rows, D)
    if seed == 0:
        group = np.array([1, 0])
    X, Y = R.split(x, group)
    mb, lb = R.counts_broadcast(X, Y)
    ms, ls = R.counts_sorted(X, Y)
    assert mb.dtype == ms.dtype == np.int64
    assert np.array_equal(mb, ms) and np.array_equal(lb, ls)
    a, b = R.table(x, group, R.counts_broadcast), R.table(x, group, R.counts_sorted)
    assert np.array_equal(a, b, equal_nan=True)
    assert np.array_equal(a[:, 4], np.full(D, len(X))) and np.array_equal(a[:, 5], np.full(D, len(Y)))


def test_signed_zeros_tie_and_empty_groups():
    x = np.array([[0.0], [-0.0], [-0.0], [0.0]], dtype=np.float32)
    t = R.table(x, [1, 1, 0, 0])
    assert t[0, 2] == 0 and t[0, 3] == 0 and t[0, 0] == 0.0 and t[0, 1] == 0.5
    for group in ([1, 1, 7, -1], [0, 0, 2, 0], [3, 3, 3, 3]):
        t = R.table(x, group)
        assert t[0, 2] == 0 and t[0, 3] == 0 and np.isnan(t[0, 0]) and np.isnan(t[0, 1])
        assert np.isnan(t[0, 6]) == (1 not in group) and np.isnan(t[0, 7]) == (0 not in group)


def test_auc_is_sklearns():
    from sklearn.metrics import roc_auc_score
    x, group = _table(11, 260, 12, nan=False)
    t = R.table(x, group)
    keep = (group == 0) | (group == 1)
    for c in range(x.shape[1]):
        want = roc_auc_score(group[keep], x[keep, c].astype(np.float64))
        assert abs(t[c, 1] - want) <= 1e-12, (c, t[c, 1], want)


def test_counts_are_mann_whitneys_u():
    from scipy.stats import mannwhitneyu
    x, group = _table(12, 180, 7, nan=False)
    X, Y = R.split(x, group)
    t = R.table(x, group)
    for c in range(x.shape[1]):
        ties = t[c, 4] * t[c, 5] - t[c, 2] - t[c, 3]
        assert t[c, 2] + ties / 2 == mannwhitneyu(X[:, c], Y[:, c]).statistic, c


def test_delta_is_twice_auc_minus_one():
    for seed in range(4):
        x, group = _table(20 + seed, 333, 11)
        t = R.table(x, group)
        assert np.all(np.abs(t[:, 0] - (2 * t[:, 1] - 1)) <= 1e-15)


def test_formula_gives_the_bits_of_the_double_loop():
    rng = np.random.default_rng(5)
    X = ((np.round(rng.normal(size=97) * 4) / 4) ** 2).astype(np.float32)
    Y = ((np.round(rng.normal(size=131) * 4) / 4) ** 2).astype(np.float32)
    X[13] = np.nan
    assert len(set(X[~np.isnan(X)]) & set(Y)) > 3                       # ties are there
    x = np.concatenate([X, Y])[:, None]
    group = np.concatenate([np.ones(97, dtype=int), np.zeros(131, dtype=int)])
    for counts in (R.counts_broadcast, R.counts_sorted):
        got = R.table(x, group, counts)[0, 0]
        want = R.literal_delta(X, Y)
        assert np.float64(got).tobytes() == np.float64(want).tobytes(), (got, want)
