"""The yardstick of the ROI-wise significance (tests/roi_significance_ref.py) against the libraries and against itself: U, p and
q against scipy, S against the pair counts of tests/roi_effect_ref.py, the label permutations' sizes and uniformity, and four
planted defects that must each change its output -- otherwise the device comparisons built on it would pin nothing."""
import numpy as np
import pytest
import scipy.stats

from tests import roi_effect_ref as E
from tests import roi_significance_ref as R

ROWS, D, SHIFTED = 171, 65, (3, 17, 31, 40, 64)


@pytest.fixture(scope="module")
def case():
    rng = np.random.default_rng(20240)
    g = rng.choice([1, 0, -1, 7], size=ROWS, p=[0.42, 0.38, 0.1, 0.1]).astype(np.int32)
    x = (np.round(rng.normal(size=(ROWS, D)) * 4) / 4) ** 2
    x[np.ix_(g == 1, SHIFTED)] += 1.0
    x = x.astype(np.float32)
    tab, P = R.table(x, g, n_perm=50, seed=11, k=2, return_parts=True)
    return x, g, tab, P


def test_u_and_p_against_scipy(case):
    x, g, tab, P = case
    X, Y = E.split(x, g)
    res = scipy.stats.mannwhitneyu(X, Y, alternative="two-sided", method="asymptotic", use_continuity=True, axis=0)
    assert P["valid"].all() and np.array_equal(tab[:, 0], res.statistic)
    rel = np.abs(tab[:, 3] - res.pvalue) / res.pvalue
    bound = R.p_bound(tab[:, 2])
    print("max |z|", np.abs(tab[:, 2]).max(), "max rel dp", rel.max(), "bound there", bound[np.argmax(rel)], "max ratio", (rel / bound).max())
    assert np.all(rel <= bound)
    assert np.abs(tab[list(SHIFTED), 2]).min() > 3.0 and np.all(tab[list(SHIFTED), 2] > 0)
    assert (P["tie"] > 0).all()                            # quantised inputs: ties in every column


def test_s_is_the_pair_count_difference(case):
    x, g, _, P = case
    more, less = E.counts_broadcast(*E.split(x, g))
    assert np.array_equal(P["S"], more - less)


def test_bh_is_scipys_bit_for_bit(case):
    tab = case[2]
    q = scipy.stats.false_discovery_control(tab[:, 3], method="bh")
    assert tab[:, 4].tobytes() == q.tobytes()
    p = np.array([0.04, 0.001, 0.04, 1.0, 0.5, 0.0])        # ties, the ends of the range
    assert R.bh(p).tobytes() == scipy.stats.false_discovery_control(p, method="bh").tobytes()


def test_every_permutation_has_n_x_ones(case):
    P = case[3]
    assert P["labels"].shape == (50, P["n"]) and np.all(P["labels"].sum(1) == P["n_x"])
    assert set(np.unique(P["labels"])) == {0, 1}
    assert len({row.tobytes() for row in P["labels"]}) == 50
    other = R.labels(P["n"], P["n_x"], 50, 11, k=3)          # the set index and the seed are part of the hash
    assert not np.array_equal(other, P["labels"]) and not np.array_equal(R.labels(P["n"], P["n_x"], 50, 12, k=2), P["labels"])


def test_positions_are_drawn_uniformly():
    n, n_x, T = 40, 13, 4000
    freq = R.labels(n, n_x, T, seed=5).sum(0)
    sd = np.sqrt(T * (n_x / n) * (1 - n_x / n))
    print("largest deviation in sd", np.abs(freq - T * n_x / n).max() / sd)
    assert np.all(np.abs(freq - T * n_x / n) <= 5 * sd)


def test_p_perm_of_a_separated_column():
    rng = np.random.default_rng(1)
    g = np.array([1] * 9 + [0] * 12)
    rng.shuffle(g)
    x = rng.normal(size=(21, 3))
    x[:, 1] = np.where(g == 1, 10.0 + x[:, 1], x[:, 1].clip(max=5.0))
    tab, P = R.table(x, g, n_perm=200, seed=3, return_parts=True)
    assert P["S"][1] == 9 * 12 and tab[1, 0] == 9 * 12
    assert tab[1, 5] == 1 / 201                              # no relabelling reaches the separated column's |S|
    assert tab[1, 6] == 1 / 201 and np.all(tab[:, 6] >= tab[:, 5]) and np.all(tab[:, 7] == 200)
    assert np.all(np.isnan(R.table(x, g)[:, 5:7])) and np.all(R.table(x, g)[:, 7] == 0)


@pytest.mark.parametrize("fault", ["rank_off_by_one", "tie_group_split", "label_flipped", "max_over_invalid"])
def test_a_planted_defect_changes_the_output(case, fault):
    x, g, _, _ = case
    x = x.copy()
    x[np.flatnonzero(g == 0)[0], 5] = np.nan                 # one column that is not valid
    good, P = R.table(x, g, n_perm=50, seed=11, k=2, return_parts=True)
    assert np.all(np.isnan(good[5])) and not P["valid"][5] and P["valid"].sum() == D - 1
    bad, Q = R.table(x, g, n_perm=50, seed=11, k=2, fault=fault, return_parts=True)
    # the output: the table and the null distribution of the maximum (maxstat_out)
    assert good.tobytes() + P["maxstat"].tobytes() != bad.tobytes() + Q["maxstat"].tobytes()
