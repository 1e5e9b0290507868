"""The yardstick of nm_auc_bootstrap (tests/auc_bootstrap_ref.py) held to independent code: scikit-learn's roc_auc_score on
literal resamples, numpy's quantiles and moments, plain loops for the paired counts -- and the seeded faults the comparison with
the device must be able to catch.  No GPU."""
import math

import numpy as np
import pytest

from tests import auc_bootstrap_ref as R


def _set(n_pos, n_neg, seed, quantum=0.25, shift=0.6):
    """A set with ties: scores quantised to `quantum`, the positives shifted up, the classes interleaved."""
    rng = np.random.default_rng(seed)
    lab = np.zeros(n_pos + n_neg, dtype=np.int32)
    lab[rng.permutation(n_pos + n_neg)[:n_pos]] = 1
    s = rng.standard_normal(n_pos + n_neg) + shift * lab
    return (np.round(s / quantum) * quantum).astype(np.float32), lab


def test_auc_and_literal_resamples_against_sklearn():
    skm = pytest.importorskip("sklearn.metrics")
    for n_pos, n_neg, seed in ((5, 7, 1), (40, 23, 2), (1, 32, 3), (63, 1, 4), (300, 200, 5)):
        s, lab = _set(n_pos, n_neg, seed)
        p, q = R.split(s, lab)
        den = 2 * n_pos * n_neg
        assert abs(R.a2(p, q) / den - skm.roc_auc_score(lab, s.astype(np.float64))) <= 1e-12
        n_boot, sigma = 6, 3
        bt = R.boot(s, lab, n_boot, seed=77, stream=sigma)
        ip, iq = R.draws(n_pos, n_neg, np.arange(1, n_boot + 1), 77, sigma)
        rows_p, rows_q = np.flatnonzero(lab != 0), np.flatnonzero(lab == 0)
        for b in range(n_boot):
            rows = np.concatenate([rows_p[ip[b]], rows_q[iq[b]]])      # the resample as literal row indices
            assert len(rows) == n_pos + n_neg
            ref = skm.roc_auc_score(lab[rows], s[rows].astype(np.float64))
            assert abs(int(bt[b]) / den - ref) <= 1e-12, (n_pos, n_neg, b)


def test_special_values_tie_as_ieee_says():
    s = np.array([-0.0, 0.0, np.inf, np.inf, -np.inf, 1.0, 0.0], dtype=np.float32)
    lab = np.array([1, 0, 1, 0, 0, 1, 1])
    p, q = R.split(s, lab)
    # positives -0, inf, 1, 0 against negatives 0, inf, -inf: by hand
    by_hand = sum(2 * (a > b) + (a == b) for a in (0.0, np.inf, 1.0, 0.0) for b in (0.0, np.inf, -np.inf))
    assert R.a2(p, q) == by_hand
    assert R.split(np.array([1.0, np.nan], dtype=np.float32), [1, 0]) is None
    assert R.split(np.array([1.0, 2.0], dtype=np.float32), [1, 1]) is None
    assert R.split(np.zeros(0, dtype=np.float32), []) is None
    assert R.split(np.zeros(3, dtype=np.float32), [1, 0, 0], max_set=2) is None
    assert R.split(np.zeros(2, dtype=np.float32), [1, 0], stream=1 << 24) is None
    assert np.all(R.boot(np.array([1.0, np.nan], dtype=np.float32), [1, 0], 5) == -1)
    assert np.all(np.isnan(R.set_row(np.array([1.0, 2.0], dtype=np.float32), [0, 0], 5, 0, 4)))


def test_interval_moments_against_numpy():
    s, lab = _set(37, 51, 11)
    den = 2 * 37 * 51
    for n_boot, ci in ((300, 0.95), (130, 0.9), (2, 0.5), (1, 0.95), (64, 0.99)):
        lo, hi = R.boot_indices(n_boot, ci)
        assert 0 <= lo <= hi < n_boot and lo + hi == n_boot - 1
        row, bt = R.set_row(s, lab, n_boot, lo, hi, seed=5, stream=2, return_boot=True)
        auc = bt.astype(np.float64) / den
        assert row[1] == np.quantile(bt, (1 - ci) / 2, method="lower") / den
        assert row[2] == np.quantile(bt, (1 + ci) / 2, method="higher") / den      # (no position here is near an integer)
        assert row[2] == np.sort(bt)[hi] / den
        assert abs(row[3] - auc.mean()) <= 4 * n_boot * 2.0 ** -52 * abs(auc.mean())
        if n_boot > 1:
            assert abs(row[4] - auc.std(ddof=1)) <= 1e-9 * auc.std(ddof=1)
        else:
            assert math.isnan(row[4]) and lo == hi == 0
        assert tuple(row[5:]) == (n_boot, 37, 51)


def test_paired_counts_and_p_against_a_plain_loop():
    s, lab = _set(29, 35, 21)
    rng = np.random.default_rng(3)
    s2 = (s + np.round(rng.standard_normal(s.size)) * 0.25).astype(np.float32)
    n_boot = 200
    lo, hi = R.boot_indices(n_boot, 0.95)
    row = R.pair_row((s, lab, 4), (s2, lab, 4), n_boot, lo, hi, seed=9)
    ba, bc = R.boot(s, lab, n_boot, 9, 4), R.boot(s2, lab, n_boot, 9, 4)
    le = ge = 0
    for x, y in zip(ba.tolist(), bc.tolist()):
        le += x - y <= 0
        ge += x - y >= 0
    assert (row[6], row[7]) == (le, ge) and le + ge >= n_boot
    assert row[5] == min(1.0, 2 * (1 + min(le, ge)) / (1 + n_boot))
    den = 2 * 29 * 35
    assert row[0] == (R.a2(*R.split(s, lab)) - R.a2(*R.split(s2, lab))) / den
    d = np.sort(ba - bc)
    assert row[1] == d[lo] / den and row[2] == d[hi] / den
    assert abs(row[3] - (ba - bc).mean() / den) <= 1e-12 and abs(row[4] - (ba - bc).std(ddof=1) / den) <= 1e-12
    # a pair with itself; across streams; one label changed; an invalid set
    me = R.pair_row((s, lab, 4), (s, lab, 4), n_boot, lo, hi, seed=9)
    assert me[0] == 0 and me[5] == 1.0 and me[6] == me[7] == n_boot and me[3] == 0 and me[4] == 0
    assert np.all(np.isnan(R.pair_row((s, lab, 4), (s2, lab, 5), n_boot, lo, hi, seed=9)))
    lab2 = lab.copy()
    i, j = np.flatnonzero(lab == 1)[0], np.flatnonzero(lab == 0)[0]
    lab2[i], lab2[j] = 0, 1                                            # (the class sizes stay: only the rows differ)
    assert np.all(np.isnan(R.pair_row((s, lab, 4), (s2, lab2, 4), n_boot, lo, hi, seed=9)))
    nan = s2.copy()
    nan[3] = np.nan
    assert np.all(np.isnan(R.pair_row((s, lab, 4), (nan, lab, 4), n_boot, lo, hi, seed=9)))


def test_the_draw_stays_in_range_and_reaches_every_member():
    hi = R.splitmix64(np.arange(4096, dtype=np.uint64)) >> np.uint64(32)
    for m in (5, 7):
        idx = R.indices(hi, m)
        assert idx.min() == 0 and idx.max() == m - 1 and set(idx.tolist()) == set(range(m))
        assert R.indices([0, (1 << 32) - 1], m).tolist() == [0, m - 1]
    ip, iq = R.draws(5, 7, np.arange(1, 200), seed=1, sigma=0)
    assert ip.shape == (199, 5) and iq.shape == (199, 7)
    assert set(ip.ravel().tolist()) == set(range(5)) and set(iq.ravel().tolist()) == set(range(7))


def test_streams_differ_and_repeat():
    s, lab = _set(20, 30, 31)
    a, b, c = R.boot(s, lab, 50, 7, 0), R.boot(s, lab, 50, 7, 1), R.boot(s, lab, 50, 7, 0)
    assert np.array_equal(a, c) and not np.array_equal(a, b)
    assert not np.array_equal(a, R.boot(s, lab, 50, 8, 0))
    # the draws depend on the class sizes and the stream only: other scores, the same subjects
    ia, ib = R.draws(20, 30, [1, 2, 3], 7, 5), R.draws(20, 30, [1, 2, 3], 7, 5)
    assert np.array_equal(ia[0], ib[0]) and np.array_equal(ia[1], ib[1])


def _flagged(ref, got):
    """What the GPU tests do with the device's output: integers and bits must be the yardstick's."""
    return not (np.array_equal(ref[0], got[0], equal_nan=True) and np.array_equal(ref[1], got[1]))


@pytest.mark.parametrize("fault", R.FAULTS)
def test_seeded_faults_are_caught(fault):
    s, lab = _set(33, 31, 41)                                          # (ties: quantised scores)
    n_boot = 40
    lo, hi = R.boot_indices(n_boot, 0.95)
    good = R.set_row(s, lab, n_boot, lo, hi, seed=3, stream=6, return_boot=True)
    again = R.set_row(s, lab, n_boot, lo, hi, seed=3, stream=6, return_boot=True)
    bad = R.set_row(s, lab, n_boot, lo, hi, seed=3, stream=6, fault=fault, return_boot=True)
    assert not _flagged(good, again)
    assert _flagged(good, bad), fault
    assert not np.array_equal(good[1], bad[1]), fault                  # the distribution itself differs
    with_unknown = R.set_row(s, lab, n_boot, lo, hi, seed=3, stream=6, fault="none such", return_boot=True)
    assert not _flagged(good, with_unknown)
