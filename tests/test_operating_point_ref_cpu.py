"""tests/operating_point_ref.py held to the real thing: sklearn 1.7's roc_curve, precision_recall_curve, f1_score,
average_precision_score, roc_auc_score(max_fpr=) and np.interp, and the five threshold rules of
multimodal_kfold_cvae_group_analysis_1x1.py (:63-103, :129-132) written out with those functions.  Thresholds, counts and
status compare exactly; average_precision, pauc and the grid to 1e-11 absolute: ten times the K * 2^-53 bound of an 8192-term
sum of terms in [0, 1], a thousand times below the smallest effect of one misplaced subject, 1 / (n_pos * n) >= 1.5e-8.
No GPU."""
import math
import warnings

import numpy as np
import pytest

from tests import operating_point_ref as R

skm = pytest.importorskip("sklearn.metrics")

TOL = 1e-11
GRID = (0.0, 1.0, 100)


# ---- the reference's rules, on sklearn's own functions ------------------------------------------------------------------
def sk_roc(y, s):
    fpr, tpr, thr = skm.roc_curve(y, s)
    i = np.argmax(tpr - fpr)
    return thr[i], (tpr - fpr)[i]


def sk_grid_f1(y, s, grid=GRID):
    best = (0, 0)
    for v in np.linspace(*grid):
        f = skm.f1_score(y, (s >= v).astype(int))
        if f > best[1]:
            best = (v, f)
    return best


def sk_grid_cost(y, s, cost_fn, cost_fp, grid=GRID):
    best = (0, math.inf)
    for v in np.linspace(*grid):
        pred = (s >= v).astype(int)
        cost = np.sum((pred == 1) & (y == 0)) * cost_fp + np.sum((pred == 0) & (y == 1)) * cost_fn
        if cost < best[1]:
            best = (v, cost)
    return best


def sk_pr(y, s):
    p, r, thr = skm.precision_recall_curve(y, s)
    with np.errstate(invalid="ignore", divide="ignore"):
        f = 2 * (p * r) / (p + r)
    i = np.argmax(f)
    return thr[i], f[i]


def sk_eer(y, s):
    fpr, tpr, thr = skm.roc_curve(y, s)
    d = np.absolute((1 - tpr) - fpr)
    i = np.nanargmin(d)
    return thr[i], d[i]


def draw(seed, n, ties=0, shift=0.0, scale=1.0, p_pos=0.4):
    """n scores in fp32 (as fp64) and labels with both classes; ties > 0 rounds the scores to that many levels."""
    g = np.random.default_rng(seed)
    y = (g.random(n) < p_pos).astype(np.int64)
    y[0], y[1] = 1, 0
    s = g.random(n) * 0.6 + 0.25 * y * g.random(n)
    if ties:
        s = np.round(s * ties) / ties
    s = (s * scale + shift).astype(np.float32).astype(np.float64)
    return s, y


CASES = {
    "distinct_171": draw(1, 171),
    "distinct_1064": draw(2, 1064),
    "ties_9_levels": draw(3, 300, ties=9),
    "ties_2_levels": draw(4, 64, ties=2),
    "tiny_2": (np.array([0.75, 0.25]), np.array([1, 0])),
    "tiny_3": (np.array([0.5, 0.25, 0.5]), np.array([1, 0, 0])),
    "all_equal": (np.full(40, 0.5), np.r_[np.ones(15, dtype=np.int64), np.zeros(25, dtype=np.int64)]),
    "signed_zero": (np.array([0.0, -0.0, 0.5, -0.5, 0.0, -0.0, 0.25]), np.array([1, 0, 1, 0, 0, 1, 0])),
    "below_grid": draw(5, 120, shift=-3.0),
    "above_grid": draw(6, 120, shift=2.0),
    "wide": draw(7, 500, shift=-0.5, scale=3.0),
    "reversed": (lambda sy: ((1.0 - sy[0]).astype(np.float32).astype(np.float64), sy[1]))(draw(8, 200)),
}


def with_top_control(seed, n):
    s, y = draw(seed, n)
    s[np.argmax(s)] = np.float32(0.99)
    y[np.argmax(s)] = 0
    return s, y


CASES["top_is_control"] = with_top_control(9, 150)
CASES["top_is_patient"] = (lambda sy: (sy[0], np.where(np.arange(sy[0].size) == np.argmax(sy[0]), 1, sy[1])))(draw(10, 150))


@pytest.mark.parametrize("name", sorted(CASES))
def test_rules_match_sklearn(name):
    s, y = CASES[name]
    c = R.Curve(s, y)
    assert c.valid
    fps, tps, thr = skm._ranking._binary_clf_curve(y, s)
    assert np.array_equal(c.thr, thr) and np.array_equal(c.tps, tps) and np.array_equal(c.fps, fps)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        want = {"roc": sk_roc(y, s), "f1": sk_grid_f1(y, s), "cost": sk_grid_cost(y, s, 1, 1), "pr": sk_pr(y, s), "eer": sk_eer(y, s)}
        want_cost = sk_grid_cost(y, s, 2.5, 0.75)
        want_f1_grid = sk_grid_f1(y, s, (-1.0, 3.0, 7))
    for rule, (t, v) in want.items():
        got_t, got_v, status = R.select(c, rule)
        assert got_t == t, (rule, got_t, t)
        if rule == "pr" and np.isnan(v):
            assert status == 1.0 and np.isnan(got_v)
        else:
            assert status == 0.0 and got_v == v, (rule, got_v, v)
    assert R.select(c, "cost", cost_fn=2.5, cost_fp=0.75)[:2] == (want_cost[0], want_cost[1])
    assert R.select(c, "f1", grid=(-1.0, 3.0, 7))[:2] == (want_f1_grid[0], want_f1_grid[1])
    # the row the reference derives from a threshold (:144-153)
    for rule in R.RULES:
        t, v, status = R.select(c, rule)
        row = R.apply(t, v, status, s, y)
        pred = (s >= t).astype(int)
        tp, fn = np.sum((pred == 1) & (y == 1)), np.sum((pred == 0) & (y == 1))
        tn, fp = np.sum((pred == 0) & (y == 0)), np.sum((pred == 1) & (y == 0))
        assert row[1] == (pred == y).mean() and row[2] == tp / (tp + fn) and row[3] == tn / (tn + fp)
        assert row[4] == tp and row[5] == fp


@pytest.mark.parametrize("name", sorted(CASES))
def test_f1max_and_spec_are_what_they_say(name):
    s, y = CASES[name]
    c = R.Curve(s, y)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        f1 = np.array([skm.f1_score(y, (s >= t).astype(int)) for t in c.thr])
    t, v, status = R.select(c, "f1max")
    assert status == 0.0 and abs(v - f1.max()) <= 4 * np.finfo(float).eps
    assert t == c.thr[np.nonzero(np.abs(f1 - f1.max()) <= 4 * np.finfo(float).eps)[0]].min() or v == f1.max() == 0
    for a in (0.0, 0.5, 0.8, 0.9, 1.0):
        t, v, _ = R.select(c, "spec", spec=a)
        spec_of = lambda u: np.sum((s < u) & (y == 0)) / np.sum(y == 0)
        assert v == spec_of(t) and v >= a
        lower = c.thr[c.thr < t]
        assert lower.size == 0 or spec_of(lower.max()) < a                  # the next lower threshold no longer has it


def test_top_control_lands_on_the_nan():
    """The 'pr' rule of the reference: with a control on top, the highest threshold has tp = 0, precision_recall_curve gives
    (precision 0, recall 0) there, 2 * 0 / 0 is NaN and np.argmax returns that index -- not the best F1."""
    s, y = CASES["top_is_control"]
    p, r, thr = skm.precision_recall_curve(y, s)
    with np.errstate(invalid="ignore"):
        f = 2 * (p * r) / (p + r)
    i = int(np.argmax(f))
    assert np.isnan(f[i]) and i == int(np.nonzero(np.isnan(f))[0][0])
    assert thr[i] == np.float64(np.float32(0.99))
    c = R.Curve(s, y)
    t, v, status = R.select(c, "pr")
    assert (t, status) == (thr[i], 1.0) and np.isnan(v)
    t2, v2, status2 = R.select(c, "f1max")
    assert status2 == 0.0 and t2 < t and v2 == np.nanmax(f)
    # a patient on top: no NaN, both rules agree
    s, y = CASES["top_is_patient"]
    c = R.Curve(s, y)
    assert R.select(c, "pr") == R.select(c, "f1max") and R.select(c, "pr")[2] == 0.0


@pytest.mark.parametrize("name", sorted(CASES))
def test_summary_and_grid_match_sklearn(name):
    s, y = CASES[name]
    c = R.Curve(s, y)
    for max_fpr in (0.1, 0.25, 1.0):
        row = R.summary(c, spec=0.9, sens=0.8, max_fpr=max_fpr)
        assert abs(row[0] - skm.roc_auc_score(y, s)) <= TOL
        assert abs(row[1] - skm.average_precision_score(y, s)) <= TOL
        assert abs(row[2] - skm.roc_auc_score(y, s, max_fpr=max_fpr)) <= TOL
        fpr, tpr, _ = skm.roc_curve(y, s, drop_intermediate=False)
        fps, tps, _ = skm._ranking._binary_clf_curve(y, s)
        fps, tps = np.r_[0, fps], np.r_[0, tps]                             # (the origin: nothing predicted positive)
        assert row[3] == (tps / c.P)[c.N - fps >= math.ceil(0.9 * c.N)].max()
        assert row[4] == ((c.N - fps) / c.N)[tps >= math.ceil(0.8 * c.P)].max()
        assert (row[5], row[6], row[7]) == (len(fpr) - 1, y.sum(), (1 - y).sum())
    for G in (2, 50, 101, 1024):
        got = R.roc_on_grid(c, G)
        want = np.interp(np.linspace(0, 1, G), fpr, tpr)
        assert np.abs(got - want).max() <= TOL
        assert got[0] == tpr[fpr == 0].max() and got[-1] == 1.0             # a vertical segment: its upper end


def test_sets_without_a_curve():
    for s, y in ((np.array([]), np.array([])), (np.array([0.5, 0.25]), np.array([1, 1])), (np.array([0.5, 0.25]), np.array([0, 0])),
                 (np.array([0.5, np.nan, 0.1]), np.array([1, 0, 1]))):
        c = R.Curve(s, y)
        assert not c.valid
        for rule in R.RULES:
            assert R.select(c, rule)[2] == -2.0
        row = R.summary(c)
        assert np.isnan(row[:6]).all() and (s.size == 0 or (row[6], row[7]) == (y.sum(), (1 - y).sum()))
        assert np.isnan(R.roc_on_grid(c, 5)).all()
    # a valid threshold on an empty evaluation set, and on sets of one class
    assert R.apply(0.5, 0.0, 0.0, np.array([]), np.array([]))[7] == -2.0
    row = R.apply(0.5, 0.0, 0.0, np.array([0.75, 0.25]), np.array([0, 0]))
    assert np.isnan(row[2]) and row[3] == 0.5 and row[1] == 0.5
    row = R.apply(0.5, 0.0, 0.0, np.array([0.75, 0.25]), np.array([1, 1]))
    assert np.isnan(row[3]) and row[2] == 0.5


def test_fold_mapping():
    a, b = CASES["distinct_171"], CASES["ties_9_levels"]
    pts, summ, grid = R.operating_points([a[0], b[0]], [a[1], b[1]], rules=R.RULES, select_of=[1, 0, 0], evaluate=[0, 1, 0], roc_grid=11)
    assert pts.shape == (3, 7, 8) and summ.shape == (2, 8) and grid.shape == (2, 11)
    ca, cb = R.Curve(*a), R.Curve(*b)
    for k, rule in enumerate(R.RULES):
        assert pts[0, k, 0] == R.select(cb, rule)[0] and pts[1, k, 0] == R.select(ca, rule)[0] and pts[2, k, 0] == R.select(ca, rule)[0]
        assert np.array_equal(pts[2, k], R.apply(*R.select(ca, rule), *a), equal_nan=True)
