"""nm_operating_points against tests/operating_point_ref.py (which tests/test_operating_point_ref_cpu.py holds to sklearn):
thresholds, tp, fp, status, the fp64 ratios and objectives, n_thresholds / n_pos / n_neg and roc_auc bit for bit (the
restatement forms them with the same expressions); average_precision, pauc and the ROC grid to 1e-11 absolute (ten times
the K * 2^-53 bound of an 8192-term sum of terms in [0, 1]).  Sizes on both sides of the workgroup width, of a sort that
pads and of the LDS limit; tie structures, signed zeros, infinities, grids that miss the scores; sets without a curve among
valid ones; the launch shape; the fold mapping."""
import math

import numpy as np
import pytest
import torch

from multi_modal_normative_modeling_amd import _lib, metrics
from tests import operating_point_ref as R
from tests.table_stats_util import same_bits

pytestmark = pytest.mark.gpu

TOL = 1e-11
EXACT_SUMMARY = [0, 3, 4, 5, 6, 7]
KW = dict(grid=(0.0, 1.0, 100), cost_fn=2.5, cost_fp=0.75, spec=0.9, sens=0.8, max_fpr=0.1)


def draw(seed, n, ties=0, shift=0.0, scale=1.0):
    g = np.random.default_rng(seed)
    y = (g.random(n) < 0.4).astype(np.int32)
    s = g.random(n) * 0.6 + 0.25 * y * g.random(n)
    if ties:
        s = np.round(s * ties) / ties
    if n >= 2:
        y[0], y[1] = 1, 0
    return (s * scale + shift).astype(np.float32), y


def device_points(sets, rules=R.RULES, roc_grid=0, **kw):
    args = dict(KW)
    args.update(kw)
    out = metrics.operating_points([torch.from_numpy(s) for s, _ in sets], [torch.from_numpy(l) for _, l in sets], rules=rules,
                                   roc_grid=roc_grid, **args)
    return tuple(o.cpu().numpy() for o in out)


def host_points(sets, rules=R.RULES, roc_grid=0, **kw):
    args = dict(KW)
    args.update(kw)
    return R.operating_points([s for s, _ in sets], [l for _, l in sets], rules=rules, roc_grid=roc_grid, **args)


def held(got, want, what):
    assert got[0].shape == want[0].shape and got[1].shape == want[1].shape, what
    for k in range(got[0].shape[1]):
        assert same_bits(got[0][:, k], want[0][:, k]), (what, "rule", k, got[0][:, k], want[0][:, k])
    assert same_bits(got[1][:, EXACT_SUMMARY], want[1][:, EXACT_SUMMARY]), (what, got[1], want[1])
    for j in (1, 2):
        assert np.array_equal(np.isnan(got[1][:, j]), np.isnan(want[1][:, j])), (what, j)
        assert np.all(np.nan_to_num(np.abs(got[1][:, j] - want[1][:, j])) <= TOL), (what, j, got[1][:, j], want[1][:, j])
    if len(want) > 2:
        assert got[2].shape == want[2].shape and np.array_equal(np.isnan(got[2]), np.isnan(want[2])), what
        assert np.all(np.nan_to_num(np.abs(got[2] - want[2])) <= TOL), what


def test_sizes_around_every_path():
    # n = 1 (one class by force), 2, 3; the workgroup width; a sort that pads by one / fills its power of two; the LDS limit
    sizes = [1, 2, 3, 255, 256, 257, 4096, 4097, 8191, 8192]
    sets = [draw(100 + n, n, ties=(0 if k % 2 else 37)) for k, n in enumerate(sizes)]
    got, want = device_points(sets, roc_grid=33), host_points(sets, roc_grid=33)
    held(got, want, "sizes")
    assert got[0][0, 0, 7] == -2.0 and np.all(got[0][1:, :, 7] >= 0.0)
    assert list(got[1][:, 5][1:]) == [R.Curve(*s).K for s in sets[1:]]


def edge_sets():
    inf = np.float32(np.inf)
    y40 = np.r_[np.ones(15, dtype=np.int32), np.zeros(25, dtype=np.int32)]
    a, ya = draw(7, 300)
    sets = {
        "all_equal": (np.full(40, 0.5, dtype=np.float32), y40),
        "all_distinct": draw(1, 700),
        "heavy_ties": draw(2, 700, ties=3),
        "signed_zero": (np.array([0.0, -0.0, 0.5, -0.5, 0.0, -0.0, 0.25], dtype=np.float32), np.array([1, 0, 1, 0, 0, 1, 0], dtype=np.int32)),
        "infinities": (np.r_[a[:40], [inf, inf, -inf, -inf, inf]].astype(np.float32), np.r_[ya[:40], [1, 0, 1, 0, 1]].astype(np.int32)),
        "inf_control_on_top": (np.r_[a[:40], [inf]].astype(np.float32), np.r_[ya[:40], [0]].astype(np.int32)),
        "below_grid": draw(3, 300, shift=-3.0),
        "above_grid": draw(4, 300, shift=2.0),
        "control_on_top": (np.r_[a, [5.0]].astype(np.float32), np.r_[ya, [0]].astype(np.int32)),
        "reversed": (lambda sy: ((1 - sy[0]).astype(np.float32), sy[1]))(draw(5, 300)),
    }
    return sets


def test_edge_sets():
    sets = edge_sets()
    names = sorted(sets)
    got, want = device_points([sets[k] for k in names], roc_grid=50), host_points([sets[k] for k in names], roc_grid=50)
    held(got, want, names)
    pr = R.RULES.index("pr")
    assert got[0][names.index("control_on_top"), pr, 7] == 1.0 and got[0][names.index("control_on_top"), pr, 0] == 5.0
    zero = got[0][names.index("signed_zero"), :, 0]
    assert not np.signbit(zero[zero == 0.0]).any()                      # -0 and +0 are one threshold, reported as +0
    held(device_points([sets[k] for k in names], grid=(-1.0, 3.0, 7)), host_points([sets[k] for k in names], grid=(-1.0, 3.0, 7)), "custom grid")
    held(device_points([sets[k] for k in names], max_fpr=1.0, spec=1.0, sens=1.0), host_points([sets[k] for k in names], max_fpr=1.0, spec=1.0, sens=1.0), "ends")
    held(device_points([sets[k] for k in names], max_fpr=0.37, spec=0.0, sens=0.0), host_points([sets[k] for k in names], max_fpr=0.37, spec=0.0, sens=0.0), "zeros")


def test_sets_without_a_curve_leave_their_neighbours_alone():
    good = [draw(11, 171), draw(12, 300, ties=5), draw(13, 64)]
    empty = (np.zeros(0, dtype=np.float32), np.zeros(0, dtype=np.int32))
    ones = (draw(14, 50)[0], np.ones(50, dtype=np.int32))
    zeros = (draw(15, 50)[0], np.zeros(50, dtype=np.int32))
    nan = draw(16, 90)
    nan[0][17] = np.nan
    sets = [good[0], empty, good[1], ones, zeros, good[2], nan]
    got, want = device_points(sets, roc_grid=20), host_points(sets, roc_grid=20)
    held(got, want, "mixed")
    alone = device_points(good, roc_grid=20)
    for k, j in enumerate((0, 2, 5)):
        for a, b in zip(got, alone):
            assert a[j].tobytes() == b[k].tobytes()
    for j in (1, 3, 4, 6):
        assert np.all(got[0][j, :, 7] == -2.0) and np.isnan(got[0][j, :, :7]).all() and np.isnan(got[2][j]).all()
    # a valid selection on a set without positives, without negatives, and on an empty one
    sel = dict(select_of=[0, 0, 0, 0, 1], evaluate=[3, 4, 1, 6, 0])
    held(device_points(sets, **sel), host_points(sets, **sel), "evaluation sets")
    pts = device_points(sets, **sel)[0]
    assert np.isnan(pts[0, :, 3]).all() and not np.isnan(pts[0, :, 2]).any()          # positives only: no specificity
    assert np.isnan(pts[1, :, 2]).all() and not np.isnan(pts[1, :, 3]).any()          # negatives only: no recall
    assert np.all(pts[2, :, 7] == -2.0) and np.all(pts[4, :, 7] == -2.0)


def test_roc_rule_and_auc_are_posthoc_metrics_bytes():
    sets = [draw(20 + k, n, ties=t) for k, (n, t) in enumerate([(171, 0), (1064, 0), (300, 4), (2, 0), (257, 11), (8192, 0), (40, 1)])]
    sets.append(edge_sets()["reversed"])
    ph = metrics.posthoc_metrics([torch.from_numpy(s) for s, _ in sets], [torch.from_numpy(l) for _, l in sets]).cpu().numpy()
    pts, summ = device_points(sets, rules=("roc",))
    assert pts[:, 0, 0].tobytes() == ph[:, 1].tobytes() and summ[:, 0].tobytes() == ph[:, 0].tobytes()
    for col_op, col_ph in ((1, 2), (2, 3), (3, 4)):
        assert pts[:, 0, col_op].tobytes() == ph[:, col_ph].tobytes()
    assert summ[:, 6:].tobytes() == ph[:, 6:].tobytes()


def test_launch_shape_does_not_matter():
    sets = [draw(300 + k, 20 + (k * 37) % 400, ties=(k % 5) * 3) for k in range(300)]
    whole = device_points(sets, roc_grid=16)
    again = device_points(sets, roc_grid=16)
    for a, b in zip(whole, again):
        assert a.tobytes() == b.tobytes()
    for k in (0, 1, 149, 299):
        for a, b in zip(whole, device_points([sets[k]], roc_grid=16)):
            assert a[k].tobytes() == b[0].tobytes(), k
    few = sets[:12]
    allr = device_points(few)
    for k, rule in enumerate(R.RULES):
        one = device_points(few, rules=(rule,))
        assert one[0][:, 0].tobytes() == np.ascontiguousarray(allr[0][:, k]).tobytes(), rule
        assert one[1].tobytes() == allr[1].tobytes()
    held(whole, host_points(sets, roc_grid=16), "300 sets")


def test_fold_mapping():
    sets = [draw(40 + k, 150 + 10 * k, ties=(0, 6, 0, 25)[k]) for k in range(4)]
    n = len(sets)
    forms = {
        "identity": dict(select_of=list(range(n)), evaluate=list(range(n))),
        "all on one": dict(select_of=[2] * n, evaluate=list(range(n))),
        "permutation": dict(select_of=[3, 0, 1, 2], evaluate=[1, 2, 3, 0]),
        "never selected on": dict(select_of=[0, 1, 0], evaluate=[3, 3, 2]),
        "repeats": dict(select_of=[1, 1, 1, 2, 2, 0, 3], evaluate=[0, 0, 1, 1, 3, 3, 3]),
    }
    for what, kw in forms.items():
        held(device_points(sets, **kw), host_points(sets, **kw), what)
    plain, ident = device_points(sets), device_points(sets, **forms["identity"])
    assert plain[0].tobytes() == ident[0].tobytes()
    # the threshold is the selection set's, the counts the evaluation set's
    pts = device_points(sets, **forms["all on one"])[0]
    assert np.all(pts[:, :, 0] == pts[2, :, 0]) and np.all(pts[:, :, 6][:, :] == pts[2, :, 6])
    s, l = sets[0]
    for k in range(len(R.RULES)):
        pred = s.astype(np.float64) >= pts[0, k, 0]
        assert (pts[0, k, 4], pts[0, k, 5]) == ((pred & (l != 0)).sum(), (pred & (l == 0)).sum())


def test_classification_performance_has_the_reference_meaning():
    s, l = draw(77, 171)
    c = R.Curve(s, l)
    auc = R.summary(c)[0]
    for method in ("roc", "f1", "pr", "cost", "eer"):
        row = R.apply(*R.select(c, method), s, l)
        got = metrics.classification_performance(torch.from_numpy(s), torch.from_numpy(l), method=method)
        assert len(got) == 5 and same_bits(got, [auc, row[1], row[2], row[3], auc / (1 - auc)]), method
    row = R.apply(0.4, math.nan, 0.0, s, l)
    got = metrics.classification_performance(s, l, optimal_threshold=0.4)
    assert same_bits(got, [auc, row[1], row[2], row[3], auc / (1 - auc)])
    with pytest.raises(ValueError):
        metrics.classification_performance(s, l, method="f1max")


def test_c_entry_without_summary_and_grid():
    import ctypes as C
    from multi_modal_normative_modeling_amd.engine import _stream_ptr
    s, l = draw(5, 100)
    dev = torch.device("cuda:0")
    sd, ld = torch.from_numpy(s).to(dev), torch.from_numpy(l).to(dev)
    off = torch.tensor([0, 100], dtype=torch.int32, device=dev)
    rules = (_lib.NmOpRule * 2)()
    rules[0].kind, rules[1].kind = _lib.NM_OP_ROC, _lib.NM_OP_F1MAX
    lib = _lib.load()
    need = lib.nm_operating_points_workspace(1, 2)
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    out = torch.empty(1, 2, 8, dtype=torch.float64, device=dev)
    _lib.check(lib.nm_operating_points(sd.data_ptr(), ld.data_ptr(), off.data_ptr(), 1, 100, rules, 2, None, 1, None, 0.9, 0.9, 0.1,
                                       ws.data_ptr(), need, out.data_ptr(), None, None, 0, _stream_ptr(dev)))
    want = device_points([(s, l)], rules=("roc", "f1max"))[0]
    assert out.cpu().numpy().tobytes() == want.tobytes()
