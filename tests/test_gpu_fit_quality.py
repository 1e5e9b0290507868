"""nm_fit_quality and nm_fit_rank on the device against the yardstick (tests/fit_quality_ref.py).  In every case the output
buffers start out poisoned, the pad columns of the inputs hold NaN / +-inf, and x, loc and var have different pitches.  The
closeness rules (R.close): n_obs, n_var, the tie counts, status words and the NaN pattern exactly; spearman and t_spearman bit for
bit; everything else within 1e-9 x max(1, |ref|), p-values within 1e-9 relative -- 1e-9 is at least 1000 times the yardstick's
own summation-order noise (tests/test_fit_quality_ref_cpu.py measures it, <= 1e-12 for every column).  coverage is compared
through the same rule after asserting on the yardstick alone that no |z| lies within 1e-6 of the threshold, and rho after
asserting that |rho| < 1 - 1e-6 outside the planted columns (conditions on the inputs, not allowances for the kernel)."""
import numpy as np
import pytest
import torch

from multi_modal_normative_modeling_amd import _lib, metrics
from multi_modal_normative_modeling_amd.engine import _stream_ptr
from tests import fit_quality_ref as R
from tests.table_stats_util import upload as _upload

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
POISON = -1.2345e300
THR = 1.96
WIDTHS = [1, 63, 64, 65, 130]
HEIGHTS = [1, 2, 3, 4, 127, 128, 129, 300]
PLANTED = 8                        # the first columns of a wide, tall case carry one planted condition each
# seeds moved on the CPU, with the yardstick alone, until input_conditions holds in every case: (D, rows, k) -> added to the seed
SEED_BUMP = {(65, 8192, 3): 100}


def make_case(D, rows, k=0, groups=(-1, 0, 1, 2), mode=None, with_mom=None):
    """One (width, height) cell: (x, loc, var or None, col_var or None, group, trivial [D, 8] or None).  The variance mode walks
    through none / var / col_var / both with D + rows + k; every other cell has a trivial model.  Wide, tall cells plant, a
    column each: 0 a NaN in an evaluated row, 1 an inf in a left-out row, 2 a constant prediction, 3 a zero and 4 a negative s2,
    5 an invalid trivial column, 6 heavy ties (values rounded to one decimal), 7 +-0.0."""
    rng = np.random.default_rng(10007 * D + 13 * rows + k + SEED_BUMP.get((D, rows, k), 0))
    x, loc, var, cv, g = R.make_case(rng, rows, D, groups=groups)
    mode = (D + rows + k) % 4 if mode is None else mode
    with_mom = bool((D + rows // 2 + k) % 2) if with_mom is None else with_mom
    train = rng.normal(size=(50, D)) * rng.uniform(0.5, 3.0, D) + rng.uniform(-5.0, 5.0, D)
    triv = np.zeros((D, 8))
    triv[:, 0], triv[:, 2], triv[:, 3] = train.mean(0), train.var(0), 50
    triv[:, 1] = np.sqrt(triv[:, 2])
    ev, out = np.flatnonzero(g == 0), np.flatnonzero(g != 0)
    if D >= 63 and len(ev) >= 20 and len(out) >= 2:
        x[ev[2], 0] = np.nan
        loc[out[1], 1] = np.inf
        loc[:, 2] = np.float32(0.25)
        var[ev[3], 3], cv[3] = 0.0, 0.0
        var[ev[4], 4] = -(abs(cv[4]) + 1.0)
        if mode == 2:
            cv[4] = -0.5
        triv[5, :3], triv[5, 7] = np.nan, -2.0
        x[:, 6], loc[:, 6] = np.round(x[:, 6], 1), np.round(loc[:, 6], 1)
        x[ev[5], 7], x[ev[6], 7], loc[ev[7], 7], loc[ev[8], 7] = 0.0, -0.0, -0.0, 0.0
    return x, loc, (var if mode in (1, 3) else None), (cv if mode in (2, 3) else None), g, (triv if with_mom else None)


def planted(D, g):
    return D >= 63 and (g == 0).sum() >= 20 and (g != 0).sum() >= 2


def input_conditions(x, loc, var, cv, g, fit, thr=THR):
    """What the comparison of coverage and of rho near +-1 rests on, asserted on the yardstick alone."""
    ev = g == 0
    s2 = R.s2_table(x.shape, var, cv)
    if s2 is not None:
        with np.errstate(all="ignore"):
            z = (x[ev].astype(np.float64) - loc[ev].astype(np.float64)) / np.sqrt(s2[ev])
            assert not np.any(np.abs(np.abs(z) - thr) < 1e-6), "a |z| within 1e-6 of the threshold: pick another seed"
    first = PLANTED if planted(x.shape[1], g) else 0
    rho = fit[first:, 0]
    if ev.sum() >= 3:
        assert np.all(np.abs(rho[~np.isnan(rho)]) < 1 - 1e-6), "|rho| within 1e-6 of 1: pick another seed"


def _poisoned(*shape):
    return torch.full(shape, POISON, dtype=torch.float64, device=DEV)


def run(views, locs, groups, vars_=None, cvs=None, mom=None, ref_of=None, thr=THR, max_rows=None, patch=None, rank=True):
    """(fit, cal, rank) [n_sets, D, 8] of the C entry points on poisoned outputs.  patch: {set index: {field: value}} written into
    the pointer table after it is built (the refused sets)."""
    D = int(views[0].shape[1])
    grp = [torch.as_tensor(np.asarray(g, dtype=np.int32)).to(DEV) for g in groups]
    cv_dev = None if cvs is None else [None if c is None else torch.as_tensor(np.asarray(c, dtype=np.float32)).to(DEV) for c in cvs]
    table = metrics._fit_table(views, locs, grp, vars_, cv_dev)
    for k, fields in (patch or {}).items():
        for name, v in fields.items():
            setattr(table[k], name, v)
    sets = torch.frombuffer(bytearray(bytes(table)), dtype=torch.uint8).to(DEV)
    n = len(views)
    fo, co, ro = _poisoned(n, D, 8), _poisoned(n, D, 8), _poisoned(n, D, 8)
    m = torch.as_tensor(np.ascontiguousarray(mom)).to(DEV) if mom is not None else None
    rf = torch.tensor(ref_of, dtype=torch.int32, device=DEV) if ref_of is not None else None
    lib, mr = _lib.load(), max_rows or metrics._max_rows(views)
    _lib.check(lib.nm_fit_quality(sets.data_ptr(), n, D, mr, m.data_ptr() if m is not None else None,
                                  int(m.shape[0]) if m is not None else 0, rf.data_ptr() if rf is not None else None, thr,
                                  fo.data_ptr(), co.data_ptr(), _stream_ptr(DEV)), "nm_fit_quality")
    if rank:
        _lib.check(lib.nm_fit_rank(sets.data_ptr(), n, D, mr, ro.data_ptr(), _stream_ptr(DEV)), "nm_fit_rank")
    torch.cuda.synchronize()
    got = [t.cpu().numpy() for t in ((fo, co, ro) if rank else (fo, co))]
    for t in got:
        assert not np.any(t == POISON), "an output element was not written"
    return got if rank else got + [None]


def upload_case(x, loc, var, D):
    return _upload(x, D + 3), _upload(loc, D + 1), None if var is None else _upload(var, D + 2)


def check(got, case, what):
    x, loc, var, cv, g, triv = case
    fit, cal = R.quality(x, loc, g, var, cv, triv, thr=THR)
    input_conditions(x, loc, var, cv, g, fit)
    worst = [R.close(got[0], fit, "fit"), R.close(got[1], cal, "cal")]
    if got[2] is not None:
        worst.append(R.close(got[2], R.rank(x, loc, g), "rank"))
    print(what, "worst error / bound (fit, cal, rank):", worst)
    assert max(worst) <= 1.0, what
    return fit, cal


@pytest.mark.parametrize("D", WIDTHS)
def test_widths_and_heights(D):
    seen = set()
    for rows in HEIGHTS:
        case = make_case(D, rows)
        x, loc, var, cv, g, triv = case
        vx, vl, vv = upload_case(x, loc, var, D)
        got = run([vx], [vl], [g], None if vv is None else [vv], None if cv is None else [cv],
                  None if triv is None else triv[None], None if triv is None else [0])
        fit, _ = check([t[0] for t in got], case, f"D={D} rows={rows} var={var is not None} col_var={cv is not None} "
                                                 f"trivial={triv is not None} n={int((g == 0).sum())}")
        seen |= set(fit[:, 7].tolist())
        if planted(D, g):
            st = fit[:PLANTED, 7]
            assert st[0] == -2 and st[1] == st[6] == st[7] and int(st[2]) & 1 and not int(st[1]) & 1
            if var is not None or cv is not None:
                assert int(st[3]) & 2 and int(st[4]) & 2 and not int(st[1]) & 2
            if triv is not None:
                assert int(st[5]) & 4 and not int(st[1]) & 4
    if D >= 63:
        assert {-2.0, 0.0} <= seen and any(int(s) & 1 for s in seen if s > 0) and any(int(s) & 2 for s in seen if s > 0)


@pytest.mark.parametrize("mode", [0, 1, 2, 3])
def test_every_variance_mode_with_and_without_the_trivial_model(mode):
    for with_mom in (False, True):
        case = make_case(65, 129, k=40 + mode, mode=mode, with_mom=with_mom)
        x, loc, var, cv, g, triv = case
        assert (var is not None) == (mode in (1, 3)) and (cv is not None) == (mode in (2, 3)) and (triv is not None) == with_mom
        vx, vl, vv = upload_case(x, loc, var, 65)
        got = run([vx], [vl], [g], None if vv is None else [vv], None if cv is None else [cv],
                  None if triv is None else triv[None], None)
        fit, cal = check([t[0] for t in got], case, f"mode={mode} trivial={with_mom}")
        clean = fit[PLANTED:]
        assert np.all(clean[:, 7] == (2 if mode == 0 else 0) + (0 if with_mom else 4))
        assert np.isnan(clean[:, 4]).all() == (mode == 0 or not with_mom) and np.isnan(cal[PLANTED:, 2:7]).all() == (mode == 0)


def test_the_largest_set_and_the_int64_bound():
    case = make_case(65, 8192, k=3, groups=(0,), mode=3, with_mom=True)
    x, loc, var, cv, g, triv = case
    x[:, 9], loc[:, 9] = np.round(x[:, 9]), np.round(loc[:, 9])           # a handful of distinct values: the largest tie blocks
    x[:, 10] = np.arange(8192, dtype=np.float32)
    loc[:, 10] = x[:, 10] * 0.5 + np.where(np.arange(8192) % 2, 400.0, -400.0).astype(np.float32)  # all distinct, no tie at all
    vx, vl, vv = upload_case(x, loc, var, 65)
    got = run([vx], [vl], [g], [vv], [cv], triv[None], [0])
    check([t[0] for t in got], case, "8192 x 65")
    assert np.all(got[2][0][:, 3] == 8192) and got[2][0][9, 4] > 8000 and got[2][0][10, 4] == 0 and got[2][0][10, 5] == 0 and got[2][0][10, 0] > 0.9


def _mixed():
    """Twenty sets of width 70 with different heights, pitches and variance modes, the third a row slice out of a taller buffer;
    three trivial models, ref_of crossing the sets and -1."""
    heights = [33, 137, 58, 1, 300, 2, 129, 64, 3, 200, 127, 4, 90, 128, 256, 17, 65, 150, 5, 299]
    cases = [make_case(70, r, k=5 + i) for i, r in enumerate(heights)]
    ups = [upload_case(c[0], c[1], c[2], 70) for c in cases]
    tall = _upload(np.concatenate([cases[0][0][:11], cases[2][0], cases[0][0][:6]]), 80)
    ups[2] = (tall[11:11 + 58], ups[2][1], ups[2][2])
    moms = np.stack([make_case(70, 40, k=900 + j, with_mom=True)[5] for j in range(3)])
    moms[1, 11, 7], moms[2, 12, 2] = -2.0, 0.0                              # an invalid trivial column each
    ref_of = [(i * 7) % 4 - 1 for i in range(len(heights))]                 # -1, 0, 1, 2 across the sets
    cases = [(c[0], c[1], c[2], c[3], c[4], None if r < 0 else moms[r]) for c, r in zip(cases, ref_of)]
    return cases, ups, moms, ref_of


def _launch(cases, ups, moms, ref_of, idx, **kw):
    return run([ups[i][0] for i in idx], [ups[i][1] for i in idx], [cases[i][4] for i in idx], [ups[i][2] for i in idx],
               [cases[i][3] for i in idx], moms, [ref_of[i] for i in idx], **kw)


def test_twenty_sets_alone_elsewhere_and_again():
    cases, ups, moms, ref_of = _mixed()
    idx = list(range(20))
    got = _launch(cases, ups, moms, ref_of, idx)
    for i in idx:
        fit, _ = check([t[i] for t in got], cases[i], f"set {i}")
        if ref_of[i] < 0:
            assert np.all(fit[fit[:, 7] >= 0, 7].astype(int) & 4)
    assert ref_of[6] == 1 and ref_of[1] == 2                                 # their trivial models hold an invalid column each
    for i, col in ((6, 11), (1, 12)):
        assert got[0][i][col, 7] >= 4 and np.isnan(got[0][i][col, 4]) and got[0][i][col + 1, 7] < 4
    again = _launch(cases, ups, moms, ref_of, idx)
    for a, b in zip(got, again):
        assert a.tobytes() == b.tobytes()
    order = idx[7:] + idx[:7]                                               # every set at another index
    moved = _launch(cases, ups, moms, ref_of, order)
    for t, m in zip(got, moved):
        for pos, i in enumerate(order):
            assert t[i].tobytes() == m[pos].tobytes(), i
    for i in (1, 4, 8):
        alone = _launch(cases, ups, moms, ref_of, [i])
        for t, a in zip(got, alone):
            assert t[i].tobytes() == a[0].tobytes(), i


def test_refused_sets_among_good_ones():
    cases, ups, moms, ref_of = _mixed()
    idx = [0, 1, 2, 4, 6, 9]
    good = _launch(cases, ups, moms, ref_of, idx)
    patch = {1: {"rows": -1}, 3: {"rows": 301}, 4: {"pitch": 69}}
    got = _launch(cases, ups, moms, ref_of, idx, max_rows=300, patch=patch)
    for pos in range(len(idx)):
        fit, cal, rk = (t[pos] for t in got)
        if pos in patch:
            assert np.isnan(fit[:, :6]).all() and np.all(fit[:, 6] == 0) and np.all(fit[:, 7] == -2)
            assert np.isnan(cal[:, :7]).all() and np.all(cal[:, 7] == 0)
            assert np.isnan(rk[:, [0, 1, 2, 4, 5]]).all() and np.all(rk[:, [3, 6]] == 0) and np.all(rk[:, 7] == -2)
        else:
            for t, g in zip(got, good):
                assert t[pos].tobytes() == g[pos].tobytes(), pos
    for fields in ({"loc_pitch": 69}, {"var_pitch": 69}, {"x": None}, {"loc": None}, {"group": None}, {"rows": 138}):
        t = _launch(cases, ups, moms, ref_of, [0, 1], max_rows=137, patch={1: fields})
        assert ups[1][2] is not None or "var_pitch" not in fields
        assert np.all(t[0][1][:, 7] == -2) and np.all(t[2][1][:, 7] == -2) and np.isnan(t[0][1][:, :6]).all(), fields
        assert t[0][0].tobytes() == good[0][0].tobytes() and t[2][0].tobytes() == good[2][0].tobytes()


def test_the_public_function_is_the_same_launch():
    cases, ups, moms, ref_of = _mixed()
    idx = [0, 1, 4, 6]
    want = _launch(cases, ups, moms, ref_of, idx)
    kw = dict(var=[ups[i][2] for i in idx], col_var=[None if cases[i][3] is None else torch.from_numpy(cases[i][3]) for i in idx],
              moments=torch.from_numpy(moms), ref_of=[ref_of[i] for i in idx], thr=THR)
    args = ([ups[i][0] for i in idx], [ups[i][1] for i in idx], [cases[i][4] for i in idx])
    res = metrics.fit_quality(*args, rank=True, **kw)
    assert len(res) == 3 and all(r.dtype == torch.float64 and r.is_cuda and tuple(r.shape) == (4, 70, 8) for r in res)
    for r, w in zip(res, want):
        assert r.cpu().numpy().tobytes() == w.tobytes()
    two = metrics.fit_quality(*args, **kw)
    assert len(two) == 2 and two[0].cpu().numpy().tobytes() == want[0].tobytes()
    bare = metrics.fit_quality(*args)                                       # no variance, no trivial model: bits 2 and 4
    st = bare[0][..., 7].cpu().numpy()
    assert np.all((st == -2) | ((st.astype(int) & 6) == 6)) and np.isnan(bare[1][..., 2:7].cpu().numpy()).all()
