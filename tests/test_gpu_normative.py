"""nm_cohort_moments, nm_normative_z, nm_cohort_cov and nm_mahalanobis on the device against the yardstick
(tests/normative_ref.py).  In every case the output buffers start out poisoned and the pad columns D..pitch of the inputs hold
NaN / +-inf.  The closeness rules (R.close): status words, row counts, the NaN pattern and argmax_z exactly; mean and sd within
1e-9 x max(|mean|, sd); the fp32 z table within one fp32 ulp of the yardstick's z rounded to fp32 (the kernel rounds an fp64
value that may sit at a rounding boundary); n_hi / n_lo exactly, after asserting on the yardstick alone that no |z| lies within
1e-6 of the threshold and no |mean| / sd exceeds 1e3 (conditions on the inputs, not allowances for the kernel); d2 within 1e-9
relative at condition numbers <= 1e3 (expected Z x cond x 2^-52 ~ 2e-11 at the largest case).  1e-9 is 1e6 times the
yardstick's own summation-order noise (tests/test_normative_ref_cpu.py prints it)."""
import numpy as np
import pytest
import torch

from multi_modal_normative_modeling_amd import _lib, metrics
from multi_modal_normative_modeling_amd.engine import _stream_ptr
from tests import normative_ref as R
from tests.table_stats_util import upload as _upload

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
POISON = -1.2345e300
THR = 1.96
WIDTHS = [1, 63, 64, 65, 130]
HEIGHTS = [1, 2, 127, 128, 129, 300]
# seeds moved on the CPU, with the yardstick alone, until input_conditions holds in every case: (D, rows) -> added to the seed
SEED_BUMP = {(65, 127): 100}


def make_case(D, rows, k=0):
    """The table of one (width, height) cell: groups drawn from {-1, 0, 1, 2}; every other cell has a `sub` matrix; tall cells
    carry a NaN in a reference row (that column's moments are refused) and an inf in a scored row (that z is NaN).  Returns
    (x, group, sub or None, ddof)."""
    rng = np.random.default_rng(10007 * D + 13 * rows + k + SEED_BUMP.get((D, rows), 0))
    x, g = R.make_table(rng, rows, D)
    ddof = (D + rows + k) % 2
    sub = (0.3 * rng.normal(size=x.shape)).astype(np.float32) if (D + rows // 2 + k) % 2 else None
    if rows >= 127 and D >= 63:
        x[np.flatnonzero(g == 0)[2], 5] = np.nan
        x[np.flatnonzero(g != 0)[1], D - 1] = np.inf
    return x, g, sub, ddof


def input_conditions(x, g, sub, mom, thr=THR):
    """What the exact comparison of n_hi / n_lo rests on, asserted on the yardstick alone."""
    z = R.z_table(x, mom, sub)
    ok = mom[:, 7] == 0
    with np.errstate(invalid="ignore"):
        assert not np.any(np.abs(np.abs(z) - thr) < 1e-6), "a |z| within 1e-6 of the threshold: pick another seed"
        assert not np.any(np.abs(mom[ok, 0]) / mom[ok, 1] > 1e3), "|mean| / sd above 1e3: pick another seed"
    return z


def _table(views, groups, subs=None, zs=None, rows=None, pitches=None):
    grp = [torch.as_tensor(np.asarray(g, dtype=np.int32)).to(DEV) for g in groups] if groups is not None else None
    table = metrics._norm_table(views, grp, subs, zs)
    for k in range(len(views)):
        if rows is not None and rows[k] is not None:
            table[k].rows = rows[k]
        if pitches is not None and pitches[k] is not None:
            table[k].pitch = pitches[k]
    return torch.frombuffer(bytearray(bytes(table)), dtype=torch.uint8).to(DEV), grp


def _poisoned(*shape, dtype=torch.float64):
    return torch.full(shape, POISON if dtype == torch.float64 else -7.0e30, dtype=dtype, device=DEV)


def _moments(views, groups, subs=None, ddof=1, max_rows=None, rows=None, pitches=None):
    D = int(views[0].shape[1])
    sets, keep = _table(views, groups, subs, rows=rows, pitches=pitches)
    out = _poisoned(len(views), D, 8)
    _lib.check(_lib.load().nm_cohort_moments(sets.data_ptr(), len(views), D, max_rows or metrics._max_rows(views), ddof,
                                              out.data_ptr(), _stream_ptr(DEV)), "nm_cohort_moments")
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert not np.any(got == POISON)
    return got


def _zscore(views, groups, mom, subs=None, ref_of=None, thr=THR, want_z=True, max_rows=None, rows=None, pitches=None):
    """(z tables with their pad columns, rows, cols) of the C entry point on poisoned outputs."""
    D = int(views[0].shape[1])
    zb = [_poisoned(int(v.shape[0]), D + 2, dtype=torch.float32) for v in views] if want_z else None
    sets, keep = _table(views, groups, subs, None if zb is None else [b[:, :D] for b in zb], rows=rows, pitches=pitches)
    total = sum(int(v.shape[0]) for v in views)
    ro, co = _poisoned(max(total, 1), 8), _poisoned(len(views), D, 8)
    m = torch.as_tensor(np.ascontiguousarray(mom)).to(DEV)
    rf = torch.tensor(ref_of, dtype=torch.int32, device=DEV) if ref_of is not None else None
    _lib.check(_lib.load().nm_normative_z(sets.data_ptr(), len(views), D, max_rows or metrics._max_rows(views), m.data_ptr(),
                                           int(m.shape[0]), rf.data_ptr() if rf is not None else None, thr, ro.data_ptr(),
                                           co.data_ptr(), _stream_ptr(DEV)), "nm_normative_z")
    torch.cuda.synchronize()
    zs = None if zb is None else [b.cpu().numpy() for b in zb]
    return zs, ro.cpu().numpy()[:total], co.cpu().numpy()


def _check_z(zs_k, rows_k, cols_k, x, g, sub, mom, what):
    z = input_conditions(x, g, sub, mom)
    D = x.shape[1]
    worst = [R.close(rows_k, R.row_summary(z, THR), "rows"), R.close(cols_k, R.col_summary(z, g, mom, THR), "cols")]
    if zs_k is not None:
        assert np.all(zs_k[:, D:] == np.float32(-7.0e30)), "pad columns of the z table were touched"
        worst.append(R.close(np.ascontiguousarray(zs_k[:, :D]), z, "z32"))
    print(what, "worst error / bound (rows, cols, z):", worst)
    assert max(worst) <= 1.0, what


@pytest.mark.parametrize("D", WIDTHS)
def test_widths_and_heights(D):
    for rows in HEIGHTS:
        x, g, sub, ddof = make_case(D, rows)
        v = _upload(x, D + 3)
        sb = None if sub is None else [_upload(sub, D + 1)]
        ref = R.moments(x, g, sub, ddof)
        got = _moments([v], [g], sb, ddof)[0]
        worst = R.close(got, ref, "moments")
        print(f"D={D} rows={rows} ddof={ddof} sub={sub is not None} n_ref={int(ref[0, 3])}: moments worst error / bound", worst)
        assert worst <= 1.0
        # the z pass on the yardstick's moments, then on the device's own
        for mom in (ref, got):
            zs, ro, co = _zscore([v], [g], mom[None], sb)
            _check_z(zs[0], ro, co[0], x, g, sub, ref, f"D={D} rows={rows}")
        _, ro2, co2 = _zscore([v], [g], got[None], sb, want_z=False)
        assert ro2.tobytes() == ro.tobytes() and co2.tobytes() == co.tobytes()


def test_no_reference_row_and_one_reference_row():
    x, g, _, _ = make_case(65, 129, k=1)
    for n_ref, ddof in ((0, 0), (0, 1), (1, 0), (1, 1), (2, 1)):
        gg = np.where(g == 0, 2, g)
        gg[np.flatnonzero(g == 1)[:n_ref]] = 0
        v = _upload(x, 70)
        ref = R.moments(x, gg, None, ddof)
        got = _moments([v], [gg], None, ddof)[0]
        assert R.close(got, ref, "moments") <= 1.0
        assert np.all(got[:, 3] == n_ref) and (np.all(got[:, 7] == -2) if n_ref < 2 else np.all(got[[0, 1, 2], 7] == 0))
        zs, ro, co = _zscore([v], [gg], got[None])
        _check_z(zs[0], ro, co[0], x, gg, None, ref, f"n_ref={n_ref} ddof={ddof}")
        if n_ref < 2:
            assert np.all(ro[:, 7] == -2) and np.all(ro[:, 5] == -1) and np.isnan(zs[0][:, :65]).all() and np.isnan(co[0][:, 6:]).all()


def _mixed():
    """Five sets of different heights and pitches, the third a row slice out of a taller buffer; a `sub` matrix for each."""
    shapes = [(33, 72), (137, 70), (58, 80), (1, 71), (300, 76)]
    cases = [make_case(70, r, k=5 + i) for i, (r, _) in enumerate(shapes)]
    xs, gs = [c[0] for c in cases], [c[1] for c in cases]
    views = [_upload(x, p) for x, (_, p) in zip(xs, shapes)]
    tall = _upload(np.concatenate([xs[0][:11], xs[2], xs[0][:6]]), 80)
    views[2] = tall[11:11 + 58]
    assert not views[2].is_contiguous() and views[2].data_ptr() == tall.data_ptr() + 11 * 80 * 4
    rng = np.random.default_rng(99)
    subs = [(0.3 * rng.normal(size=x.shape)).astype(np.float32) for x in xs]
    return views, xs, gs, subs


@pytest.mark.parametrize("with_sub", [False, True])
def test_five_sets_in_one_launch_through_the_host_functions(with_sub):
    views, xs, gs, subs = _mixed()
    sb = [_upload(s, s.shape[1] + 2) for s in subs] if with_sub else None
    hs = subs if with_sub else [None] * 5
    ptrs = [v.data_ptr() for v in views]
    mom = metrics.cohort_moments(views, gs, sub=sb, ddof=1, device=DEV)
    assert mom.dtype == torch.float64 and mom.is_cuda and tuple(mom.shape) == (5, 70, 8)
    refs = [R.moments(x, g, s, 1) for x, g, s in zip(xs, gs, hs)]
    for k in range(5):
        assert R.close(mom[k].cpu().numpy(), refs[k], "moments") <= 1.0, k
    # statistics of one table applied to another: ref_of points across sets
    ref_of = [4, 4, 1, 4, 1]
    z, rows, cols = metrics.normative_z(views, gs, mom, ref_of=ref_of, thr=THR, sub=sb, device=DEV)
    assert [v.data_ptr() for v in views] == ptrs and tuple(rows.shape) == (529, 8) and tuple(cols.shape) == (5, 70, 8)
    rows_k = torch.split(rows, [33, 137, 58, 1, 300])
    for k in range(5):
        assert z[k].dtype == torch.float32 and tuple(z[k].shape) == (xs[k].shape[0], 70)
        _check_z(z[k].cpu().numpy(), rows_k[k].cpu().numpy(), cols[k].cpu().numpy(), xs[k], gs[k], hs[k], refs[ref_of[k]], f"set {k}")
    none, rows2, cols2 = metrics.normative_z(views, gs, mom, ref_of=ref_of, thr=THR, sub=sb, return_z=False, device=DEV)
    assert none is None and torch.equal(rows2, rows) and torch.equal(cols2.nan_to_num(7.0), cols.nan_to_num(7.0))
    # two launches on poisoned outputs: the same bytes
    a, b = _moments(views, gs, sb), _moments(views, gs, sb)
    assert a.tobytes() == b.tobytes() == mom.cpu().numpy().tobytes()
    za, ra, ca = _zscore(views, gs, a, sb, ref_of=ref_of)
    zb, rb, cb = _zscore(views, gs, a, sb, ref_of=ref_of)
    assert ra.tobytes() == rb.tobytes() == rows.cpu().numpy().tobytes() and ca.tobytes() == cb.tobytes()
    assert all(p.tobytes() == q.tobytes() for p, q in zip(za, zb))
    # the sets in reverse order: the same bytes, permuted
    rev = lambda seq: None if seq is None else list(seq)[::-1]
    ar = _moments(rev(views), rev(gs), rev(sb))
    assert ar[::-1].tobytes() == a.tobytes()
    zr, rr, cr = _zscore(rev(views), rev(gs), ar, rev(sb), ref_of=[4 - r for r in ref_of][::-1])
    assert cr[::-1].tobytes() == ca.tobytes() and all(p.tobytes() == q.tobytes() for p, q in zip(zr[::-1], za))
    off = np.cumsum([0, 300, 1, 58, 137, 33])
    assert np.concatenate([rr[off[4 - k]:off[5 - k]] for k in range(5)]).tobytes() == ra.tobytes()


def test_refused_table_entries_leave_their_neighbours_alone():
    x, g, _, _ = make_case(65, 50, k=3)
    n, D = x.shape
    v = _upload(x, D + 3)
    ref = R.moments(x, g)
    clean = _moments([v], [g])
    got = _moments([v] * 4, [g] * 4, max_rows=n, rows=[None, n + 1, -1, None], pitches=[None, None, None, D - 1])
    assert got[0].tobytes() == clean[0].tobytes() and R.close(got[0], ref, "moments") <= 1.0
    for k in (1, 2, 3):
        assert np.all(got[k, :, 7] == -2) and np.all(got[k, :, [3, 6]] == 0) and np.isnan(got[k][:, [0, 1, 2, 4, 5]]).all()
    zc, rc, cc = _zscore([v], [g], ref[None])
    zs, ro, co = _zscore([v] * 4, [g] * 4, ref[None], ref_of=[0, 0, 0, 0], max_rows=n, rows=[None, n + 1, -1, None],
                         pitches=[None, None, None, D - 1])
    assert zs[0].tobytes() == zc[0].tobytes() and ro[:n].tobytes() == rc.tobytes() and co[0].tobytes() == cc[0].tobytes()
    assert np.isnan(co[1:]).all()
    # a row count outside 0..max_rows names no rows to write; a bad pitch with a good count gives status rows
    assert np.all(ro[n:3 * n] == POISON) and np.all(ro[3 * n:, 7] == -2) and np.all(ro[3 * n:, 5] == -1) and np.isnan(ro[3 * n:, 2:5]).all()
    assert all(np.all(zs[k] == np.float32(-7.0e30)) for k in (1, 2, 3))
    # a reference index outside the moments table
    _, rb, cb = _zscore([v, v], [g, g], ref[None], ref_of=[0, 1])
    assert rb[:n].tobytes() == rc.tobytes() and np.all(rb[n:, 7] == -2) and np.isnan(cb[1]).all() and cb[0].tobytes() == cc[0].tobytes()


# ---- the latent side ---------------------------------------------------------------------------------------------------------

def _cov(views, groups, Z, ridge, max_rows=None, rows=None, pitches=None):
    sets, keep = _table(views, groups, rows=rows, pitches=pitches)
    mean, chol = _poisoned(len(views), Z), _poisoned(len(views), Z, Z)
    st = torch.full((len(views),), 12345, dtype=torch.int32, device=DEV)
    _lib.check(_lib.load().nm_cohort_cov(sets.data_ptr(), len(views), Z, max_rows or metrics._max_rows(views), ridge, mean.data_ptr(),
                                          chol.data_ptr(), st.data_ptr(), _stream_ptr(DEV)), "nm_cohort_cov")
    torch.cuda.synchronize()
    assert not torch.any(mean == POISON) and not torch.any(chol == POISON) and not torch.any(st == 12345)
    return mean, chol, st


def _maha(views, Z, mean, chol, st, ref_of=None, max_rows=None, rows=None, pitches=None):
    sets, _ = _table(views, None, rows=rows, pitches=pitches)
    total = sum(int(v.shape[0]) for v in views)
    d2, d = _poisoned(total), _poisoned(total)
    rf = torch.tensor(ref_of, dtype=torch.int32, device=DEV) if ref_of is not None else None
    _lib.check(_lib.load().nm_mahalanobis(sets.data_ptr(), len(views), Z, max_rows or metrics._max_rows(views), mean.data_ptr(),
                                           chol.data_ptr(), st.data_ptr(), int(st.numel()), rf.data_ptr() if rf is not None else None,
                                           d2.data_ptr(), d.data_ptr(), _stream_ptr(DEV)), "nm_mahalanobis")
    torch.cuda.synchronize()
    return d2.cpu().numpy(), d.cpu().numpy()


def latent_case(Z, n_ref):
    rng = np.random.default_rng(31 * Z + n_ref)
    return R.make_latent(rng, n_ref, 70, Z)


@pytest.mark.parametrize("Z", [1, 2, 10, 64, 65, 128])
def test_mahalanobis(Z):
    for n_ref in (Z, Z + 1, 4 * Z):
        x, g = latent_case(Z, n_ref)
        x[np.flatnonzero(g != 0)[0], Z - 1] = np.inf              # a scored row with a non-finite entry
        v = _upload(x, Z + 3)
        for ridge in (0.0, 1e-3):
            mean_r, L_r, st_r = R.cov_chol(x, g, ridge)
            mean, chol, st = _cov([v], [g], Z, ridge)
            assert int(st[0]) == st_r, (Z, n_ref, ridge)
            assert st_r == (-2 if (n_ref < 2 or (ridge == 0.0 and n_ref <= Z)) else 0)
            d2, d = _maha([v], Z, mean, chol, st)
            want = R.mahalanobis(x, mean_r, L_r, st_r)
            assert np.isnan(d2[g != 0][0]) and np.array_equal(np.isnan(d), np.isnan(d2))
            if st_r != 0:
                assert torch.isnan(chol).all() and np.isnan(d2).all()
                continue
            cond = np.linalg.cond(L_r @ L_r.T)
            assert cond <= 1e3, (Z, n_ref, ridge, cond)
            worst = [R.close(mean[0].cpu().numpy(), mean_r, "factor"), R.close(chol[0].cpu().numpy(), L_r, "factor"),
                     R.close(d2, want, "rel"), R.close(d, np.sqrt(want), "rel")]
            print(f"Z={Z} n_ref={n_ref} ridge={ridge} cond={cond:.1f}: worst error / bound (mean, factor, d2, d)", worst)
            assert max(worst) <= 1.0 and np.isfinite(np.delete(d2, np.flatnonzero(g != 0)[0])).all()
            assert np.all(np.triu(chol[0].cpu().numpy(), 1) == 0)


def test_latent_sets_in_one_launch_reference_across_sets_and_refusals():
    Z = 10
    cases = [latent_case(Z, n) for n in (40, 11, 10, 25)]                     # (the third: n_ref <= Z, no factor at ridge 0)
    views = [_upload(x, Z + 1 + k) for k, (x, _) in enumerate(cases)]
    gs = [g for _, g in cases]
    mean, chol, st = metrics.cohort_cov(views, gs, ridge=0.0, device=DEV)
    assert st.cpu().tolist() == [0, 0, -2, 0] and tuple(chol.shape) == (4, Z, Z)
    refs = [R.cov_chol(x, g) for x, g in cases]
    ref_of = [1, 0, 3, 2]
    d = metrics.mahalanobis(views, mean, chol, st, ref_of=ref_of, device=DEV)
    for k in range(4):
        want = np.sqrt(R.mahalanobis(cases[k][0], *refs[ref_of[k]]))
        assert d[k].dtype == torch.float64 and R.close(d[k].cpu().numpy(), want, "rel") <= 1.0, k
    assert torch.isnan(d[3]).all()
    # twice the same bytes; the sets reversed: the same bytes, permuted
    a, b = _cov(views, gs, Z, 0.0), _cov(views, gs, Z, 0.0)
    assert all(torch.equal(p.nan_to_num(7.0), q.nan_to_num(7.0)) for p, q in zip(a, b)) and torch.equal(a[1].nan_to_num(7.0), chol.nan_to_num(7.0))
    r = _cov(views[::-1], gs[::-1], Z, 0.0)
    assert all(torch.equal(p.flip(0).nan_to_num(7.0), q.nan_to_num(7.0)) for p, q in zip(r, a))
    d2a, _ = _maha(views, Z, mean, chol, st, ref_of)
    d2b, _ = _maha(views, Z, mean, chol, st, ref_of)
    assert d2a.tobytes() == d2b.tobytes()
    # refused entries: their factor is NaN with status -2, their neighbour's bytes do not change
    n = cases[0][0].shape[0]
    v, g = views[0], gs[0]
    alone = _cov([v], [g], Z, 0.0)
    got = _cov([v] * 4, [g] * 4, Z, 0.0, max_rows=n, rows=[None, n + 1, -1, None], pitches=[None, None, None, Z - 1])
    assert got[2].cpu().tolist() == [0, -2, -2, -2] and torch.equal(got[1][0], alone[1][0]) and torch.isnan(got[1][1:]).all()
    d2r, dr = _maha([v] * 4, Z, alone[0], alone[1], alone[2], ref_of=[0, 0, 0, 0], max_rows=n, rows=[None, n + 1, -1, None],
                    pitches=[None, None, None, Z - 1])
    d21, _ = _maha([v], Z, *alone)
    assert d2r[:n].tobytes() == d21.tobytes() and np.all(d2r[n:3 * n] == POISON) and np.isnan(d2r[3 * n:]).all() and np.isnan(dr[3 * n:]).all()
    _, dbad = _maha([v], Z, *alone, ref_of=[5])
    assert np.isnan(dbad).all()
