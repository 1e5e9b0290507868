"""The modality-subset pass (nm_devpass_subsets: encoders once per tile, then per subset the fusion of that subset's experts,
the full pass's draw, the decoders) --
  anchor        the full subset without presence bytes against nm_devpass_multi on the same job, bit for bit, wherever it sits
                in the list;
  independence  every subset of one launch against the same subset alone, lists permuted, 20 models against each alone;
  oracle        every subset against tests/subset_ref.py in the oracle's fp32 and bf16-operand modes;
  presence      per-row presence bits against the subsets they select, NaN where nothing was observed;
  skipped       decoders an entry does not export are left alone;
  on top        pred_recon_given of the drop-in classes.
Shapes: those of tests/test_gpu_devpass_multi.py -- A (three experts, two full tiles, a ragged one, an empty half), B (four
experts, width and latent at the limits, one row in its second tile), C (two experts, the scalar fusion path, fewer rows
than a tile)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import multi_modal_normative_modeling_amd as nm
from oracle import cvae_ref as R
from tests import subset_ref as S
from tests import twin_cases as T
from tests.golden_util import Golden
from tests.test_gpu_devpass_multi import _data, _job, _tables
from tests.test_gpu_twins import built

DEV = "cuda:0"
COMBINERS = ("poe", "gpoe", "moe", "mopoe")
SHAPES = {
    "A": (300, (61, 90, 47), (64, 48), 12, 3),
    "B": (129, (40, 40, 40, 120), (112,), 32, 5),
    "C": (40, (116, 50), (110, 110), 10, 2),
}
WHAT = ("out_loc", "out_sqerr", "out_rowdev")


def _eps(N, Z, seed=7):
    return torch.randn((N + 255) // 256, 256, Z, generator=torch.Generator().manual_seed(seed))


def _sub_exports(job, s):
    torch.cuda.synchronize()
    return [tuple(None if b[s][m] is None else b[s][m].cpu().clone() for b in (job.sub_loc, job.sub_sqerr, job.sub_rowdev))
            for m in range(len(job.kmods))]


def _multi_exports(job):
    torch.cuda.synchronize()
    return [(job.out_loc[m].cpu().clone(), job.out_sqerr[m].cpu().clone(), job.out_rowdev[m].cpu().clone())
            for m in range(len(job.kmods))]


def _fill(job, v=7.0):
    for bufs in (job.sub_loc, job.sub_sqerr, job.sub_rowdev):
        for row in bufs:
            for t in row:
                if t is not None:
                    t.fill_(v)


def _same(a, b, tag):
    """Bit for bit, NaN equal to NaN."""
    for m, (ea, eb) in enumerate(zip(a, b)):
        for ta, tb, what in zip(ea, eb, WHAT):
            assert torch.equal(torch.nan_to_num(ta, nan=-123.0), torch.nan_to_num(tb, nan=-123.0)), (tag, m, what)
            assert torch.equal(torch.isnan(ta), torch.isnan(tb)), (tag, m, what)


def _seven_with_full_at(M, pos):
    """Up to seven distinct subsets, the full one at `pos` (first / middle / last of the list)."""
    full = tuple(range(M))
    others = [s for s in S.all_subsets(M) if s != full][:6]
    at = {"first": 0, "middle": len(others) // 2, "last": len(others)}[pos]
    return others[:at] + [full] + others[at:], at


def _anchor(make_job, M, tag):
    """make_job() -> a fresh job on the case's tables: nm_devpass_multi's exports, then the full subset at three places."""
    ref = make_job()
    nm.JobSet([ref]).forward(loss=False, compact=True)
    want = _multi_exports(ref)
    N = ref.tables[0].N
    assert all(float(w[1][:N].abs().max()) > 0 for w in want)
    for pos in ("first", "middle", "last"):
        subsets, at = _seven_with_full_at(M, pos)
        job = make_job()
        job.enable_subset_exports(subsets)
        _fill(job)
        nm.JobSet([job]).forward_subsets()
        got = _sub_exports(job, at)
        for m in range(M):
            for a, b, what in zip(want[m], got[m], WHAT):
                assert torch.equal(a, b), (tag, pos, m, what, float((a - b).abs().max()))


@pytest.mark.parametrize("inject", [True, False], ids=["injected", "in-kernel"])
@pytest.mark.parametrize("combine", COMBINERS)
@pytest.mark.parametrize("shape", ["A", "B", "C"])
def test_full_subset_equals_devpass_multi_bit_for_bit(shape, combine, inject):
    N, dims, hidden, Z, cd = SHAPES[shape]
    xs, cs = _data(N, dims, cd, seed=21)
    tables = _tables(xs, cs)
    eps = _eps(N, Z) if inject else None
    _anchor(lambda: _job(tables, dims, hidden, Z, cd, combine, seed=11, eps=eps), len(dims), (shape, combine, inject))


@pytest.mark.parametrize("cs", list(T.FIXED["devpass_multi"]) + [T.draw("devpass_multi", s) for s in range(8)], ids=lambda cs: cs.id)
def test_full_subset_equals_devpass_multi_over_the_twin_cases(cs):
    b = built(cs)
    _anchor(lambda: b.job("mod"), cs.M, cs.id)


@pytest.mark.parametrize("shape,combine,inject", [("A", "gpoe", False), ("A", "mopoe", True), ("B", "gpoe", True), ("C", "moe", True)])
def test_every_subset_of_one_launch_equals_it_alone_and_lists_permute(shape, combine, inject):
    N, dims, hidden, Z, cd = SHAPES[shape]
    M = len(dims)
    xs, cs = _data(N, dims, cd, seed=3)
    tables = _tables(xs, cs)
    eps = _eps(N, Z, 5) if inject else None
    subs = S.all_subsets(M)

    def run(subsets):
        job = _job(tables, dims, hidden, Z, cd, combine, seed=17, eps=eps)
        job.enable_subset_exports(subsets)
        _fill(job)
        nm.JobSet([job]).forward_subsets()
        return [_sub_exports(job, s) for s in range(len(subsets))]

    together = run(subs)
    for s, sub in enumerate(subs):
        _same(run([sub])[0], together[s], (shape, "alone", sub))
    perm = torch.randperm(len(subs), generator=torch.Generator().manual_seed(1)).tolist()
    shuffled = run([subs[i] for i in perm])
    for k, i in enumerate(perm):
        _same(shuffled[k], together[i], (shape, "permuted", subs[i]))
    # the subsets are different posteriors under one draw: they differ, and none is all zeros
    assert not torch.equal(together[0][0][0], together[-1][0][0])
    assert all(float(t[0][0][:N].abs().max()) > 0 for t in together)


def test_twenty_models_in_one_launch_equal_each_alone():
    N, dims, hidden, Z, cd = SHAPES["A"]
    xs, cs = _data(N, dims, cd, seed=8)
    tables = _tables(xs, cs)
    subs = S.all_subsets(3)

    def make(j):
        job = _job(tables, dims, hidden, Z, cd, COMBINERS[j % 4], seed=100 + j)
        job.enable_subset_exports(subs[j % 7:] + subs[:j % 7])          # (every model its own order)
        _fill(job)
        return job

    jobs = [make(j) for j in range(20)]
    nm.JobSet(jobs).forward_subsets()
    together = [[_sub_exports(job, s) for s in range(7)] for job in jobs]
    for j in range(20):
        alone = make(j)
        nm.JobSet([alone]).forward_subsets()
        for s in range(7):
            _same(_sub_exports(alone, s), together[j][s], (j, s))


def _oracle_case(name):
    if name in ("A", "B"):
        N, dims, hidden, Z, cd = SHAPES[name]
        spec = nm.ModelSpec(list(dims), list(hidden), Z, cd, True, "multimodal")
        P = nm.ParamLayout(spec).init_reference_rule(31)
        g = torch.Generator().manual_seed(2)
        for m in range(len(dims)):                                   # distinct gPoE logits: the softmax over a subset matters
            P[f"alpha_m_list.{m}"] = torch.randn(P[f"alpha_m_list.{m}"].shape, generator=g)
        return N, tuple(dims), tuple(hidden), Z, cd, P
    g = Golden(name)                                                 # the goldens' own shapes and weights
    return 300, tuple(g.dims), tuple(g.hidden), g.Z, g.c_dim, dict(g.weights("w0"))


@pytest.mark.parametrize("name,combine", [("A", "gpoe"), ("A", "mopoe"), ("B", "gpoe"), ("mm3_gpoe", "gpoe"), ("mm4_uca_gpoe", "gpoe")])
def test_every_subset_matches_the_oracle(name, combine):
    """|got - bf16| <= 1.5 noise + 1e-5 and |got - fp32| <= 3 noise + 1e-5 per modality and subset, noise the distance
    between the oracle's two operand modes for that subset (the bounds of test_devpass_multi_matches_the_oracle); the
    per-subject means against the row sums at that test's rtol 2e-5."""
    N, dims, hidden, Z, cd, P = _oracle_case(name)
    M = len(dims)
    xs, cs = _data(N, dims, cd, seed=5)
    eps = _eps(N, Z, 9)
    subs = S.all_subsets(M)
    job = _job(_tables(xs, cs), dims, hidden, Z, cd, combine, seed=0, eps=eps, state=P)
    job.enable_subset_exports(subs)
    nm.JobSet([job]).forward_subsets()
    torch.cuda.synchronize()
    rs = R.Spec(list(dims), list(hidden), Z, cd)
    e = eps.reshape(-1, Z)[:N]
    out = {}
    for mode in ("fp32", "bf16"):
        R.set_operand_rounding(mode)
        try:
            res = S.forward_subsets(P, rs, xs, [c.long() for c in cs], combine, e, subs)
            out[mode] = [[(xs[m] - r["locs"][m]) ** 2 for m in range(M)] for r in res]
        finally:
            R.set_operand_rounding("fp32")
    fails = []
    for s, sub in enumerate(subs):
        for m in range(M):
            got = job.sub_sqerr[s][m][:N].cpu()
            noise = float((out["bf16"][s][m] - out["fp32"][s][m]).abs().max())
            db, df = float((got - out["bf16"][s][m]).abs().max()), float((got - out["fp32"][s][m]).abs().max())
            print(f"{name} {combine} subset {sub} modality {m}: |got - bf16| {db:.3e}  |got - fp32| {df:.3e}  noise {noise:.3e}")
            if not (db <= 1.5 * noise + 1e-5 and df <= 3.0 * noise + 1e-5):
                fails.append((sub, m, db, df, noise))
            np.testing.assert_allclose(job.sub_rowdev[s][m][:N].cpu().numpy(), got.sum(1).numpy() / dims[m], rtol=2e-5, atol=1e-7)
    assert not fails, fails


@pytest.mark.parametrize("shape,combine,inject", [("A", "gpoe", True), ("A", "mopoe", False), ("B", "gpoe", False),
                                                  ("B", "moe", True), ("C", "poe", True)])
def test_presence_bits_select_the_experts_row_by_row(shape, combine, inject):
    """Rows with present = p under the full mask equal the same rows under mask p without presence bytes; a row with nothing
    observed is NaN in every export (columns < D); out_sqerr / out_rowdev of an unobserved modality are NaN, its out_loc
    finite; pad columns and rows past the table are 0 -- all from buffers that held 7.0."""
    N, dims, hidden, Z, cd = SHAPES[shape]
    M = len(dims)
    xs, cs = _data(N, dims, cd, seed=12)
    tables = _tables(xs, cs)
    eps = _eps(N, Z, 4) if inject else None
    g = torch.Generator().manual_seed(6)
    present = (torch.arange(N) % (1 << M))[torch.randperm(N, generator=g)]      # every value 0 .. 2^M - 1, in any row
    full = tuple(range(M))
    job = _job(tables, dims, hidden, Z, cd, combine, seed=9, eps=eps)
    job.enable_subset_exports([full, (0,)])
    _fill(job)
    nm.JobSet([job]).forward_subsets(present=[[present.numpy(), None]])
    got = _sub_exports(job, 0)
    plain = _sub_exports(job, 1)                                     # (the entry beside it has no presence bytes: no NaN)
    assert all(bool(torch.isfinite(t).all()) for e in plain for t in e)
    subs = S.all_subsets(M)
    ref = _job(tables, dims, hidden, Z, cd, combine, seed=9, eps=eps)
    ref.enable_subset_exports(subs)
    nm.JobSet([ref]).forward_subsets()
    for s, sub in enumerate(subs):
        p = S.mask_of(sub)
        rows = (present == p).nonzero().flatten()
        assert rows.numel() > 0
        want = _sub_exports(ref, s)
        for m in range(M):
            assert torch.equal(got[m][0][rows], want[m][0][rows]), (sub, m, "out_loc")
            assert bool(torch.isfinite(got[m][0][rows]).all())
            if (p >> m) & 1:
                assert torch.equal(got[m][1][rows], want[m][1][rows]), (sub, m, "out_sqerr")
                assert torch.equal(got[m][2][rows], want[m][2][rows]), (sub, m, "out_rowdev")
            else:
                assert bool(torch.isnan(got[m][1][rows]).all()) and bool(torch.isnan(got[m][2][rows]).all()), (sub, m)
    none = (present == 0).nonzero().flatten()
    assert none.numel() > 0
    for m in range(M):
        for k in range(3):
            assert bool(torch.isnan(got[m][k][none]).all()), (m, WHAT[k])
        # pad columns (the storage behind the [rows, D] view) and rows past the table: zeros
        for bufs in (job.sub_loc, job.sub_sqerr):
            store = bufs[0][m]
            pitch = tables[m].x_pitch
            whole = torch.as_strided(store, (store.shape[0], pitch), (pitch, 1)).cpu()
            assert float(whole[:, dims[m]:].abs().max() if pitch > dims[m] else 0.0) == 0.0, m
            assert float(whole[N:].abs().max()) == 0.0, m
        assert float(job.sub_rowdev[0][m][N:].abs().max()) == 0.0, m


def test_skipped_decoders_leave_their_buffers_alone():
    """decoders=[(m,)] per subset ("predict m from the rest" costs one decoder): what is written equals the all-decoders run,
    what is not asked for does not exist, and an entry's buffers of another entry's decoder keep their fill."""
    N, dims, hidden, Z, cd = SHAPES["A"]
    xs, cs = _data(N, dims, cd, seed=14)
    tables = _tables(xs, cs)
    subs = [(1, 2), (0, 2), (0, 1)]                                  # leave one out ...
    job = _job(tables, dims, hidden, Z, cd, "gpoe", seed=3)
    job.enable_subset_exports(subs)
    nm.JobSet([job]).forward_subsets()
    want = [_sub_exports(job, s) for s in range(3)]
    one = _job(tables, dims, hidden, Z, cd, "gpoe", seed=3)
    one.enable_subset_exports(subs, decoders=[(0,), (1,), (2,)])     # ... and predict it
    _fill(one)
    assert all((one.sub_loc[s][m] is not None) == (s == m) for s in range(3) for m in range(3))
    nm.JobSet([one]).forward_subsets()
    got = [_sub_exports(one, s) for s in range(3)]
    for s in range(3):
        for a, b, what in zip(want[s][s], got[s][s], WHAT):
            assert torch.equal(a, b), (s, what)
    # the same table over buffers that exist but are not named in it: they keep their fill
    kept = _job(tables, dims, hidden, Z, cd, "gpoe", seed=3)
    kept.enable_subset_exports(subs)
    _fill(kept)
    named = kept.subset_structs

    def own_decoder_only(present=None):
        entries = named(present)
        for s, e in enumerate(entries):
            for m in range(3):
                if m != s:
                    e.out_loc[m] = e.out_sqerr[m] = e.out_rowdev[m] = None
        return entries

    kept.subset_structs = own_decoder_only
    nm.JobSet([kept]).forward_subsets()
    got = [_sub_exports(kept, s) for s in range(3)]
    for s in range(3):
        for m in range(3):
            for a, b, what in zip(want[s][m], got[s][m], WHAT):
                if m == s:
                    assert torch.equal(a, b), (s, m, what)
                else:
                    assert float((b - 7.0).abs().max()) == 0.0, (s, m, what)
    # the same run with only out_rowdev asked for: out_loc / out_sqerr do not exist, out_rowdev is the same
    rd = _job(tables, dims, hidden, Z, cd, "gpoe", seed=3)
    rd.enable_subset_exports(subs, loc=False, sqerr=False, decoders=[(0,), (1,), (2,)])
    _fill(rd)
    nm.JobSet([rd]).forward_subsets()
    torch.cuda.synchronize()
    for s in range(3):
        assert rd.sub_loc[s][s] is None and rd.sub_sqerr[s][s] is None
        assert torch.equal(rd.sub_rowdev[s][s].cpu(), want[s][s][2]), s


@pytest.mark.parametrize("why,hidden,Z,kind,extra", [
    ("hidden 120", (120, 48), 12, "multimodal", ()),
    ("latent 40", (64, 48), 40, "multimodal", ()),
    ("endtoend trunk", (64, 48), 12, "endtoend", ((32, 16), 2)),
])
def test_refused_jobs_raise_naming_the_refusal(why, hidden, Z, kind, extra):
    N, dims, cd = 200, (61, 90, 47), 3
    xs, cs = _data(N, dims, cd, seed=13)
    job = _job(_tables(xs, cs), dims, hidden, Z, cd, "poe", seed=6, kind=kind, extra=extra)
    job.enable_subset_exports([(0,), (0, 1)])
    with pytest.raises(ValueError, match="nm_devpass_subsets_ok refuses"):
        nm.JobSet([job]).forward_subsets()


@pytest.mark.parametrize("cls", ["cVAE_multimodal", "mmJSD", "cVAE_multimodal_regression"])
def test_pred_recon_given_with_the_full_subset_is_pred_recon(cls):
    import pandas as pd
    N, dims, cd = 200, (61, 90, 47), 3
    xs, cs = _data(N, dims, cd, seed=17)
    model = getattr(nm, cls)(list(dims), [64, 48], 12, cd, modalities=3, non_linear=True)
    model.to(DEV)
    frames = [pd.DataFrame(x.numpy()) for x in xs]
    c = cs[0].long().numpy()
    torch.manual_seed(5)
    want = (model.pred_recon if hasattr(model, "pred_recon") else
            lambda *a: nm.cVAE_multimodal.pred_recon(model, *a))(frames, c, DEV, "gpoe")
    torch.manual_seed(5)
    got = model.pred_recon_given(frames, c, DEV, "gpoe", [(0,), (0, 1, 2), (1, 2)])
    assert len(got) == 3 and all(len(g) == 3 for g in got)
    for m in range(3):
        assert np.array_equal(got[1][m], want[m]), m
        assert got[0][m].shape == (N, dims[m]) and np.isfinite(got[0][m]).all()
        assert not np.array_equal(got[0][m], want[m]) and not np.array_equal(got[2][m], got[0][m])
    # a subject without modality 0: under (0,) nothing is left (NaN), under (0, 1, 2) it is imputed from the other two
    present = np.full(N, 7)
    present[:10] = 6
    torch.manual_seed(5)
    pres = model.pred_recon_given(frames, c, DEV, "gpoe", [(0,), (0, 1, 2), (1, 2)], present=present)
    assert np.isnan(pres[0][0][:10]).all() and np.isfinite(pres[0][0][10:]).all()
    for m in range(3):
        assert np.array_equal(pres[1][m][:10], got[2][m][:10]), m      # present = {1, 2} under the full set = the set (1, 2)
        assert np.array_equal(pres[1][m][10:], got[1][m][10:]), m
