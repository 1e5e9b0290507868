"""Input preparation on the device (csrc/nm_prep.hip) against prep.py (itself pinned to sklearn / pandas in
tests/test_prep_cpu.py): bit-exact scaler statistics, one-hot covariates and packed tables."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import multi_modal_normative_modeling_amd as nm
from multi_modal_normative_modeling_amd import prep
from multi_modal_normative_modeling_amd.prep_device import DeviceCohort
from tests import pack_ref as PR

DEV = "cuda:0"


@pytest.mark.parametrize("n,d", [(1280, 379), (333, 41)])
def test_fold_tables_from_the_raw_cohort_bit_exact(n, d):
    cohort = prep.synthetic_cohort(n=n, d=d, seed=7 + n)
    # ties and a constant column: the rank / IQR edge cases
    cohort.x["T1w_sMRI"][:, 3] = 2.5
    cohort.x["fMRI"][::3, 5] = cohort.x["fMRI"][0, 5]
    dc = DeviceCohort(cohort, DEV)
    folds = prep.kfold_indices(n, 5, 42)
    for k in (0, 3):
        tr = folds[k][0]
        rows = torch.as_tensor(tr.astype(np.int32)).to(DEV)
        mods = list(prep.HCP_MODALITIES) + [prep.EARLY_FUSION]
        xs, c = prep.fold_train_tables(cohort, mods, tr)
        c_dev = dc.one_hot(rows)
        assert torch.equal(c_dev.cpu(), torch.from_numpy(c)), k
        for m, x_host in zip(mods, xs):
            src = cohort.x[m] if m in cohort.x else prep.early_fusion(cohort.x, prep.HCP_MODALITIES)
            center, scale = prep.robust_scaler_fit(src[tr])
            cd, sd = dc.scaler_fit(m, rows)
            assert np.array_equal(cd.cpu().numpy(), center) and np.array_equal(sd.cpu().numpy(), scale), (k, m)
        host = [nm.Table(x, c, DEV) for x in xs]
        dev = dc.fold_tables(mods, tr)
        for m, th, td in zip(mods, host, dev):
            assert (th.N, th.D, th.C, th.Kx, th.rows_alloc, th.x_pitch, th.Cz) == (td.N, td.D, td.C, td.Kx, td.rows_alloc, td.x_pitch, td.Cz)
            assert torch.equal(th.x_f32, td.x_f32), (k, m)
            assert torch.equal(th.xb.view(torch.int16), td.xb.view(torch.int16)), (k, m)
            assert torch.equal(th.cz.view(torch.int16), td.cz.view(torch.int16)), (k, m)


def test_training_from_device_built_tables_equals_host_built():
    """The same model trained three steps on host-built and on device-built tables ends bit-identical."""
    cohort = prep.synthetic_cohort(n=640, d=379)
    tr = prep.kfold_indices(640, 5, 42)[1][0]
    xs, c = prep.fold_train_tables(cohort, prep.HCP_MODALITIES, tr)
    spec = nm.ModelSpec([379] * 3, [110, 110], 10, 29)
    out = []
    for tabs in ([nm.Table(x, c, DEV) for x in xs], DeviceCohort(cohort, DEV).fold_tables(prep.HCP_MODALITIES, tr)):
        job = nm.Job(spec, tabs, combine="gpoe", seed=3, init_seed=11)
        nm.JobSet([job]).train(3)
        torch.cuda.synchronize()
        out.append(job.params.cpu().clone())
    assert torch.equal(out[0], out[1])


def test_prep_argument_errors():
    lib = nm._lib.load()
    assert lib.nm_prep_scaler_fit(None, None, 1, 1, None, 1, None, None, None) == nm._lib.NM_E_NULL
    dc = DeviceCohort(prep.synthetic_cohort(n=64, d=8), DEV)
    ptrs, widths, n_src, D, keep = dc._sources("fMRI")
    rows = torch.zeros(9000, dtype=torch.int32, device=DEV)
    out = torch.empty(D, dtype=torch.float64, device=DEV)
    assert lib.nm_prep_scaler_fit(ptrs.data_ptr(), widths.data_ptr(), n_src, D, rows.data_ptr(), 9000, out.data_ptr(),
                                  out.data_ptr(), None) == nm._lib.NM_E_PREP


# ---- the three kernels at their sizes and edges --------------------------------------------------------------------------
# (everything below compares with prep.py on the same rows, which tests/test_prep_cpu.py holds to sklearn / pandas at the
# same sizes; every comparison is exact)

def _plain_cohort(x, age=None, gender=None, resource="HCPimage", seed=0):
    n = next(iter(x.values())).shape[0]
    rng = np.random.default_rng(seed)
    age = rng.integers(22, 37, size=n).astype(np.float64) if age is None else np.asarray(age, dtype=np.float64)
    gender = rng.integers(0, 2, size=n).astype(np.float64) if gender is None else np.asarray(gender, dtype=np.float64)
    return prep.SyntheticCohort(iid=np.arange(100001, 100001 + n, dtype=np.int64), age=age, gender=gender,
                                dia=np.ones(n, dtype=np.int64), fi=np.zeros(n), x=x, resource=resource)


def _dev_rows(rows):
    return torch.as_tensor(np.asarray(rows, dtype=np.int32)).to(DEV)


def _scaler_columns(n_all, rng):
    """The seven columns of a scaler case: continuous, rounded to integers (heavy ties), resampled with replacement from
    itself, constant (IQR 0 -> scale 1), scaled by 1e-300, scaled by 1e300 (no overflow), all negative.  No -0.0: which
    zero numpy's median returns over both is not defined."""
    base = rng.standard_normal(n_all) * 3.0 + 0.5
    ints = np.rint(rng.standard_normal(n_all) * 2.0) + 0.0
    cols = [base, ints, rng.choice(base, size=n_all, replace=True), np.full(n_all, 2.5), rng.standard_normal(n_all) * 1e-300,
            rng.standard_normal(n_all) * 1e300, -np.abs(rng.standard_normal(n_all)) - 1e-3]
    x = np.stack(cols, axis=1)
    assert not (np.signbit(x) & (x == 0)).any() and np.isfinite(x).all()
    return x


SCALER_N = (1, 2, 3, 4, 5, 7, 8, 9, 255, 256, 257, 1023, 1024, 1025, 4096, 4097, 8191, 8192)


@pytest.mark.parametrize("n", SCALER_N)
def test_scaler_fit_at_its_sizes(n):
    """n rows drawn four ways (ascending, permuted, a bootstrap draw with duplicates, one cohort row n times) from a
    cohort a little larger than n, two modalities of seven columns and their early fusion.  From 4097 rows the launch
    asks for 64 KiB of dynamic LDS."""
    rng = np.random.default_rng(9000 + n)
    n_all = n + 3
    cohort = _plain_cohort({"fMRI": _scaler_columns(n_all, rng), "T1w_sMRI": _scaler_columns(n_all, rng)[:, ::-1].copy()})
    dc = DeviceCohort(cohort, DEV)
    asc = np.sort(rng.choice(n_all, size=n, replace=False))
    boot = prep.rows_of_ids(cohort.iid, rng.choice(cohort.iid, size=n, replace=True))
    assert len(boot) == n and (n < 4 or len(np.unique(boot)) < n)
    for kind, rows in (("ascending", asc), ("permuted", rng.permutation(asc)), ("bootstrap", boot),
                       ("one row", np.full(n, int(rng.integers(0, n_all))))):
        rd = _dev_rows(rows)
        for m in ("fMRI", "T1w_sMRI", cohort.fusion_name):
            center, scale = prep.robust_scaler_fit(prep.source_table(cohort, m)[rows])
            cd, sd = dc.scaler_fit(m, rd)
            assert np.array_equal(cd.cpu().numpy(), center), (kind, m)
            assert np.array_equal(sd.cpu().numpy(), scale), (kind, m)


def test_scaler_fit_refuses_more_rows_than_it_sorts():
    lib = nm._lib.load()
    dc = DeviceCohort(_plain_cohort({"fMRI": np.zeros((4, 7))}), DEV)
    ptrs, widths, n_src, D, keep = dc._sources("fMRI")
    rows = torch.zeros(8193, dtype=torch.int32, device=DEV)
    out = torch.empty(D, dtype=torch.float64, device=DEV)
    assert lib.nm_prep_scaler_fit(ptrs.data_ptr(), widths.data_ptr(), n_src, D, rows.data_ptr(), 8193, out.data_ptr(),
                                  out.data_ptr(), None) == nm._lib.NM_E_PREP
    assert lib.nm_prep_onehot(dc.age.data_ptr(), dc.gender.data_ptr(), rows.data_ptr(), 8193, dc.edges(8193, 27).data_ptr(), 27,
                              dc.edges(8193, 2).data_ptr(), 2, out.data_ptr(), None) == nm._lib.NM_E_PREP


def _onehot_case(n, rows, age, gender):
    """one_hot on the device against prep.one_hot_covariates of the same rows; the output buffer's every element is written."""
    cohort = _plain_cohort({"fMRI": np.zeros((len(age), 1))}, age=age, gender=gender)
    dc = DeviceCohort(cohort, DEV)
    want = torch.from_numpy(prep.one_hot_covariates(cohort.age[rows], cohort.gender[rows]))
    got = dc.one_hot(_dev_rows(rows)).cpu()
    assert got.shape == (n, 29) and not torch.isnan(got).any()
    assert torch.equal(got, want)


def _onehot_inputs(n, seed=0):
    rng = np.random.default_rng(500 + n + seed)
    n_all = n + 3
    return rng, n_all, rng.integers(22, 37, size=n_all).astype(np.float64), rng.integers(0, 2, size=n_all).astype(np.float64)


ONEHOT_N = (1, 2, 5, 26, 27, 28, 257, 4096)


@pytest.mark.parametrize("n", ONEHOT_N)
def test_onehot_at_its_edges(n):
    """27 age bins over n rows: below 27 rows some bins stay empty; at n = 1 all 28 edges are 1.0.  Rows ascending, permuted
    and with duplicate ids (ties are broken by the position in `rows`, not by the cohort row)."""
    rng, n_all, age, gender = _onehot_inputs(n)
    edges = prep.qcut_edges(n, 27)
    assert (np.diff(edges) > 0).all() if n >= 2 else (edges == 1.0).all()
    asc = np.sort(rng.choice(n_all, size=n, replace=False))
    dup = rng.integers(0, max(1, n_all // 2), size=n)                      # unsorted, with repeats
    for rows in (asc, rng.permutation(asc), dup, prep.rows_of_ids(np.arange(n_all), rng.choice(n_all, size=n, replace=True))):
        _onehot_case(n, rows, age, gender)
    # ages all distinct and descending in cohort order: the rank is decided by the values alone
    _onehot_case(n, rng.permutation(asc), np.arange(n_all, 0, -1) + 0.5, gender)


@pytest.mark.parametrize("n", ONEHOT_N)
def test_onehot_constant_age(n):
    """One AGE throughout: every rank is a tie, the bins follow the position in `rows`."""
    rng, n_all, age, gender = _onehot_inputs(n, 1)
    _onehot_case(n, rng.integers(0, n_all, size=n), np.full(n_all, 31.0), gender)


@pytest.mark.parametrize("n", (2, 5, 28, 257, 4096))
def test_onehot_signed_zero_gender(n):
    """PTGENDER coded 0.0 / -0.0: pandas ranks the two zeros as a tie broken by position (prep.qcut_rank_bins([0., -0., 0.,
    -0.], 2) = [0 0 1 1]); a sort that puts -0.0 first gives [1 0 1 0]."""
    rng, n_all, age, gender = _onehot_inputs(n, 2)
    gender = np.where(np.arange(n_all) % 2 == 1, -0.0, 0.0)
    assert np.array_equal(prep.qcut_rank_bins(np.array([0.0, -0.0, 0.0, -0.0]), 2), [0, 0, 1, 1])
    _onehot_case(n, np.sort(rng.choice(n_all, size=n, replace=False)), age, gender)
    age[::3] = -0.0                                                     # and the same in AGE, among other values
    age[1::3] = 0.0
    _onehot_case(n, rng.integers(0, n_all, size=n), age, gender)


@pytest.mark.parametrize("n", (4097, 8192))
def test_onehot_above_the_default_lds_limit(n):
    """From 4097 rows the kernel asks for 96 KiB of dynamic LDS (12 bytes per padded row), above the 64 KiB a launch gets
    without raising the kernel's limit first."""
    rng, n_all, age, gender = _onehot_inputs(n)
    _onehot_case(n, np.sort(rng.choice(n_all, size=n, replace=False)), age, gender)
    _onehot_case(n, rng.integers(0, n_all, size=n), age, gender)


# ---- cohort shapes the sweep really uses --------------------------------------------------------------------------------

def _assert_tables_equal(host, dev, what):
    for i, (th, td) in enumerate(zip(host, dev)):
        assert (th.N, th.D, th.C, th.Kx, th.rows_alloc, th.x_pitch, th.Cz) == (td.N, td.D, td.C, td.Kx, td.rows_alloc, td.x_pitch, td.Cz), (what, i)
        assert torch.equal(th.x_f32.view(torch.int32), td.x_f32.view(torch.int32)), (what, i)
        assert torch.equal(th.xb.view(torch.int16), td.xb.view(torch.int16)), (what, i)
        assert torch.equal(th.cz.view(torch.int16), td.cz.view(torch.int16)), (what, i)


def _assert_plain_layout(t, x, c):
    """A device-built table against tests/pack_ref.py: the three buffers bit for bit, and packed_rows() = x | c | 1 | 0."""
    u16 = lambda b: b.view(torch.int16).cpu().numpy().view(np.uint16)
    assert PR.compare_packed(u16(t.xb), t.x_f32.cpu().numpy(), u16(t.cz), x, c) == []
    want = np.zeros((t.rows_alloc, t.Kx), dtype=np.float32)
    want[:t.N, :t.D], want[:t.N, t.D:t.D + t.C], want[:t.N, t.D + t.C] = x, c, 1.0
    assert np.array_equal(u16(t.packed_rows().contiguous()), PR.bf16_rne(want))


def _adni_like(n, seed=5):
    """Three modalities of different widths (as ADNI's av45 / vbm / fdg are), built by hand."""
    rng = np.random.default_rng(seed)
    x = {m: rng.standard_normal((n, w)) * rng.lognormal(0.0, 0.5, size=w) + rng.normal(0.0, 2.0, size=w)
         for m, w in zip(prep.DATASET_MODALITIES["ADNI"], (5, 70, 33))}
    return _plain_cohort(x, resource="ADNI", seed=seed)


def test_modalities_of_different_widths_and_their_fusion():
    cohort = _adni_like(300)
    fusion = cohort.fusion_name
    assert fusion == prep.FUSION_PREFIX + "ADNI"
    mods = cohort.modalities + [fusion]
    dc = DeviceCohort(cohort, DEV)
    tr = prep.kfold_indices(300, 5, 42)[2][0]
    rd = _dev_rows(tr)
    fused = prep.early_fusion(cohort.x, cohort.modalities)
    assert fused.shape == (300, 108) and np.array_equal(fused[:, 5:75], cohort.x["vbm"])
    fc, fs = prep.robust_scaler_fit(fused[tr])
    cd, sd = dc.scaler_fit(fusion, rd)
    assert np.array_equal(cd.cpu().numpy(), fc) and np.array_equal(sd.cpu().numpy(), fs)
    for m in cohort.modalities:
        center, scale = prep.robust_scaler_fit(cohort.x[m][tr])
        cd, sd = dc.scaler_fit(m, rd)
        assert np.array_equal(cd.cpu().numpy(), center) and np.array_equal(sd.cpu().numpy(), scale), m
    xs, c = prep.fold_train_tables(cohort, mods, tr)
    assert [x.shape[1] for x in xs] == [5, 70, 33, 108]
    assert np.array_equal(xs[3], ((fused[tr] - fc) / fs).astype(np.float32))
    dev = dc.fold_tables(mods, tr)
    _assert_tables_equal([nm.Table(x, c, DEV) for x in xs], dev, "widths")
    for x, td in zip(xs, dev):                                          # and against the plain layout, not only the other kernel
        _assert_plain_layout(td, x, c)


def test_bootstrap_train_rows_with_duplicates():
    """The train rows of the real path: generate_kfold_ids' bootstrap draw (1.5 x oversampled), rows_of_ids of it."""
    cohort = _adni_like(83, seed=6)
    ids = prep.generate_kfold_ids(cohort.iid[:57], cohort.iid[57:], oversample_percentage=1.5)[0][0]
    tr = prep.rows_of_ids(cohort.iid, ids)
    assert len(tr) == 99 and len(np.unique(tr)) == 51
    mods = cohort.modalities + [cohort.fusion_name]
    xs, c = prep.fold_train_tables(cohort, mods, tr)
    dc = DeviceCohort(cohort, DEV)
    assert torch.equal(dc.one_hot(_dev_rows(tr)).cpu(), torch.from_numpy(c))
    dev = dc.fold_tables(mods, tr)
    _assert_tables_equal([nm.Table(x, c, DEV) for x in xs], dev, "bootstrap")
    for x, td in zip(xs, dev):
        _assert_plain_layout(td, x, c)


def test_cached_fold_tables_with_and_without_covariates():
    cohort = _adni_like(300, seed=7)
    mods = cohort.modalities + [cohort.fusion_name]
    tr = prep.kfold_indices(300, 5, 42)[0][0]
    xs, c = prep.fold_train_tables(cohort, mods, tr)
    dc = DeviceCohort(cohort, DEV)
    bare = dc.fold_tables_cached("fold0", mods, tr, with_covariates=False)
    assert [t.C for t in bare] == [0] * 4 and [t.Kx for t in bare] == [32, 96, 64, 128]
    _assert_tables_equal([nm.Table(x, np.zeros((len(tr), 0), dtype=np.float32), DEV) for x in xs], bare, "no covariates")
    for x, td in zip(xs, bare):
        _assert_plain_layout(td, x, np.zeros((len(tr), 0), dtype=np.float32))
    full = dc.fold_tables_cached("fold0", mods, tr, with_covariates=True)      # same key, made afterwards
    _assert_tables_equal(dc.fold_tables(mods, tr), full, "cached")
    _assert_tables_equal([nm.Table(x, c, DEV) for x in xs], full, "cached against host")
    for again, first in ((dc.fold_tables_cached("fold0", mods, tr, with_covariates=True), full),
                         (dc.fold_tables_cached("fold0", mods, tr, with_covariates=False), bare)):
        assert all(a is b for a, b in zip(again, first))
    assert all(a is not b for a, b in zip(full, bare))
