"""Input preparation on the device (csrc/nm_prep.hip) against prep.py (itself pinned to sklearn / pandas in
tests/test_prep_cpu.py): bit-exact scaler statistics, one-hot covariates and packed tables."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import multi_modal_normative_modeling_amd as nm
from multi_modal_normative_modeling_amd import prep
from multi_modal_normative_modeling_amd.prep_device import DeviceCohort

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
