"""The compact deviation-pass kernel for models with several experts (nm_devpass_multi: 128-row tiles, two workgroups
per CU, the experts' statistics through the batch's workspace tile) against the general forward-only kernel (nm_forward),
which tests/test_gpu_parity.py and tests/test_gpu_fullsize.py hold to the oracle: row by row the two run the same
arithmetic with the same draws and fuse the experts through the same code, so out_loc and out_sqerr of EVERY modality must
agree bit for bit at every shape the compact kernel admits (out_rowdev to fp32 summation order: the general kernel adds the
four column-group sums of a row in arrival order); directly against the oracle; many models in one launch; the shapes it
refuses; and sweep.test_folds (all folds of a procedure in one launch) against sweep.test_fold.
Reference: multimodal_kfold_test_cvae_supervised.py:64-153 (pred_recon with the joint latent, then
reconstruction_deviation_multimodal)."""
import filecmp
import tempfile
from pathlib import Path

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import multi_modal_normative_modeling_amd as nm
from multi_modal_normative_modeling_amd import prep, sweep
from oracle import cvae_ref as R
from tests.golden_util import Golden

DEV = "cuda:0"


def _data(N, dims, c_dim, seed, own_cov=False):
    g = torch.Generator().manual_seed(seed)
    xs = [torch.randn(N, d, generator=g) * 1.1 for d in dims]
    cs = []
    for _ in range(len(dims) if own_cov else 1):
        c = torch.zeros(N, c_dim)
        c[torch.arange(N), torch.randint(0, c_dim, (N,), generator=g)] = 1
        cs.append(c)
    return xs, (cs if own_cov else cs * len(dims))


def _tables(xs, cs):
    return [nm.Table(x, c, DEV) for x, c in zip(xs, cs)]


def _job(tables, dims, hidden, Z, c_dim, combine, seed, eps=None, state=None, kind="multimodal", latent=False, extra=()):
    spec = nm.ModelSpec(list(dims), list(hidden), Z, c_dim, True, kind, *extra)
    job = nm.Job(spec, tables, combine=combine, state=state, seed=seed, init_seed=seed, n_tiles_ws=tables[0].n_tiles,
                 **({"single_bypass": False} if kind == "endtoend" else {}))
    if eps is not None:
        job.set_eps(eps)
    job.enable_exports(loc=True, sqerr=True, rowdev=True, latent=latent)
    return job


def _exports(job):
    torch.cuda.synchronize()
    return [(job.out_loc[m].cpu().clone(), job.out_sqerr[m].cpu().clone(), job.out_rowdev[m].cpu().clone())
            for m in range(len(job.kmods))]


CASES = [
    # N, D per modality, hidden, Z, c_dim, combine, injected eps, own covariates per modality
    (300, (61, 90, 47), (64, 48), 12, 3, "poe", True, False),     # two full 128-row tiles, a 44-row one, an empty half
    (300, (61, 90, 47), (64, 48), 12, 3, "gpoe", True, False),
    (300, (61, 90, 47), (64, 48), 12, 3, "moe", True, False),
    (300, (61, 90, 47), (64, 48), 12, 3, "mopoe", True, False),
    (300, (61, 90, 47), (64, 48), 12, 3, "gpoe", False, False),   # in-kernel draws
    (129, (40, 40, 40, 120), (112,), 32, 5, "gpoe", True, False), # four experts, width and latent at the limits, one row in tile 2
    (40, (116, 50), (110, 110), 10, 2, "poe", True, False),       # fewer rows than one tile; Z not a multiple of 4
    (517, (379, 379, 379), (110, 110), 10, 29, "gpoe", False, False),   # the SE shape over three 256-row batches
    (300, (61, 90, 47), (64, 48), 12, 3, "mopoe", False, True),   # every modality its own covariates: no shared z | c | 1
]


@pytest.mark.parametrize("N,dims,hidden,Z,c_dim,combine,inject,own_cov", CASES)
def test_devpass_multi_equals_general_forward_bit_for_bit(N, dims, hidden, Z, c_dim, combine, inject, own_cov):
    nt = (N + 255) // 256
    eps = torch.randn(nt, 256, Z, generator=torch.Generator().manual_seed(7)) if inject else None
    xs, cs = _data(N, dims, c_dim, seed=21, own_cov=own_cov)
    tables = _tables(xs, cs)
    res = []
    for compact in (False, True):
        job = _job(tables, dims, hidden, Z, c_dim, combine, seed=11, eps=eps)
        js = nm.JobSet([job])
        assert js.devpass_multi_ok() and not js.devpass_ok()
        js.forward(loss=not compact, compact=compact or None)
        res.append(_exports(job))
    for m in range(len(dims)):
        (loc_g, sq_g, rd_g), (loc_c, sq_c, rd_c) = res[0][m], res[1][m]
        assert torch.equal(loc_g, loc_c), (m, "out_loc", float((loc_g - loc_c).abs().max()))
        assert torch.equal(sq_g, sq_c), (m, "out_sqerr", float((sq_g - sq_c).abs().max()))
        assert torch.allclose(rd_g, rd_c, rtol=2e-6, atol=1e-9), (m, "out_rowdev", float((rd_g - rd_c).abs().max()))
        assert float(sq_c[:N].abs().max()) > 0 and float(loc_c[:N].abs().max()) > 0
        if sq_c.shape[0] > N:                                        # rows past the table: zeros in every modality
            assert float(sq_c[N:].abs().max()) == 0.0 and float(loc_c[N:].abs().max()) == 0.0
            assert float(rd_c[N:].abs().max()) == 0.0


def test_empty_half_tile_is_zeroed_in_every_modality():
    """300 rows: the 128-row tile [384, 512) holds no row -- its export rows must come back as zeros in EVERY modality, also
    when the buffers held something else before the launch (the general kernel stores the whole 256-row batch).  (Dead
    16-row tiles inside a live 128-row tile, rows 304..383 here, are skipped in every phase, as in nm_devpass; their export
    rows are zeroed once the output phase is through -- tests/test_gpu_twins.py looks at every row past the table.)"""
    N, dims = 300, (61, 90, 47)
    xs, cs = _data(N, dims, 3, seed=2)
    job = _job(_tables(xs, cs), dims, (64, 48), 12, 3, "gpoe", seed=4)
    for m in range(3):
        job.out_loc[m].fill_(7.0)
        job.out_sqerr[m].fill_(7.0)
    nm.JobSet([job]).forward(loss=False, compact=True)
    torch.cuda.synchronize()
    for m in range(3):
        assert float(job.out_loc[m][384:].abs().max()) == 0.0, m
        assert float(job.out_sqerr[m][384:].abs().max()) == 0.0, m
        assert float(job.out_loc[m][N:304].abs().max()) == 0.0, m         # the ragged tile's live 16-row tiles: masked rows
        assert float(job.out_sqerr[m][N:304].abs().max()) == 0.0, m


@pytest.mark.parametrize("name", ["mm3_gpoe", "mm4_uca_gpoe"])
def test_devpass_multi_matches_the_oracle(name):
    """The goldens' weights on 300 fresh rows with an injected draw, against the oracle in fp32 and bf16 operand modes: the
    squared residuals within the distance between the two (the bound of the general kernel's own test), the per-subject
    means consistent with the matrix."""
    g = Golden(name)
    N, M = 300, g.M
    xs, cs = _data(N, g.dims, g.c_dim, seed=5)
    eps = torch.randn(2, 256, g.Z, generator=torch.Generator().manual_seed(9))
    P = {k: v for k, v in g.weights("w0").items()}
    job = _job(_tables(xs, cs), g.dims, g.hidden, g.Z, g.c_dim, g.combine, seed=0, eps=eps, state=P)
    js = nm.JobSet([job])
    assert js.devpass_multi_ok()
    js.forward(loss=False, compact=True)
    torch.cuda.synchronize()
    rs = R.Spec(g.dims, g.hidden, g.Z, g.c_dim)
    e = eps.reshape(-1, g.Z)[:N]
    out = {}
    for mode in ("fp32", "bf16"):
        R.set_operand_rounding(mode)
        try:
            locs = R.forward_multimodal(P, rs, xs, [c.long() for c in cs], g.combine, e)["locs"]
            out[mode] = [(xs[m] - locs[m].detach()) ** 2 for m in range(M)]
        finally:
            R.set_operand_rounding("fp32")
    for m in range(M):
        got = job.out_sqerr[m][:N].cpu()
        noise = float((out["bf16"][m] - out["fp32"][m]).abs().max())
        print(f"{name} modality {m}: |got - bf16| {float((got - out['bf16'][m]).abs().max()):.3e}  "
              f"|got - fp32| {float((got - out['fp32'][m]).abs().max()):.3e}  noise {noise:.3e}")
        assert float((got - out["bf16"][m]).abs().max()) <= 1.5 * noise + 1e-5, m
        assert float((got - out["fp32"][m]).abs().max()) <= 3.0 * noise + 1e-5, m
        np.testing.assert_allclose(job.out_rowdev[m][:N].cpu().numpy(), got.sum(1).numpy() / g.dims[m], rtol=2e-5, atol=1e-7)


def test_twenty_models_in_one_launch_equal_each_alone():
    """20 three-expert models over shared 300-row tables in one launch: every model's exports bit-identical to that model
    run alone (its workspace tiles are its own; a tile's two workgroups touch disjoint rows)."""
    N, dims, hidden, Z, cd = 300, (61, 90, 47), (64, 48), 12, 3
    xs, cs = _data(N, dims, cd, seed=8)
    tables = _tables(xs, cs)
    jobs = [_job(tables, dims, hidden, Z, cd, ("gpoe", "poe", "moe", "mopoe")[j % 4], seed=100 + j) for j in range(20)]
    js = nm.JobSet(jobs)
    assert js.devpass_multi_ok()
    js.forward(loss=False, compact=True)
    together = [_exports(j) for j in jobs]
    for j in range(20):
        alone = _job(tables, dims, hidden, Z, cd, ("gpoe", "poe", "moe", "mopoe")[j % 4], seed=100 + j)
        nm.JobSet([alone]).forward(loss=False, compact=True)
        for m, (a, b) in enumerate(zip(_exports(alone), together[j])):
            for ta, tb, what in zip(a, b, ("out_loc", "out_sqerr", "out_rowdev")):
                assert torch.equal(ta, tb), (j, m, what)
        assert float(together[j][0][1][:N].abs().max()) > 0


@pytest.mark.parametrize("why", ["latent exports", "hidden 120", "latent 40", "endtoend trunk", "NMHIP_DEVPASS=0"])
def test_fallbacks_run_on_the_general_kernel(why, monkeypatch):
    """What the compact kernel does not take still runs forward(loss=False) -- through nm_forward -- and fills the exports."""
    N, dims, cd = 200, (61, 90, 47), 3
    hidden, Z, kind, extra, latent = (64, 48), 12, "multimodal", (), False
    if why == "latent exports":
        latent = True
    elif why == "hidden 120":
        hidden = (120, 48)
    elif why == "latent 40":
        Z = 40
    elif why == "endtoend trunk":
        kind, extra = "endtoend", ((32, 16), 2)
    xs, cs = _data(N, dims, cd, seed=13)
    job = _job(_tables(xs, cs), dims, hidden, Z, cd, "poe", seed=6, kind=kind, latent=latent, extra=extra)
    if why == "NMHIP_DEVPASS=0":
        assert nm.JobSet([job]).devpass_multi_ok()
        monkeypatch.setenv("NMHIP_DEVPASS", "0")
    js = nm.JobSet([job])
    assert not js.devpass_multi_ok()
    js.forward(loss=False)
    torch.cuda.synchronize()
    for m in range(len(job.kmods)):
        assert float(job.out_sqerr[m][:N].abs().max()) > 0, m
        assert float(job.out_rowdev[m][:N].abs().max()) > 0, m
    if latent:
        assert float(job.out_z[:N].abs().max()) > 0


def test_pred_recon_of_the_drop_in_class_takes_the_compact_kernel():
    """cVAE_multimodal.pred_recon wants neither loss nor latent: it runs with the latent exports off (the compact kernel
    where the shape allows) and returns the reconstruction the general kernel gives for the same draw; a following
    forward_multimodal gets its latent exports back."""
    import pandas as pd
    N, dims, cd = 200, (61, 90, 47), 3             # (one 256-row batch: the train step below keeps the job and its buffers)
    xs, cs = _data(N, dims, cd, seed=17)
    model = nm.cVAE_multimodal(list(dims), [64, 48], 12, cd, modalities=3, non_linear=True)
    model.to(DEV)
    torch.manual_seed(5)
    preds = model.pred_recon([pd.DataFrame(x.numpy()) for x in xs], cs[0].long().numpy(), DEV, "gpoe")
    job = model._job
    assert job.out_mu is None and nm.JobSet([job]).devpass_multi_ok()
    assert all(p.shape == (N, d) and np.isfinite(p).all() and np.abs(p).max() > 0 for p, d in zip(preds, dims))
    nm.JobSet([job]).forward(loss=True)                              # the same job, draw and tables on the general kernel
    torch.cuda.synchronize()
    for m in range(3):
        assert np.array_equal(preds[m], job.out_loc[m][:N].cpu().numpy()), m
    out = model.forward_multimodal([x[:64] for x in xs], [cs[0][:64].long()] * 3, "gpoe")
    assert model._job is job and job.out_mu is not None
    assert out["mu_multimodal"].shape == (64, 12) and float(out["mu_multimodal"].abs().max()) > 0


def test_test_folds_equals_test_fold():
    """sweep.test_folds (all folds of a procedure as one launch, one job per fold on its own test tables) against the
    fold-by-fold sweep.test_fold: equal per-subject errors, equal reconstructions, and every one of the five CSV kinds
    per modality and fold byte-identical."""
    K, n, d = 3, 300, 40
    cohort = prep.synthetic_cohort(n=n, d=d)
    folds = prep.kfold_indices(n, K, 42)
    mods = list(prep.HCP_MODALITIES)
    spec = nm.ModelSpec([d] * 3, [32, 24], 8, 29)
    jobs = []
    for k, (tr, _) in enumerate(folds):
        xs, cov = prep.fold_train_tables(cohort, mods, tr)
        job = nm.Job(spec, [nm.Table(x, cov, DEV) for x in xs], combine="gpoe", seed=1000 * k, init_seed=50 + k)
        nm.JobSet([job]).train(3)
        jobs.append(job)
    kinds = ("normalized", "reconstruction", "reconstruction_error", "reconstruction_error_roi", "deviation_as_feature_importance")
    with tempfile.TemporaryDirectory() as da, tempfile.TemporaryDirectory() as db:
        one = [sweep.test_fold(jobs[k], cohort, tr, te, mods, "gpoe", DEV, out_dir=Path(da) / f"{k:03d}")
               for k, (tr, te) in enumerate(folds)]
        many = sweep.test_folds(jobs, cohort, folds, mods, "gpoe", DEV, out_dirs=[Path(db) / f"{k:03d}" for k in range(K)])
        assert len(many) == K
        for k in range(K):
            for m in mods:
                assert len(one[k][m]) == len(folds[k][1]) and float(np.abs(one[k][m]).max()) > 0
                assert np.array_equal(one[k][m], many[k][m]), (k, m)
                for kind in kinds:
                    fa, fb = Path(da) / f"{k:03d}" / m / f"{kind}_{m}.csv", Path(db) / f"{k:03d}" / m / f"{kind}_{m}.csv"
                    assert fa.exists() and fb.exists(), (k, m, kind)
                    assert filecmp.cmp(fa, fb, shallow=False), (k, m, kind)
    # the reconstructions themselves: the evaluation jobs of both forms, out_loc bit for bit
    evs = [sweep._fold_eval_job(jobs[k], cohort, tr, te, mods, "gpoe", DEV)[0] for k, (tr, te) in enumerate(folds)]
    assert nm.JobSet(evs).devpass_multi_ok()
    nm.JobSet(evs).forward(loss=False)
    torch.cuda.synchronize()
    for k, (tr, te) in enumerate(folds):
        ev = sweep._fold_eval_job(jobs[k], cohort, tr, te, mods, "gpoe", DEV)[0]
        nm.JobSet([ev]).forward(loss=False)
        torch.cuda.synchronize()
        for m in range(3):
            assert torch.equal(ev.out_loc[m], evs[k].out_loc[m]), (k, m)
            assert torch.equal(ev.out_rowdev[m], evs[k].out_rowdev[m]), (k, m)
