"""The decoder pass on the device (nm_decode_pass: the decoder half alone, under the rows' own covariates or under every cell
of a covariate grid): against the forward kernels bit for bit with z = out_z at every shape class the encoder half's test
admits plus the SE shape; a grid cell against the per-row launch whose covariate table repeats that grid row, bit for bit;
against the oracle's decoder in both operand modes; many models with requests of different heights and cell counts in one
launch; the shapes it refuses; the drop-in classes' decode / decode_grid / normative_trajectory /
pred_recon_counterfactual; and that the covariates reach the output at all."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import multi_modal_normative_modeling_amd as nm
from multi_modal_normative_modeling_amd import engine, metrics
from oracle import cvae_ref as R
from tests.golden_util import Golden
from tests.test_gpu_devpass_multi import _data, _tables
from tests.test_gpu_latent import CASES as LATENT_CASES

DEV = "cuda:0"

# the shape classes of the encoder half's twin test and the SE shape over three 256-row batches (c 29)
CASES = list(LATENT_CASES) + [(517, (379, 379, 379), (110, 110), 10, 29, "gpoe", False, "multimodal", True)]


def _job(tables, dims, hidden, Z, c_dim, combine, seed, kind="multimodal", bypass=True, state=None, latent=True):
    spec = nm.ModelSpec(list(dims), list(hidden), Z, c_dim, True, kind)
    job = nm.Job(spec, tables, combine=combine, state=state, seed=seed, init_seed=seed, n_tiles_ws=tables[0].n_tiles,
                 single_bypass=bypass)
    job.enable_exports(loc=True, sqerr=True, rowdev=True, latent=latent)
    return job


def _fill(job, v=7.0):
    for kind in ("loc", "sqerr", "rowdev"):
        for t in job.dec_full[kind]:
            if t is not None:
                t.fill_(v)


@pytest.mark.parametrize("N,dims,hidden,Z,c_dim,combine,own_cov,kind,bypass", CASES)
def test_per_row_mode_equals_the_forward_kernels_bit_for_bit(N, dims, hidden, Z, c_dim, combine, own_cov, kind, bypass):
    xs, cs = _data(N, dims, c_dim, seed=21, own_cov=own_cov)
    tables = _tables(xs, cs)
    M = len(dims)
    gen = _job(tables, dims, hidden, Z, c_dim, combine, seed=11, kind=kind, bypass=bypass)
    nm.JobSet([gen]).forward()                                        # the general kernel, every export on
    assert nm.JobSet([gen]).decode_ok()
    gen.enable_decode_exports(N, 0, sqerr=True, rowdev=True)
    _fill(gen)
    gen.set_decode_inputs(gen.out_z[:N], c=None, x="tables")          # the tables' own cz and x
    nm.JobSet([gen]).decode()
    torch.cuda.synchronize()
    ra = tables[0].rows_alloc
    assert gen.dec_rows_alloc == ra and ra > N
    for m in range(M):
        D = dims[m]
        loc, sq, rd = gen.dec_full["loc"][m][0], gen.dec_full["sqerr"][m][0], gen.dec_full["rowdev"][m][0]
        assert torch.equal(loc[:, :D], gen.out_loc[m]), (m, "loc", float((loc[:, :D] - gen.out_loc[m]).abs().max()))
        assert torch.equal(sq[:, :D], gen.out_sqerr[m]), (m, "sqerr", float((sq[:, :D] - gen.out_sqerr[m]).abs().max()))
        assert torch.allclose(rd, gen.out_rowdev[m], rtol=2e-6, atol=1e-9), (m, "rowdev", float((rd - gen.out_rowdev[m]).abs().max()))
        assert float(loc[:N].abs().max()) > 0 and float(sq[:N].abs().max()) > 0 and float(rd[:N].abs().min()) > 0
        # buffers pre-filled with 7.0: zeros past row N (the ragged tile's rows, the empty half tile) and in the pad columns
        assert float(loc[N:].abs().max()) == 0.0 and float(sq[N:].abs().max()) == 0.0 and float(rd[N:].abs().max()) == 0.0, m
        if loc.shape[1] > D:
            assert float(loc[:, D:].abs().max()) == 0.0 and float(sq[:, D:].abs().max()) == 0.0, m
        # the views the caller reads
        assert tuple(gen.dec_loc[m].shape) == (1, N, D) and tuple(gen.dec_rowdev[m].shape) == (1, N)
        assert torch.equal(gen.dec_loc[m][0], gen.out_loc[m][:N])
    # the compact kernels' per-subject means: the same summation order, bit for bit
    cmp_ = _job(tables, dims, hidden, Z, c_dim, combine, seed=11, kind=kind, bypass=bypass, latent=False)
    js = nm.JobSet([cmp_])
    if js.devpass_multi_ok() or js.devpass_ok():                      # (one expert with the bypass off has no compact kernel)
        seen = []
        real = nm.JobSet._issue
        try:
            nm.JobSet._issue = lambda self, entry, *a: (seen.append(entry), real(self, entry, *a))[1]
            js.forward(loss=False, compact=True if M > 1 else None)
        finally:
            nm.JobSet._issue = real
        torch.cuda.synchronize()
        assert seen == ["nm_devpass_multi" if M > 1 else "nm_devpass"]
        for m in range(M):
            assert torch.equal(cmp_.out_loc[m], gen.out_loc[m]), m                  # (the same draw, the same z)
            assert torch.equal(gen.dec_full["rowdev"][m][0], cmp_.out_rowdev[m]), (m, "rowdev against the compact kernel")
    else:
        assert M == 1 and not bypass


def _grid(G, c_dim, seed):
    """G covariate rows: one-hot rows, and -- row min(1, G - 1) -- one that is not (values that round in bf16)."""
    g = torch.Generator().manual_seed(seed)
    grid = torch.zeros(G, c_dim)
    grid[torch.arange(G), torch.randint(0, c_dim, (G,), generator=g)] = 1
    odd = torch.tensor([0.3, -1.7, 0.123, 2.51, -0.077]).repeat((c_dim + 4) // 5)[:c_dim]
    grid[min(1, G - 1)] = odd
    assert not torch.equal(odd.to(torch.bfloat16).float(), odd)
    return grid


@pytest.mark.parametrize("G", [1, 3, 64])
def test_cell_mode_equals_per_row_mode_bit_for_bit(G):
    N, dims, hidden, Z, cd = 300, (61, 90, 47), (64, 48), 12, 3
    xs, cs = _data(N, dims, cd, seed=3)
    tables = _tables(xs, cs)
    z = torch.randn(N, Z, generator=torch.Generator().manual_seed(40 + G)) * 1.3
    grid = _grid(G, cd, seed=G)
    cell = _job(tables, dims, hidden, Z, cd, "gpoe", seed=9)
    cell.enable_decode_exports(N, G, sqerr=True, rowdev=True)
    _fill(cell)
    cell.set_decode_inputs(z, c_grid=grid, x="tables")
    nm.JobSet([cell]).decode()
    row = _job(tables, dims, hidden, Z, cd, "gpoe", seed=9)
    row.enable_decode_exports(N, 0, sqerr=True, rowdev=True)
    js = nm.JobSet([row])
    for g in range(G):
        _fill(row)
        row.set_decode_inputs(z, c=grid[g:g + 1].repeat(N, 1), x="tables")
        js.decode()
        for kind in ("loc", "sqerr", "rowdev"):
            for m in range(3):
                a, b = cell.dec_full[kind][m][g], row.dec_full[kind][m][0]
                assert torch.equal(a, b), (g, kind, m, float((a - b).abs().max()))
    torch.cuda.synchronize()
    for m in range(3):
        assert float(cell.dec_loc[m].abs().max()) > 0 and float(cell.dec_sqerr[m].abs().max()) > 0
        assert float(cell.dec_full["loc"][m][:, N:].abs().max()) == 0.0           # every cell's rows past N: zeros, not the 7.0


def test_packed_covariates_equal_the_table_s_bytes():
    N, cd = 300, 5
    g = torch.Generator().manual_seed(2)
    for c in (torch.randn(N, cd, generator=g) * 3, torch.randint(0, 2, (N, cd), generator=g)):
        t = nm.Table(torch.zeros(N, 7), c, DEV)
        mine = engine.pack_covariates(c, t.Cz, t.rows_alloc, DEV)
        torch.cuda.synchronize()
        assert mine.shape == t.cz.shape and torch.equal(mine.view(torch.int16), t.cz.view(torch.int16))


@functools.lru_cache(maxsize=None)
def _golden_decode(name):
    """The golden's weights, 300 random latent rows, three grid rows: the pass's loc per modality [3, 300, D] -- computed once,
    shared, never modified."""
    g = Golden(name)
    N = 300
    P = {k: v for k, v in g.weights("w0").items()}
    xs, cs = _data(N, g.dims, g.c_dim, seed=5)
    job = _job(_tables(xs, cs), g.dims, g.hidden, g.Z, g.c_dim, g.combine, seed=0, state=P)
    z = torch.randn(N, g.Z, generator=torch.Generator().manual_seed(77)) * 1.2
    grid = _grid(3, g.c_dim, seed=1)
    job.enable_decode_exports(N, 3)
    job.set_decode_inputs(z, c_grid=grid, x=None)
    nm.JobSet([job]).decode()
    torch.cuda.synchronize()
    return g, P, z, grid, [t.cpu() for t in job.dec_loc]


@pytest.mark.parametrize("name", ["mm3_gpoe", "mm4_uca_gpoe"])
def test_loc_matches_the_oracle_decoder(name):
    g, P, z, grid, locs = _golden_decode(name)
    rs = R.Spec(g.dims, g.hidden, g.Z, g.c_dim)
    N = z.shape[0]
    ref = {}
    for mode in ("fp32", "bf16"):
        R.set_operand_rounding(mode)
        try:
            with torch.no_grad():
                ref[mode] = [torch.stack([R.decoder_fwd(P, rs, m, z, grid[c:c + 1].repeat(N, 1))[0] for c in range(3)])
                             for m in range(g.M)]
        finally:
            R.set_operand_rounding("fp32")
    for m in range(g.M):
        got = locs[m]
        noise = float((ref["bf16"][m] - ref["fp32"][m]).abs().max())
        d16, d32 = float((got - ref["bf16"][m]).abs().max()), float((got - ref["fp32"][m]).abs().max())
        print(f"{name} modality {m}: |got - bf16| {d16:.3e}  |got - fp32| {d32:.3e}  noise {noise:.3e}  "
              f"max |ref| {float(ref['fp32'][m].abs().max()):.3e}")
        assert d16 <= 1.5 * noise + 1e-5, (m, d16, noise)
        assert d32 <= 3.0 * noise + 1e-5, (m, d32, noise)


def test_twenty_models_in_one_launch_equal_each_alone():
    dims, hidden, Z, cd = (61, 90, 47), (64, 48), 12, 3
    xs, cs = _data(300, dims, cd, seed=8)
    tables = _tables(xs, cs)
    one = _tables([xs[0]], [cs[0]])
    heights, cells = (300, 129, 40, 517), (0, 1, 3, 5, 2)

    def make(j):        # every fourth model has one expert; heights and cell counts differ from model to model
        job = (_job(one, dims[:1], hidden, Z, cd, "poe", seed=100 + j) if j % 4 == 3 else
               _job(tables, dims, hidden, Z, cd, ("gpoe", "poe", "moe")[j % 4], seed=100 + j))
        Rj, G = heights[j % 4], cells[j % 5]
        g = torch.Generator().manual_seed(500 + j)
        z = torch.randn(Rj, Z, generator=g)
        job.enable_decode_exports(Rj, G)
        _fill(job)
        if G:
            job.set_decode_inputs(z, c_grid=_grid(G, cd, seed=j), x=None)
        else:
            c = torch.zeros(Rj, cd)
            c[torch.arange(Rj), torch.randint(0, cd, (Rj,), generator=g)] = 1
            job.set_decode_inputs(z, c=c, x=None)
        return job

    jobs = [make(j) for j in range(20)]
    js = nm.JobSet(jobs)
    assert js.decode_ok()
    js.decode()
    for j in range(20):
        alone = make(j)
        nm.JobSet([alone]).decode()
        for m in range(len(alone.kmods)):
            assert torch.equal(alone.dec_full["loc"][m], jobs[j].dec_full["loc"][m]), (j, m)
            assert float(jobs[j].dec_loc[m].abs().max()) > 0
            assert float(jobs[j].dec_full["loc"][m][:, jobs[j].dec_rows:].abs().max()) == 0.0
    torch.cuda.synchronize()


def test_identical_runs_give_identical_bytes():
    g, P, z, grid, locs = _golden_decode("mm3_gpoe")
    xs, cs = _data(300, g.dims, g.c_dim, seed=5)
    job = _job(_tables(xs, cs), g.dims, g.hidden, g.Z, g.c_dim, g.combine, seed=0, state=P)
    job.enable_decode_exports(300, 3)
    job.set_decode_inputs(z, c_grid=grid, x=None)
    nm.JobSet([job]).decode()
    torch.cuda.synchronize()
    for m in range(g.M):
        assert torch.equal(job.dec_loc[m].cpu(), locs[m]), m


def test_covariates_reach_the_output():
    """Two grid rows that differ give different loc; identical rows give identical slabs."""
    N, dims, hidden, Z, cd = 200, (61, 90, 47), (64, 48), 12, 3
    xs, cs = _data(N, dims, cd, seed=4)
    job = _job(_tables(xs, cs), dims, hidden, Z, cd, "poe", seed=3)
    grid = torch.tensor([[1.0, 0, 0], [0, 1.0, 0], [1.0, 0, 0]])
    job.enable_decode_exports(N, 3)
    job.set_decode_inputs(torch.randn(N, Z, generator=torch.Generator().manual_seed(1)), c_grid=grid, x=None)
    nm.JobSet([job]).decode()
    torch.cuda.synchronize()
    for m in range(3):
        t = job.dec_loc[m]
        assert torch.equal(t[0], t[2]), m
        assert not torch.equal(t[0], t[1]) and float((t[0] - t[1]).abs().max()) > 1e-3, m


def _spy(monkeypatch):
    seen = []
    real = nm.JobSet._issue
    monkeypatch.setattr(nm.JobSet, "_issue", lambda self, entry, *a: (seen.append(entry), real(self, entry, *a))[1])
    return seen


def _model(dims, hidden, Z, cd, cls=None, seed=3):
    torch.manual_seed(seed)
    if cls is nm.cVAE:
        model = nm.cVAE(dims[0], list(hidden), Z, cd, non_linear=True)
    else:
        model = (cls or nm.cVAE_multimodal)(list(dims), list(hidden), Z, cd, modalities=len(dims), non_linear=True)
    model.to(DEV)
    return model


@pytest.mark.parametrize("why", ["hidden 120", "latent 40", "NMHIP_DECODE=0"])
def test_fallbacks_leave_decode_on_the_old_path(why, monkeypatch):
    dims, cd, B = (61, 90, 47), 3, 300
    hidden, Z = ((120, 48), 12) if why == "hidden 120" else (((64, 48), 40) if why == "latent 40" else ((64, 48), 12))
    model = _model(dims, hidden, Z, cd)
    z = torch.randn(B, Z, generator=torch.Generator().manual_seed(6)).to(DEV)
    c = torch.zeros(B, cd, dtype=torch.long)
    c[torch.arange(B), torch.arange(B) % cd] = 1
    monkeypatch.delenv("NMHIP_DECODE", raising=False)
    before = [model.decode(z, c, m).loc.clone() for m in range(3)]
    monkeypatch.setenv("NMHIP_DECODE", "0" if why == "NMHIP_DECODE=0" else "1")
    seen = _spy(monkeypatch)
    after = [model.decode(z, c, m).loc.clone() for m in range(3)]
    torch.cuda.synchronize()
    assert seen and "nm_decode_pass" not in seen
    for m in range(3):
        assert torch.equal(before[m], after[m]) and float(after[m].abs().max()) > 0, m
    # the pass itself says why it does not run
    with pytest.raises(ValueError, match="NMHIP_DECODE=0" if why == "NMHIP_DECODE=0" else "nm_decode_pass_ok refuses"):
        model.decode_grid(z, torch.eye(cd))
    job = model._decode_job()[0]
    assert nm.JobSet([job]).decode_ok() is False


@pytest.mark.parametrize("cls", [nm.cVAE_multimodal, nm.mmJSD, nm.cVAE_multimodal_regression, nm.cVAE])
def test_decode_through_the_pass_equals_the_old_route(cls, monkeypatch):
    dims, hidden, Z, cd, B = ((61, 90, 47) if cls is not nm.cVAE else (61,)), (64, 48), 12, 3, 300
    model = _model(dims, hidden, Z, cd, cls)
    z = torch.randn(B, Z, generator=torch.Generator().manual_seed(6)).to(DEV)
    c = torch.zeros(B, cd, dtype=torch.long)
    c[torch.arange(B), torch.arange(B) % cd] = 1
    call = (lambda m: model.decode(z, c)) if cls is nm.cVAE else (lambda m: model.decode(z, c, m))
    monkeypatch.setenv("NMHIP_DECODE", "0")
    old = [call(m) for m in range(len(dims))]
    monkeypatch.setenv("NMHIP_DECODE", "1")
    seen = _spy(monkeypatch)
    new = [call(m) for m in range(len(dims))]
    torch.cuda.synchronize()
    assert seen == ["nm_decode_pass"] * len(dims)
    for m in range(len(dims)):
        assert tuple(new[m].loc.shape) == (B, dims[m])
        assert torch.equal(old[m].loc, new[m].loc), (m, float((old[m].loc - new[m].loc).abs().max()))
        assert torch.equal(old[m].scale, new[m].scale) and float(new[m].loc.abs().max()) > 0


@pytest.mark.parametrize("cls", [nm.cVAE_multimodal, nm.mmJSD])
def test_counterfactual_under_the_cohort_s_own_cell_is_pred_recon(cls):
    import pandas as pd
    N, dims, cd = 300, (61, 90, 47), 3
    xs, _ = _data(N, dims, cd, seed=17)
    r = torch.tensor([0, 1, 0])
    c = r.repeat(N, 1).numpy()                                        # every subject carries covariate row r
    frames = [pd.DataFrame(x.numpy()) for x in xs]
    model = _model(dims, (64, 48), 12, cd, cls)
    model.pred_recon(frames, c, DEV, "gpoe")                          # (the first call builds the job)
    torch.manual_seed(5)
    want = model.pred_recon(frames, c, DEV, "gpoe")
    torch.manual_seed(5)
    got = model.pred_recon_counterfactual(frames, c, DEV, "gpoe", c_grid=r[None].float(), latent="draw")
    assert len(got) == 1 and len(got[0]) == 3
    for m in range(3):
        assert got[0][m].shape == (N, dims[m]) and np.array_equal(got[0][m], want[m]), m
    # the posterior mean under two cells: the subjects' own cell first, another second
    two = model.pred_recon_counterfactual(frames, c, DEV, "gpoe", c_grid=torch.tensor([[0.0, 1, 0], [1.0, 0, 0]]), latent="mean")
    assert len(two) == 2 and all(np.isfinite(a).all() for cell in two for a in cell)
    assert not np.array_equal(two[0][0], two[1][0]) and not np.array_equal(two[0][0], want[0])
    with pytest.raises(ValueError):
        model.pred_recon_counterfactual(frames, c, DEV, "gpoe", c_grid=r[None].float(), latent="median")


def test_cvae_counterfactual_mean_under_its_own_cell_is_pred_recon():
    import pandas as pd
    N, cd = 200, 3
    xs, _ = _data(N, (61,), cd, seed=19)
    r = torch.tensor([0, 0, 1])
    c = r.repeat(N, 1).numpy()
    model = _model((61,), (64, 48), 12, cd, nm.cVAE)
    want = model.pred_recon(pd.DataFrame(xs[0].numpy()), c, DEV)     # decodes mu through today's route
    got = model.pred_recon_counterfactual(pd.DataFrame(xs[0].numpy()), c, DEV, c_grid=r[None].float(), latent="mean")
    assert len(got) == 1 and np.array_equal(got[0], want)


@pytest.mark.parametrize("cls", [nm.cVAE_multimodal, nm.cVAE])
def test_normative_trajectory_is_cohort_moments_of_decode_grid(cls):
    dims, cd, S = ((40, 40, 40, 120) if cls is not nm.cVAE else (61,)), 5, 48
    model = _model(dims, (64, 48), 12, cd, cls)
    grid = torch.eye(cd)[[0, 3, 3, 1]]
    traj = model.normative_trajectory(grid, n_draws=S, seed=4)
    z = torch.randn(S, 12, generator=torch.Generator().manual_seed(4))
    locs = model.decode_grid(z, grid)
    assert len(traj) == len(dims) == len(locs)
    sd_state = model.state_dict()
    for m, D in enumerate(dims):
        assert tuple(locs[m].shape) == (4, S, D)
        mom = metrics.cohort_moments([locs[m][g] for g in range(4)], [np.zeros(S, np.int32)] * 4, ddof=1).cpu().numpy()
        t = traj[m]
        assert t["mean"].dtype == t["var_latent"].dtype == t["noise_var"].dtype == t["sd_pred"].dtype == np.float64
        assert t["mean"].shape == (4, D) and t["noise_var"].shape == (D,)
        assert np.array_equal(t["mean"], mom[:, :, 0]) and np.array_equal(t["var_latent"], mom[:, :, 2])
        assert (t["sd_pred"] == np.sqrt(t["var_latent"] + t["noise_var"].astype(np.float64)[None, :])).all()
        lv = sd_state[f"{model.spec.dec_prefix(m)}logvar_out"].reshape(-1).float().to(DEV)    # (exp where refresh_noise_var takes it)
        assert np.array_equal(t["noise_var"], torch.exp(lv).cpu().numpy().astype(np.float64))
        # the moments are those of the decoded rows: fp64 numpy on the export
        x = locs[m].cpu().numpy().astype(np.float64)
        np.testing.assert_allclose(t["mean"], x.mean(1), rtol=1e-12, atol=1e-12)
        np.testing.assert_allclose(t["var_latent"], x.var(1, ddof=1), rtol=1e-9, atol=1e-15)
        assert np.array_equal(t["mean"][1], t["mean"][2]) and not np.array_equal(t["mean"][0], t["mean"][1])
    # the rows may be handed in: the same rows, the same chart
    again = model.normative_trajectory(grid, z=z)
    assert all(np.array_equal(a["mean"], b["mean"]) and np.array_equal(a["sd_pred"], b["sd_pred"]) for a, b in zip(traj, again))
    with pytest.raises(ValueError):
        model.decode_grid(z, torch.zeros(65, cd))
