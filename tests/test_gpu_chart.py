"""The chart pass on the device (nm_chart_pass: the grid request of the decoder pass with the cells dealt to workgroups and the
per-cell moments folded in the kernel): its loc export against nm_decode_pass bit for bit at the MFMA-tile, 128-row-tile,
256-row-tile and 64-ROI-chunk edges; the tile partials and the chart against the numpy restatement (tests/chart_ref.py)
applied to that loc, bit for bit; the chart against fp64 numpy at the tolerances the project applies to this quantity;
independence from the launch; the drop-in classes; the shapes it refuses."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import multi_modal_normative_modeling_amd as nm
from tests import chart_ref
from tests.test_gpu_decode import _grid, _job, _model, _spy
from tests.test_gpu_devpass_multi import _data, _tables

DEV = "cuda:0"
NAN = float("nan")

SHAPES = {                                                            # dims, hidden, Z, c_dim, decoders wanted
    "three": ((63, 64, 65), (64, 48), 12, 3, None),                   # the 64-ROI chunk's edges
    "one": ((379,), (110, 110), 10, 29, None),                        # six chunks, the last ragged; Z not a multiple of 4
    "four": ((40, 40, 40, 120), (112,), 32, 5, (0, 1, 3)),            # four decoders, one of them skipped; both shape limits
}
# (shape, cells, rows): every row edge at three cells, the cell counts' ends at a one-row last tile and at the tallest request
CASES = ([("three", 3, R) for R in (1, 16, 17, 127, 128, 129, 256, 257, 400)] + [("three", 1, 129), ("three", 64, 129), ("three", 64, 400)]
         + [("one", 3, 257), ("one", 1, 17), ("four", 3, 300), ("four", 64, 128)])


def _bits(a):
    return np.ascontiguousarray(a).view(np.int64)


def _make(shape, G, R, seed=0, loc=True):
    dims, hidden, Z, cd, want = SHAPES[shape]
    xs, cs = _data(40, dims, cd, seed=3)
    job = _job(_tables(xs, cs), dims, hidden, Z, cd, "poe", seed=9 + seed, latent=False)
    z = torch.randn(R, Z, generator=torch.Generator().manual_seed(40 + G + R + seed)) * 1.3
    grid = _grid(G, cd, seed=G + seed)
    job.enable_chart_exports(R, G, decoders=want, loc=loc)
    for kind in ("part", "chart", "loc"):
        for t in job.chart_full[kind]:
            if t is not None:
                t.fill_(NAN)
    job.set_chart_inputs(z, grid)
    return job, z, grid


@functools.lru_cache(maxsize=None)
def _run(shape, G, R):
    """One request through both passes -- computed once, shared, never modified: per wanted decoder the decode pass's loc, and
    the chart pass's loc, partials and chart (whole buffers, pre-filled with NaN), as numpy arrays."""
    job, z, grid = _make(shape, G, R)
    nm.JobSet([job]).chart()
    job.enable_decode_exports(R, G, decoders=job.chart_decoders)
    for t in job.dec_full["loc"]:
        if t is not None:
            t.fill_(NAN)
    job.set_decode_inputs(z, c_grid=grid, x=None)
    nm.JobSet([job]).decode()
    torch.cuda.synchronize()
    out = {}
    for m in job.chart_decoders:
        out[m] = {"D": job.tables[m].D, "dec": job.dec_full["loc"][m].cpu(), "loc": job.chart_full["loc"][m].cpu(),
                  "part": job.chart_full["part"][m].cpu().numpy(), "chart": job.chart_full["chart"][m].cpu().numpy()}
    skipped = [m for m in range(len(job.kmods)) if m not in job.chart_decoders]
    assert all(job.chart[m] is None and job.chart_full["part"][m] is None for m in skipped)
    return out


@pytest.mark.parametrize("shape,G,R", CASES)
def test_loc_equals_the_decode_pass_bit_for_bit(shape, G, R):
    res = _run(shape, G, R)
    assert len(res) == (3 if shape != "one" else 1)
    for m, r in res.items():
        D, ra = r["D"], (R + 255) // 256 * 256
        assert tuple(r["loc"].shape) == tuple(r["dec"].shape) == (G, ra, (D + 3) // 4 * 4)
        assert torch.equal(r["loc"], r["dec"]), (m, float((r["loc"] - r["dec"]).abs().max()))
        # over the NaN the buffer held: dead rows and pad columns are zeros, live values are values
        assert float(r["loc"][:, R:].abs().max() if ra > R else 0.0) == 0.0
        assert float(r["loc"][:, :, D:].abs().max() if r["loc"].shape[2] > D else 0.0) == 0.0
        assert torch.isfinite(r["loc"]).all() and float(r["loc"][:, :R, :D].abs().max()) > 0


@pytest.mark.parametrize("shape,G,R", CASES)
def test_partials_and_chart_equal_the_restatement_bit_for_bit(shape, G, R):
    for m, r in _run(shape, G, R).items():
        D, T = r["D"], (R + 127) // 128
        x = r["loc"][:, :R, :D].numpy()                               # [G, R, D] fp32
        cols = np.ascontiguousarray(x.transpose(1, 0, 2)).reshape(R, G * D)            # the cells side by side: [R, G D]
        want_part = chart_ref.partials(cols).reshape(T, G, D, 2).transpose(1, 0, 2, 3)
        got_part = r["part"][:, :T, :D]
        assert np.array_equal(_bits(got_part), _bits(want_part)), (m, np.abs(got_part - want_part).max())
        assert np.all(r["part"][:, :T, D:] == 0.0)                    # pad columns of a tile with rows: zeros
        assert np.isnan(r["part"][:, T:]).all()                       # tiles without a row: untouched
        want = chart_ref.merge(want_part.transpose(1, 0, 2, 3).reshape(T, G * D, 2), R).reshape(G, D, 4)
        got = r["chart"][:, :D]
        if R >= 2:
            assert np.array_equal(_bits(got), _bits(want)), (m, np.abs(got - want).max())
            assert np.all(got[:, :, 3] == 0) and np.all(got[:, :, 2] == R)
        else:
            assert np.isnan(got[:, :, :2]).all() and np.all(got[:, :, 3] == -2) and np.all(got[:, :, 2] == 1)
            assert np.array_equal(got[:, :, 2:], want[:, :, 2:]) and np.isnan(want[:, :, :2]).all()
        assert np.all(r["chart"][:, D:] == 0.0)                       # pad columns of the chart: zeros


@pytest.mark.parametrize("shape,G,R", [c for c in CASES if c[2] >= 2])
def test_chart_against_numpy_over_the_same_loc(shape, G, R):
    for m, r in _run(shape, G, R).items():
        D = r["D"]
        x = r["loc"][:, :R, :D].numpy().astype(np.float64)
        got = r["chart"][:, :D]
        np.testing.assert_allclose(got[:, :, 0], x.mean(1), rtol=1e-12, atol=1e-12)
        np.testing.assert_allclose(got[:, :, 1], x.var(1, ddof=1), rtol=1e-9, atol=1e-15)
        # and within the restatement's own derived bound (numpy's pairwise sums stand in for exact arithmetic here: a last-bit
        # allowance for them; tests/test_chart_ref_cpu.py holds the bound against exact rationals)
        for g in range(G if G <= 3 else 2):
            b_mean, b_var = chart_ref.bound(r["loc"][g, :R, :D].numpy())
            assert np.all(np.abs(got[g, :, 0] - x[g].mean(0)) <= b_mean + 2.0 ** -52 * np.abs(x[g].mean(0)))
            assert np.all(np.abs(got[g, :, 1] - x[g].var(0, ddof=1)) <= b_var + 1e-13 * x[g].var(0, ddof=1))


def test_a_non_finite_latent_row_is_flagged_not_averaged():
    job, z, grid = _make("three", 3, 129)
    z = z.clone()
    z[128, 0] = float("inf")
    job.set_chart_inputs(z, grid)
    nm.JobSet([job]).chart()
    torch.cuda.synchronize()
    for m in range(3):
        tab = job.chart[m].cpu().numpy()
        assert np.all(tab[:, :, 3] == -2) and np.isnan(tab[:, :, :2]).all() and np.all(tab[:, :, 2] == 129)


def test_the_chart_does_not_depend_on_the_launch():
    """One job alone, the same job among twenty with other heights and cell counts, a rerun, and loc on or off: the same
    bytes in the chart and in the partials."""
    shape, G, R = "three", 3, 400
    base = _run(shape, G, R)
    heights, cells = (400, 129, 40, 517, 1), (3, 1, 5, 64, 2, 7)
    jobs = []
    for j in range(20):
        if j == 7:
            jobs.append(_make(shape, G, R)[0])
        else:
            jobs.append(_make(("three", "four")[j % 2], cells[j % 6], heights[j % 5], seed=j, loc=j % 3 == 0)[0])
    js = nm.JobSet(jobs)
    js.chart()
    js.chart()                                                        # a rerun over its own results
    noloc = _make(shape, G, R, loc=False)[0]
    nm.JobSet([noloc]).chart()
    torch.cuda.synchronize()
    assert noloc.chart_loc == [None] * 3
    for m, r in base.items():
        for job, what in ((jobs[7], "among twenty"), (noloc, "without loc")):
            assert np.array_equal(_bits(job.chart_full["chart"][m].cpu().numpy()), _bits(r["chart"])), (m, what)
            got, T = job.chart_full["part"][m].cpu().numpy(), (R + 127) // 128
            assert np.array_equal(_bits(got[:, :T]), _bits(r["part"][:, :T])), (m, what)
        assert torch.equal(jobs[7].chart_full["loc"][m].cpu(), r["loc"])
    # every other job of the launch holds a chart of its own request
    for j, job in enumerate(jobs):
        for m in job.chart_decoders:
            tab = job.chart[m].cpu().numpy()
            assert tab.shape == (job.chart_cells, job.tables[m].D, 4) and np.all(tab[:, :, 2] == job.chart_rows), (j, m)
            assert np.all(tab[:, :, 3] == (0 if job.chart_rows >= 2 else -2)), (j, m)


def test_rows_split_over_launches_merge_only_when_covered():
    """The merge runs from tile 0 and only for a request the launch covers: a first launch over the first 256-row tile of a
    400-row request leaves the chart alone, the launch of all tiles writes it -- the same bytes as one launch alone."""
    shape, G, R = "three", 3, 400
    job = _make(shape, G, R)[0]
    js = nm.JobSet([job])
    js.chart(tile0=0, n_tiles=1)
    torch.cuda.synchronize()
    assert all(torch.isnan(job.chart_full["chart"][m]).all() for m in range(3))
    assert all(torch.isnan(job.chart_full["part"][m][:, 2:]).all() and torch.isfinite(job.chart_full["part"][m][:, :2]).all()
               for m in range(3))
    js.chart()
    torch.cuda.synchronize()
    for m, r in _run(shape, G, R).items():
        assert np.array_equal(_bits(job.chart_full["chart"][m].cpu().numpy()), _bits(r["chart"])), m


@pytest.mark.parametrize("cls", [nm.cVAE_multimodal, nm.mmJSD, nm.cVAE_multimodal_regression, nm.cVAE])
def test_normative_trajectory_kernel_fold_against_export_fold(cls, monkeypatch):
    dims, cd, S = ((61, 90, 47) if cls is not nm.cVAE else (61,)), 3, 300
    model = _model(dims, (64, 48), 12, cd, cls)
    grid = torch.eye(cd)[[0, 2, 2, 1]]
    monkeypatch.delenv("NMHIP_CHART", raising=False)
    seen = _spy(monkeypatch)
    old = model.normative_trajectory(grid, n_draws=S, seed=4)         # the default: today's route, today's bytes
    exp = model.normative_trajectory(grid, n_draws=S, seed=4, fold="export")
    assert seen and "nm_chart_pass" not in seen and "nm_decode_pass" in seen
    del seen[:]
    new = model.normative_trajectory(grid, n_draws=S, seed=4, fold="kernel")
    assert seen == ["nm_chart_pass"]
    monkeypatch.setenv("NMHIP_CHART", "1")
    del seen[:]
    env = model.normative_trajectory(grid, n_draws=S, seed=4)
    assert seen == ["nm_chart_pass"]
    z = torch.randn(S, 12, generator=torch.Generator().manual_seed(4))
    locs = model.decode_grid(z, grid)
    dealt = model.decode_grid(z, grid, deal=True)
    assert seen[-2:] == ["nm_decode_pass", "nm_chart_pass"]
    assert len(old) == len(new) == len(dims)
    for m, D in enumerate(dims):
        assert torch.equal(locs[m], dealt[m]) and tuple(dealt[m].shape) == (4, S, D)
        for k in ("mean", "var_latent", "noise_var", "sd_pred"):
            assert np.array_equal(old[m][k], exp[m][k]), (m, k)
            assert np.array_equal(new[m][k], env[m][k]) and new[m][k].dtype == np.float64 and new[m][k].shape == old[m][k].shape, (m, k)
        np.testing.assert_allclose(new[m]["mean"], old[m]["mean"], rtol=1e-12, atol=1e-12)
        np.testing.assert_allclose(new[m]["var_latent"], old[m]["var_latent"], rtol=1e-9, atol=1e-15)
        assert np.array_equal(new[m]["noise_var"], old[m]["noise_var"])
        assert (new[m]["sd_pred"] == np.sqrt(new[m]["var_latent"] + new[m]["noise_var"][None, :])).all()
        assert np.array_equal(new[m]["mean"][1], new[m]["mean"][2]) and not np.array_equal(new[m]["mean"][0], new[m]["mean"][1])
        # the kernel's chart is the restatement applied to the decoded rows
        want = np.stack([chart_ref.chart(locs[m][g].cpu().numpy()) for g in range(4)])
        assert np.array_equal(_bits(new[m]["mean"]), _bits(want[:, :, 0])) and np.array_equal(_bits(new[m]["var_latent"]), _bits(want[:, :, 1]))
    with pytest.raises(ValueError, match="fold"):
        model.normative_trajectory(grid, fold="device")


@pytest.mark.parametrize("why", ["wide", "hidden 120", "dmvae"])
def test_refused_models_raise_in_the_decode_refusal_s_wording_and_launch_nothing(why, monkeypatch):
    dims, cd = (61, 90, 47), 3
    if why == "dmvae":
        torch.manual_seed(3)
        model = nm.DMVAE(list(dims), [64, 48], 12, cd, modalities=3, non_linear=True)
        model.to(DEV)
    else:
        model = _model(dims, (300, 300) if why == "wide" else (120, 48), 12, cd)
    seen = _spy(monkeypatch)
    match = "general-shape" if why == "wide" else "nm_decode_pass_ok refuses"
    with pytest.raises(ValueError, match=match):
        model.normative_trajectory(torch.eye(cd), n_draws=32, fold="kernel")
    with pytest.raises(ValueError, match=match):
        model.decode_grid(torch.zeros(32, 12), torch.eye(cd), deal=True)
    monkeypatch.setenv("NMHIP_CHART", "1")                            # the switch does not widen what is admitted
    with pytest.raises(ValueError, match=match):
        model.normative_trajectory(torch.eye(cd), n_draws=32)
    assert "nm_chart_pass" not in seen
    job = model._decode_job()[0]
    assert job.chart_rows is None and job.chart_full is None          # nothing was allocated, nothing written
    assert not nm.JobSet([job]).chart_ok()
