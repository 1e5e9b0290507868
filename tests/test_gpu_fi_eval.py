"""The evaluation pass of the regression model (nm_fi_pass: one workgroup per (job, 128-row tile) runs the encoders once, then
per latent draw the fusion, every decoder and the regressor on the residuals, which stay in LDS) against the two-launch route
it replaces (the general forward kernel with exports + nm_head_regression, JobSet.forward_fi(compact=False)), which the
existing tests hold to the oracle: row by row the two run the same arithmetic, so out_fi_pred / out_mu / out_logvar / out_z /
out_loc / out_sqerr must agree bit for bit (out_rowdev to fp32 summation order, as in tests/test_gpu_devpass_multi.py).  The
row table against tests/fi_ref.py fed with the pass's own exports; the draws one by one; the oracle directly; stale memory;
many jobs, tile sub-ranges and repeats; the export mask; the shapes it refuses."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import multi_modal_normative_modeling_amd as nm
from multi_modal_normative_modeling_amd import metrics
from multi_modal_normative_modeling_amd.engine import draw_seeds
from oracle import cvae_ref as R
from tests import fi_ref as F
from tests.golden_util import Golden
from tests.hip_harness import rel_err

DEV = "cuda:0"
COLS = metrics.FI_ROW_COLUMNS

# (dims, hidden, Z, c_dim, rows, single_bypass): the smallest shapes at which each boundary can break -- ROI widths that are no
# multiple of a tile, 65 / 130 across the 64-column chunk of the residual and of W1, exact chunks; 1 .. 300 rows around the
# 16-row tile, the 128-row tile and the 256-row batch; latent 1 .. 32 on both sides of the 16-column tile; the first hidden
# width at the stage's limit (112); 1 .. 4 experts, the one-expert bypass on and off; the flagship widths at 300 rows
SHAPES = {
    "z10_300": ([17, 23, 29], [40, 32], 10, 2, 300, False),
    "chunk_z16_129": ([65, 130], [24], 16, 3, 129, False),
    "one_expert_bypass_h112_z1_17": ([17], [112], 1, 2, 17, True),
    "one_expert_h112_z1_17": ([17], [112], 1, 2, 17, False),
    "four_experts_z17_257": ([17, 23, 29, 65], [40, 32], 17, 4, 257, False),
    "exact_chunks_z32_128": ([64, 128], [32], 32, 5, 128, False),
    "z32_127": ([29, 17], [40], 32, 5, 127, False),
    "one_row": ([29], [16], 16, 3, 1, False),
    "uca_300": ([379, 379, 379], [110, 110], 10, 2, 300, False),
}


def _job(dims, hidden, Z, cd, N, seed=0, combine="gpoe", bypass=False, target=True):
    spec = nm.ModelSpec(list(dims), list(hidden), Z, cd, True, "regression")
    g = torch.Generator().manual_seed(2000 + seed)
    c = torch.rand(N, cd, generator=g)
    tables = [nm.Table(torch.randn(N, d, generator=g), c, DEV) for d in dims]
    job = nm.Job(spec, tables, combine=combine, seed=91 + seed, init_seed=7 + seed, single_bypass=bypass,
                 n_tiles_ws=tables[0].n_tiles)
    sd = job.state_dict()
    for k, v in sd.items():                        # every tensor moved off its initial value
        if v.is_floating_point():
            sd[k] = v + 0.05 * torch.randn(v.shape, generator=g)
    job.load_state_dict(sd)
    if target:
        job.set_fi(torch.rand(N, generator=g))
    return job


def _bufs(job):
    out = [job.out_mu, job.out_logvar, job.out_z, job.out_fi_pred, job.fi_row, job.fi_draws, *job.out_loc, *job.out_sqerr, *job.out_rowdev]
    return [t for t in out if t is not None]


def _poison(job):
    for t in _bufs(job):
        t.fill_(float("nan"))


def _snap(job):
    torch.cuda.synchronize()
    out = {k: (getattr(job, k).cpu().clone() if getattr(job, k) is not None else None)
           for k in ("out_mu", "out_logvar", "out_z", "out_fi_pred", "fi_row", "fi_draws")}
    for k in ("out_loc", "out_sqerr", "out_rowdev"):
        out[k] = [t.cpu().clone() if t is not None else None for t in getattr(job, k)]
    return out


def _amax(t) -> float:
    return float(t.abs().max()) if t.numel() else 0.0


def _check_table(job, s, N, draws=None):
    """The row table against the restatement fed with the same route's exports; returns the share of the kl bound."""
    d = s["fi_draws"][:N].numpy() if draws is None else draws
    tgt = job.fi_target[:N].cpu().numpy() if job.fi_target is not None else None
    wrong, share = F.check_table(s["fi_row"][:N].numpy(), d, [r[:N].numpy() for r in s["out_rowdev"]], s["out_mu"][:N].numpy(),
                                 s["out_logvar"][:N].numpy(), tgt)
    print(f"kl: worst share of the bound {share:.3f}")
    assert not wrong, wrong
    assert share <= 1.0
    assert _amax(s["fi_row"][N:]) == 0.0              # rows past the table: zeros
    return share


@pytest.mark.parametrize("name", list(SHAPES))
def test_twin(name):
    """Every export of nm_fi_pass equals the two-launch route's -- the seeded draw, injected noise, the joint mean; gPoE and
    PoE.  The buffers hold NaN before the compact launch: nothing stale enters, dead rows come back as zeros, no parameter and
    no byte of the shadow moves."""
    dims, hidden, Z, cd, N, byp = SHAPES[name]
    g = torch.Generator().manual_seed(3)
    for combine in ("gpoe", "poe"):
        job = _job(dims, hidden, Z, cd, N, seed=len(name), combine=combine, bypass=byp)
        job.enable_fi_exports(rows=True, draws=True, loc=True, sqerr=True, rowdev=True, latent=True)
        assert job.fi_ok()
        js = nm.JobSet([job])
        noise = torch.randn(job.tables[0].n_tiles, 256, Z, generator=g)
        js.forward_fi(compact=False)                   # (descriptors and shadow up)
        torch.cuda.synchronize()
        params0, shadow0 = job.params.clone(), job._wsh.clone()
        for latent, eps in (("draw", None), ("draw", noise), ("mean", None)):
            job.set_eps(eps)
            _poison(job)
            js.forward_fi(latent=latent, compact=False)
            a = _snap(job)
            _poison(job)
            js.forward_fi(latent=latent, compact=True)
            b = _snap(job)
            tag = (name, combine, latent, eps is not None)
            for k in ("out_fi_pred", "out_mu", "out_logvar", "out_z"):
                assert torch.equal(a[k][:N], b[k][:N]), (tag, k, float((a[k][:N] - b[k][:N]).abs().max()))
                assert _amax(b[k][N:]) == 0.0 and torch.isfinite(b[k]).all(), (tag, k)
                assert _amax(a[k][N:]) == 0.0, (tag, k)
            assert _amax(b["out_fi_pred"][:N]) > 0
            assert torch.equal(b["fi_draws"][:, 0], b["out_fi_pred"]) and torch.equal(a["fi_draws"], b["fi_draws"])
            if latent == "mean":
                assert torch.equal(b["out_z"][:N], b["out_mu"][:N])
            else:
                assert not torch.equal(b["out_z"][:N], b["out_mu"][:N])
            for m in range(len(job.kmods)):
                assert torch.equal(a["out_loc"][m], b["out_loc"][m]), (tag, m, "out_loc")
                assert torch.equal(a["out_sqerr"][m], b["out_sqerr"][m]), (tag, m, "out_sqerr")
                # (rows past the table: the general kernel leaves out_rowdev alone there, the pass stores zeros)
                assert torch.allclose(a["out_rowdev"][m][:N], b["out_rowdev"][m][:N], rtol=2e-6, atol=1e-9), (tag, m, "out_rowdev")
                assert torch.isfinite(b["out_loc"][m]).all() and torch.isfinite(b["out_sqerr"][m]).all()
                assert _amax(b["out_sqerr"][m][:N]) > 0
                assert _amax(b["out_sqerr"][m][N:]) == 0.0 and _amax(b["out_loc"][m][N:]) == 0.0 and _amax(b["out_rowdev"][m][N:]) == 0.0
            _check_table(job, b, N)
            _check_table(job, a, N)                    # (the two-launch route fills the same table from ITS exports)
            assert torch.isfinite(b["fi_row"]).all() and (b["fi_row"][:N, COLS.index("status")] == 0).all()
        torch.cuda.synchronize()
        assert torch.equal(job.params, params0) and torch.equal(job._wsh, shadow0)


@pytest.mark.parametrize("Z", [1, 10, 16])
def test_twin_one_expert_bypass_without_latent_exports(Z):
    """One expert, the bypass on, no latent export: the general kernel then makes the draw inside the heads' epilogue
    (fwd_heads), and the pass takes the same expression -- predictions and reconstructions bit for bit, for the seeded draw
    (element-wise generator at Z = 1 and 10, the pair generator at Z = 16), injected noise and the joint mean."""
    N = 145
    job = _job([65], [112], Z, 2, N, seed=30 + Z, bypass=True)
    job.enable_fi_exports(rows=True, draws=True, loc=True, sqerr=True, rowdev=True, latent=False)
    assert job.fi_ok() and job.out_mu is None and job.out_z is None
    js = nm.JobSet([job])
    noise = torch.randn(job.tables[0].n_tiles, 256, Z, generator=torch.Generator().manual_seed(8))
    seen = []
    for latent, eps in (("draw", None), ("draw", noise), ("mean", None)):
        job.set_eps(eps)
        _poison(job)
        js.forward_fi(latent=latent, compact=False)
        a = _snap(job)
        _poison(job)
        js.forward_fi(latent=latent, compact=True)
        b = _snap(job)
        tag = (Z, latent, eps is not None)
        assert torch.equal(a["out_fi_pred"], b["out_fi_pred"]), (tag, float((a["out_fi_pred"] - b["out_fi_pred"]).abs().max()))
        assert torch.equal(a["fi_draws"], b["fi_draws"]) and _amax(b["out_fi_pred"][:N]) > 0 and _amax(b["out_fi_pred"][N:]) == 0.0
        assert torch.equal(a["out_loc"][0], b["out_loc"][0]) and torch.equal(a["out_sqerr"][0], b["out_sqerr"][0]), tag
        assert torch.allclose(a["out_rowdev"][0][:N], b["out_rowdev"][0][:N], rtol=2e-6, atol=1e-9)
        for n in ("fi_pred", "fi_sd", "fi_min", "fi_max", "err", "status"):
            assert torch.equal(a["fi_row"][:, COLS.index(n)], b["fi_row"][:, COLS.index(n)]), (tag, n)
        assert torch.isfinite(b["fi_row"]).all() and (b["fi_row"][:N, COLS.index("status")] == 0).all()
        seen.append(b["out_fi_pred"])
    assert not torch.equal(seen[0], seen[1]) and not torch.equal(seen[0], seen[2])


@pytest.mark.parametrize("S", [1, 2, 5, 64])
def test_draws(S):
    """Column s of fi_draws is the prediction of a single-draw launch under that key, bit for bit; the row table is the
    restatement on the pass's own exports; one draw: no spread, and mean = minimum = maximum = the prediction."""
    dims, hidden, Z, cd, N, _ = SHAPES["z10_300"]
    job = _job(dims, hidden, Z, cd, N, seed=S)
    job.enable_fi_exports(rows=True, draws=True, rowdev=True)
    js = nm.JobSet([job])
    keys = draw_seeds(job.seed, S)
    _poison(job)
    js.forward_fi(n_draws=S, seeds=keys, compact=True)
    s = _snap(job)
    share = _check_table(job, s, N)
    assert share <= 1.0
    row = s["fi_row"][:N]
    assert (row[:, COLS.index("status")] == 0).all() and torch.isfinite(s["fi_draws"]).all() and _amax(s["fi_draws"][N:]) == 0.0
    assert torch.equal(s["fi_draws"][:, 0], s["out_fi_pred"])
    one = _job(dims, hidden, Z, cd, N, seed=S)
    one.enable_fi_exports(rows=True, draws=False, rowdev=True)
    os_ = nm.JobSet([one])
    for k in sorted({0, min(1, S - 1), S // 2, S - 1}):
        os_.forward_fi(n_draws=1, seeds=[keys[k]], compact=True)
        torch.cuda.synchronize()
        assert torch.equal(one.out_fi_pred.cpu(), s["fi_draws"][:, k]), k
    if S == 1:
        c = {n: row[:, COLS.index(n)] for n in COLS}
        assert _amax(c["fi_sd"]) == 0.0
        assert torch.equal(c["fi_pred"], c["fi_min"]) and torch.equal(c["fi_pred"], c["fi_max"])
        assert torch.equal(c["fi_pred"], s["out_fi_pred"][:N])
    else:
        assert float(row[:, COLS.index("fi_sd")].min()) > 0
        # the two-launch route folds the same draws into the same table
        _poison(job)
        js.forward_fi(n_draws=S, seeds=keys, compact=False)
        t = _snap(job)
        assert torch.equal(t["fi_draws"], s["fi_draws"])
        for n in F.EXACT:
            if n != "dev":                            # (dev: out_rowdev agrees to summation order only)
                assert torch.equal(t["fi_row"][:, COLS.index(n)], s["fi_row"][:, COLS.index(n)]), n


def test_against_the_oracle_on_golden_reg3():
    """Golden reg3_gpoe with its own weights and injected draws: fi_pred against oracle.cvae_ref at the bound
    tests/test_gpu_api_sweep.py holds the general route to."""
    g = Golden("reg3_gpoe")
    spec = nm.ModelSpec(g.dims, g.hidden, g.Z, g.c_dim, True, "regression")
    xes, c, eps = g.xs(0), g.t("c")[0], g.t("eps")[0]
    tables = [nm.Table(xes[m], c, DEV) for m in range(g.M)]
    job = nm.Job(spec, tables, combine=g.combine, state=g.weights("w0"), single_bypass=False)
    job.set_eps(eps)
    job.enable_fi_exports(rows=True, rowdev=True)
    assert job.fi_ok()
    nm.JobSet([job]).forward_fi(compact=True)
    torch.cuda.synchronize()
    rs = R.Spec(g.dims, g.hidden, g.Z, g.c_dim, kind="regression")
    of = R.forward_regression(g.weights("w0"), rs, xes, [c] * g.M, g.combine, eps)
    B = g.B
    got = job.fi_row[:B, COLS.index("fi_pred")].cpu()
    r, r_gold = rel_err(got, of["fi_pred"].detach().reshape(-1)), rel_err(got, g.t("fi_pred").reshape(-1))
    print(f"fi_pred: rel_err {r:.3e} against the oracle, {r_gold:.3e} against the golden file")
    assert r < 3e-2 and r_gold < 3e-2
    assert torch.equal(got, job.out_fi_pred[:B].cpu())


def test_twenty_jobs_tile_ranges_and_repeats():
    """Twenty jobs of mixed shapes in one launch against each alone; two runs; a tile sub-range: bit for bit."""
    names = ("z10_300", "chunk_z16_129", "four_experts_z17_257", "z32_127", "one_expert_h112_z1_17")
    combos = ("gpoe", "poe", "moe")

    def make(j):
        dims, hidden, Z, cd, N, byp = SHAPES[names[j % len(names)]]
        job = _job(dims, hidden, Z, cd, N, seed=j, combine=combos[j % 3], bypass=byp)
        job.enable_fi_exports(rows=True, draws=True, loc=True, rowdev=True)
        return job

    jobs = [make(j) for j in range(20)]
    js = nm.JobSet(jobs)
    nt = max(j.tables[0].n_tiles for j in jobs)
    js.forward_fi(n_draws=3, compact=True, n_tiles=nt)
    together = [_snap(j) for j in jobs]
    js.forward_fi(n_draws=3, compact=True, n_tiles=nt)
    again = [_snap(j) for j in jobs]
    keys = ("out_mu", "out_logvar", "out_z", "out_fi_pred", "fi_row", "fi_draws")
    for j in range(20):
        alone = make(j)
        nm.JobSet([alone]).forward_fi(n_draws=3, compact=True)
        a = _snap(alone)
        for k in keys:
            assert torch.equal(a[k], together[j][k]) and torch.equal(again[j][k], together[j][k]), (j, k)
        for m in range(len(alone.kmods)):
            for k in ("out_loc", "out_rowdev"):
                assert torch.equal(a[k][m], together[j][k][m]) and torch.equal(again[j][k][m], together[j][k][m]), (j, k, m)
        assert _amax(together[j]["fi_row"]) > 0 and torch.isfinite(together[j]["fi_row"]).all()
    # the second 256-row batch alone (rows 256 .. 299): those rows as in the whole launch, the others untouched
    part, N = jobs[0], 300
    _poison(part)
    nm.JobSet([part]).forward_fi(n_draws=3, compact=True, tile0=1, n_tiles=1)
    p = _snap(part)
    for k in ("fi_row", "fi_draws", "out_fi_pred", "out_z"):
        assert torch.equal(p[k][256:], together[0][k][256:]) and torch.isnan(p[k][:256]).all(), k
    for m in range(3):
        assert torch.equal(p["out_loc"][m][256:], together[0]["out_loc"][m][256:]) and torch.isnan(p["out_loc"][m][:256]).all()


def test_export_mask_and_missing_tables():
    """A want_mask that leaves out decoders' exports: those buffers stay as they were (the decoders still run: the head needs
    their residuals), the predictions are the same.  No row table, no fi_draws: out_fi_pred alone."""
    dims, hidden, Z, cd, N, _ = SHAPES["z10_300"]
    full = _job(dims, hidden, Z, cd, N, seed=2)
    full.enable_fi_exports(rows=True, draws=True, loc=True, sqerr=True, rowdev=True)
    nm.JobSet([full]).forward_fi(n_draws=2, compact=True)
    f = _snap(full)
    some = _job(dims, hidden, Z, cd, N, seed=2)
    some.enable_fi_exports(rows=True, draws=True, loc=True, sqerr=True, rowdev=True, decoders=[1])
    _poison(some)
    nm.JobSet([some]).forward_fi(n_draws=2, compact=True)
    s = _snap(some)
    assert torch.equal(s["fi_row"], f["fi_row"]) and torch.equal(s["fi_draws"], f["fi_draws"])
    for m in range(3):
        if m == 1:
            assert torch.equal(s["out_loc"][m], f["out_loc"][m]) and torch.equal(s["out_rowdev"][m], f["out_rowdev"][m])
        else:
            assert torch.isnan(s["out_loc"][m]).all() and torch.isnan(s["out_sqerr"][m]).all() and torch.isnan(s["out_rowdev"][m]).all()
    bare = _job(dims, hidden, Z, cd, N, seed=2)
    bare.enable_fi_exports(rows=False, draws=False, loc=False, sqerr=False, rowdev=False, latent=True)
    nm.JobSet([bare]).forward_fi(n_draws=2, compact=True)
    torch.cuda.synchronize()
    assert bare.fi_row is None and bare.fi_draws is None
    assert torch.equal(bare.out_fi_pred.cpu(), f["out_fi_pred"])


@pytest.mark.parametrize("hidden,Z", [([256], 16), ([40, 32], 33)])
def test_refused_shapes_take_the_two_launch_route(hidden, Z):
    """A trunk on the general-shape path and a latent above 32: nm_fi_pass_ok refuses them, forward_fi runs them on the
    forward kernel + nm_head_regression and fills the same table; compact=True names the refusal."""
    N = 150
    job = _job([17, 23, 29], hidden, Z, 2, N, seed=4)
    job.enable_fi_exports(rows=True, draws=True, rowdev=True)
    assert not job.fi_ok()
    js = nm.JobSet([job])
    with pytest.raises(ValueError, match="nm_fi_pass"):
        js.forward_fi(compact=True)
    _poison(job)
    js.forward_fi(n_draws=2)
    s = _snap(job)
    _check_table(job, s, N)
    assert torch.isfinite(s["fi_row"]).all() and float(s["fi_row"][:N, COLS.index("dev")].min()) > 0


def test_mean_takes_one_draw_and_a_missing_target_is_flagged():
    dims, hidden, Z, cd, N, _ = SHAPES["z32_127"]
    job = _job(dims, hidden, Z, cd, N, seed=5, target=False)
    job.enable_fi_exports(rows=True, draws=True, rowdev=True)
    js = nm.JobSet([job])
    sentinel = job.out_fi_pred.fill_(7.0).clone()
    for compact in (True, False, None):
        with pytest.raises(ValueError, match="n_draws"):
            js.forward_fi(latent="mean", n_draws=2, compact=compact)
    torch.cuda.synchronize()
    assert torch.equal(job.out_fi_pred, sentinel)      # refused before any launch
    for compact in (True, False):
        _poison(job)
        js.forward_fi(compact=compact)
        s = _snap(job)
        _check_table(job, s, N)
        assert _amax(s["fi_row"][:N, COLS.index("err")]) == 0.0 and (s["fi_row"][:N, COLS.index("status")] == 2).all()
