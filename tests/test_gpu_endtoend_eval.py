"""The evaluation pass of the end-to-end model (nm_e2e_pass: one workgroup per (job, 128-row tile) runs the encoders, the
fusion, the latent, the eval-mode classifier, both decoder banks and the per-subject row table) against the two-launch route
it replaces (nm_forward + nm_head_classifier, JobSet.forward_endtoend(compact=False)), which the existing tests hold to the
oracle: row by row the two run the same arithmetic, so out_mu / out_logvar / out_z / out_logits / out_loc / out_sqerr must
agree bit for bit (out_rowdev to fp32 summation order, as in tests/test_gpu_devpass_multi.py: the general kernel adds the
four column-group sums of a row in arrival order).  The row table against tests/endtoend_ref.py fed with the pass's own
exports; the oracle directly; stale memory; many jobs, tile sub-ranges and repeats; the export mask; the shapes it refuses."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import multi_modal_normative_modeling_amd as nm
from multi_modal_normative_modeling_amd import _lib, metrics
from oracle import cvae_ref as R
from tests import endtoend_ref as E
from tests.golden_util import Golden
from tests.hip_harness import rel_err

DEV = "cuda:0"
COLS = metrics.ENDTOEND_ROW_COLUMNS
EXACT = ("pred", "margin", "dev_health", "dev_disease", "contrast", "status")

# (dims, hidden, Z, c_dim, classifier, classes, rows): small shapes on the edges -- ROI widths that are no multiple of a tile and
# 65 / 130 across the 64-ROI chunk boundary; 1 .. 300 rows (a lone row, one 16-row tile and a row, 127 / 128 / 129 around the
# 128-row tile, 256 / 257 around the batch, a ragged third tile); latent 1 .. 64 on both sides of every 16-column tile, once
# with Z + C = 127; the first hidden width at the stage's limit (112); 1, 2, 3 and 4 experts; 1 and 5 classifier blocks of
# width 1 .. 128; 2 and 4 classes; and BASELINE config 5's widths at 300 rows
SHAPES = {
    "z10_300": ([17, 23, 29], [40, 32], 10, 5, (32, 16), 2, 300),
    "chunk_z16_129": ([65, 130], [24], 16, 3, (1,), 4, 129),
    "one_expert_h112_z1_17": ([17], [112], 1, 2, (128,), 2, 17),
    "four_experts_z17_257": ([17, 23, 29, 65], [40, 32], 17, 4, (32, 128, 1, 16, 8), 2, 257),
    "z64_c63_128": ([23, 29, 17], [32, 40, 24], 64, 63, (128, 64), 4, 128),
    "z32_127": ([29, 17], [40], 32, 5, (64,), 2, 127),
    "z33_256": ([17, 23, 29], [40, 32], 33, 5, (32,), 2, 256),
    "one_row": ([29], [16], 16, 3, (8,), 2, 1),
    "config5_300": ([379, 379, 379], [110, 110], 64, 29, (128, 64, 32), 2, 300),
}


class _NoBlockJob(nm.Job):
    """A classifier with no hidden block (cls_layers = 0), which ModelSpec cannot name: the logits layer straight on the
    latent, its [classes, Z] matrix and bias being the first rows of block 0's Linear (the tiled layout of a [n, Z] matrix
    does not depend on n within the first 16 rows).  Both routes read the same descriptor."""

    def _shape_struct(self):
        j = super()._shape_struct()
        j.cls_layers = 0
        return j


def _job(dims, hidden, Z, cd, layers, classes, N, seed=0, cls=nm.Job, combine="poe"):
    spec = nm.ModelSpec(list(dims), list(hidden), Z, cd, True, "endtoend", tuple(layers), classes)
    g = torch.Generator().manual_seed(1000 + seed)
    c = torch.rand(N, cd, generator=g)
    tables = [nm.Table(torch.randn(N, d, generator=g), c, DEV) for d in dims]
    job = cls(spec, tables, combine=combine, seed=77 + seed, init_seed=5 + seed, single_bypass=False,
              n_tiles_ws=tables[0].n_tiles)
    sd = job.state_dict()
    for k, v in sd.items():                        # every tensor moved off its initial value, running statistics off (0, 1)
        if k.endswith("running_var"):
            sd[k] = 0.3 + 2.0 * torch.rand(v.shape, generator=g)
        elif k.endswith("running_mean"):
            sd[k] = 0.5 * torch.randn(v.shape, generator=g)
        elif v.is_floating_point():
            sd[k] = v + 0.05 * torch.randn(v.shape, generator=g)
    job.load_state_dict(sd)
    return job


def _snap(job):
    torch.cuda.synchronize()
    out = {k: getattr(job, k).cpu().clone() for k in ("out_mu", "out_logvar", "out_z", "out_logits")}
    out["row"] = job.e2e_row.cpu().clone() if job.e2e_row is not None else None
    for k in ("out_loc", "out_sqerr", "out_rowdev"):
        out[k] = [t.cpu().clone() if t is not None else None for t in getattr(job, k)]
    return out


def _amax(t) -> float:
    return float(t.abs().max()) if t.numel() else 0.0


def _poison(job):
    for t in (job.out_mu, job.out_logvar, job.out_z, job.out_logits, job.e2e_row, *job.out_loc, *job.out_sqerr, *job.out_rowdev):
        if t is not None:
            t.fill_(float("nan"))


def _check_table(job, snap, N, worst):
    """The row table against the restatement fed with the same pass's exports."""
    t = E.row_table(snap["out_logits"][:N, : job.spec.num_classes].numpy(), [d[:N].numpy() for d in snap["out_rowdev"]],
                    snap["out_mu"][:N].numpy(), snap["out_logvar"][:N].numpy())
    row = snap["row"].numpy()
    for name in EXACT:
        got = row[:N, COLS.index(name)]
        assert (got == t[name]).all(), name
    val, bnd = E.reference64(snap["out_logits"][:N, : job.spec.num_classes].numpy(), snap["out_mu"][:N].numpy(), snap["out_logvar"][:N].numpy())
    for name in ("p_disease", "kl"):
        ratio = E.worst_ratio(row[:N, COLS.index(name)], val[name], bnd[name])
        worst[name] = max(worst.get(name, 0.0), ratio)
        print(f"{name}: worst share of the bound {ratio:.3f}")
        assert ratio <= 1.0, (name, ratio)
    assert (row[:N, COLS.index("status")] == 0).all()
    assert float(np.abs(row[N:]).max(initial=0.0)) == 0.0              # rows past the table: zeros


@pytest.mark.parametrize("name", list(SHAPES))
def test_twin_and_row_table(name):
    """Every export of nm_e2e_pass equals the two-launch route's, for the joint mean, the seeded draw and injected noise and
    for the classifier on mu and on z; the pass's row table equals the restatement on its own exports.  The buffers hold
    NaN before the compact launch: nothing stale enters, dead rows come back as zeros, no parameter moves."""
    dims, hidden, Z, cd, layers, classes, N = SHAPES[name]
    job = _job(dims, hidden, Z, cd, layers, classes, N, seed=len(name))
    job.enable_endtoend_exports(rows=True, loc=True, sqerr=True, rowdev=True, latent=True)
    assert job.e2e_ok()
    js = nm.JobSet([job])
    g = torch.Generator().manual_seed(3)
    noise = torch.randn(job.tables[0].n_tiles, 256, Z, generator=g)
    params0 = job.params.clone()
    worst = {}
    for latent, eps, use_mu in (("mean", None, True), ("mean", None, False), ("draw", None, False), ("draw", noise, False),
                                ("draw", None, True)):
        job.set_eps(eps)
        job.cls_use_mu = use_mu
        job.touch()
        _poison(job)
        js.forward_endtoend(latent=latent, compact=False)
        a = _snap(job)
        _poison(job)
        js.forward_endtoend(latent=latent, compact=True)
        b = _snap(job)
        tag = (name, latent, eps is not None, use_mu)
        for k in ("out_mu", "out_logvar", "out_z"):
            assert torch.equal(a[k][:N], b[k][:N]), (tag, k, float((a[k][:N] - b[k][:N]).abs().max()))
        assert torch.equal(a["out_logits"][:N], b["out_logits"][:N]), (tag, float((a["out_logits"][:N] - b["out_logits"][:N]).abs().max()))
        assert torch.isfinite(b["out_logits"][:N]).all() and float(b["out_logits"][:N, :classes].abs().max()) > 0
        assert _amax(b["out_logits"][:N, classes:]) == 0.0
        for k in ("out_mu", "out_logvar", "out_z", "out_logits"):       # rows past the table, NaN before the launch: zeros
            assert _amax(b[k][N:]) == 0.0 and torch.isfinite(b[k]).all(), (tag, k)
            assert _amax(a[k][N:]) == 0.0, (tag, k)
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
            assert float(b["out_sqerr"][m][:N].abs().max()) > 0
            assert _amax(b["out_sqerr"][m][N:]) == 0.0 and _amax(b["out_loc"][m][N:]) == 0.0 and _amax(b["out_rowdev"][m][N:]) == 0.0
        _check_table(job, b, N, worst)
        _check_table(job, a, N, worst)              # (the two-launch route fills the same table from ITS exports)
        assert torch.isfinite(b["row"]).all()
    assert torch.equal(job.params, params0)          # running statistics and every other parameter: bit-unchanged
    print(f"{name}: worst share of a bound {worst}")


def test_classifier_without_hidden_blocks():
    """cls_layers = 0 (the logits layer on the latent itself): both routes, bit for bit."""
    job = _job([17, 23, 29], [40, 32], 10, 5, (32, 16), 4, 150, seed=9, cls=_NoBlockJob)
    job.enable_endtoend_exports(rows=True, rowdev=True)
    assert job.e2e_ok() and job.struct().cls_layers == 0
    js = nm.JobSet([job])
    for use_mu in (True, False):
        job.cls_use_mu = use_mu
        job.touch()
        js.forward_endtoend(latent="draw", compact=False)
        a = _snap(job)
        _poison(job)
        js.forward_endtoend(latent="draw", compact=True)
        b = _snap(job)
        assert torch.equal(a["out_logits"][:150], b["out_logits"][:150]) and float(b["out_logits"][:150].abs().max()) > 0
        _check_table(job, b, 150, {})


def test_against_the_oracle_on_golden_e2e3():
    """Golden e2e3's trained weights in eval mode: the pass's logits (classifier on the joint mean) and the deviations of both
    banks against oracle.cvae_ref with the kernel's operand rounding, at the bounds of
    test_classifier_head_config5_shape_vs_oracle."""
    g = Golden("e2e3")
    layers = [int(v) for v in g.z["layers"]]
    spec = nm.ModelSpec(g.dims, g.hidden, g.Z, g.c_dim, True, "endtoend", tuple(layers), 2)
    state = {k: v for k, v in g.weights(f"w{g.n_steps}").items() if not k.endswith("num_batches_tracked")}
    xes, c = g.xs(0), g.t("c")[0]
    tables = [nm.Table(xes[m], c, DEV) for m in range(g.M)]
    job = nm.Job(spec, tables, combine="poe", state=state, single_bypass=False)
    job.cls_use_mu = True
    job.enable_endtoend_exports(rows=True, loc=True, rowdev=True)
    nm.JobSet([job]).forward_endtoend(latent="mean", compact=True)
    s = _snap(job)
    rs = R.Spec(g.dims, g.hidden, g.Z, g.c_dim, True, kind="endtoend", classifier_layers=layers)
    P = {k: v.clone() for k, v in g.weights(f"w{g.n_steps}").items()}
    bn = {k: v for k, v in P.items() if "running" in k}
    R.set_operand_rounding("bf16")
    try:
        of = R.forward_endtoend(P, rs, xes, [c] * g.M, torch.zeros(g.B, g.Z), training=False, bn_stats=bn)
        ref_logits = R.classifier_fwd(P, rs, of["mu"], False, bn)
    finally:
        R.set_operand_rounding("fp32")
    B = g.B
    assert rel_err(s["out_logits"][:B, :2], ref_logits) < 2e-2
    assert rel_err(s["out_mu"][:B], of["mu"]) < 2e-2
    devs = [((xes[m] - of[key][m]) ** 2).mean(dim=1) for key in ("locs_h", "locs_d") for m in range(g.M)]
    for k, d in enumerate(devs):
        assert rel_err(s["out_rowdev"][k][:B], d) < 2e-2, k
    row = s["row"][:B]
    assert rel_err(row[:, COLS.index("dev_health")], torch.stack(devs[: g.M]).mean(dim=0)) < 2e-2
    assert rel_err(row[:, COLS.index("dev_disease")], torch.stack(devs[g.M:]).mean(dim=0)) < 2e-2


def test_twenty_jobs_tile_ranges_and_repeats():
    """20 jobs in one launch against each alone; a tile sub-range; two runs: bit for bit."""
    dims, hidden, Z, cd, layers, classes, N = [17, 23, 29], [40, 32], 17, 5, (32, 16), 2, 300
    jobs = [_job(dims, hidden, Z, cd, layers, classes, N, seed=j, combine=("poe", "moe", "mopoe")[j % 3]) for j in range(20)]
    for j in jobs:
        j.enable_endtoend_exports(rows=True, loc=True, sqerr=True, rowdev=True)
    js = nm.JobSet(jobs)
    js.forward_endtoend(latent="draw", compact=True)
    together = [_snap(j) for j in jobs]
    js.forward_endtoend(latent="draw", compact=True)
    again = [_snap(j) for j in jobs]
    for j in range(20):
        alone = _job(dims, hidden, Z, cd, layers, classes, N, seed=j, combine=("poe", "moe", "mopoe")[j % 3])
        alone.enable_endtoend_exports(rows=True, loc=True, sqerr=True, rowdev=True)
        nm.JobSet([alone]).forward_endtoend(latent="draw", compact=True)
        a = _snap(alone)
        for k in ("out_mu", "out_logvar", "out_z", "out_logits", "row"):
            assert torch.equal(a[k], together[j][k]), (j, k)
        for k in ("out_loc", "out_sqerr", "out_rowdev"):
            for m in range(6):
                assert torch.equal(a[k][m], together[j][k][m]), (j, k, m)
    for j in range(20):
        for k in ("out_mu", "out_logvar", "out_z", "out_logits", "row"):
            assert torch.equal(again[j][k], together[j][k]), (j, k)
        for m in range(6):
            assert torch.equal(again[j]["out_rowdev"][m], together[j]["out_rowdev"][m]), (j, m)
        assert float(together[j]["row"][:N].abs().max()) > 0
    assert not torch.equal(together[0]["row"], together[3]["row"])
    # the second 256-row batch alone (rows 256 .. 299): those rows as in the whole launch, the others untouched
    part = jobs[3]
    _poison(part)
    nm.JobSet([part]).forward_endtoend(latent="draw", compact=True, tile0=1, n_tiles=1)
    p = _snap(part)
    assert torch.equal(p["row"][256:], together[3]["row"][256:]) and torch.isnan(p["row"][:256]).all()
    assert torch.equal(p["out_logits"][256:N], together[3]["out_logits"][256:N])
    for m in range(6):
        assert torch.equal(p["out_loc"][m][256:], together[3]["out_loc"][m][256:]) and torch.isnan(p["out_loc"][m][:256]).all()


def test_gpoe_is_refused_before_any_launch():
    """The end-to-end model has no alpha parameters: the library refuses a gPoE job (nm_e2e_alpha_ok) where its exports are
    asked for, and again at the launch if the combiner changes afterwards -- on either route."""
    job = _job([17, 23, 29], [40, 32], 16, 5, (32, 16), 2, 40, seed=1, combine="gpoe")
    assert not job.e2e_ok()
    with pytest.raises(ValueError, match="nm_e2e_alpha_ok"):
        job.enable_endtoend_exports()
    late = _job([17, 23, 29], [40, 32], 16, 5, (32, 16), 2, 40, seed=1)
    late.enable_endtoend_exports()
    assert late.e2e_ok()
    late.combine = "gpoe"                           # (no touch(): the answer follows the attribute itself)
    assert not late.e2e_ok()
    for compact in (True, False, None):
        with pytest.raises(ValueError):
            nm.JobSet([late]).forward_endtoend(compact=compact)


def test_export_mask_and_logits_only():
    """A want_mask that leaves out decoders' exports: those buffers stay as they were, the row table is the same.  With no
    row table and no decoder export the pass returns predict()'s logits."""
    dims, hidden, Z, cd, layers, classes, N = [17, 23, 29], [40, 32], 16, 5, (32, 16), 2, 200
    full = _job(dims, hidden, Z, cd, layers, classes, N, seed=2)
    full.cls_use_mu = True
    full.enable_endtoend_exports(rows=True, loc=True, sqerr=True, rowdev=True)
    nm.JobSet([full]).forward_endtoend(compact=True)
    f = _snap(full)
    some = _job(dims, hidden, Z, cd, layers, classes, N, seed=2)
    some.cls_use_mu = True
    some.enable_endtoend_exports(rows=True, loc=True, sqerr=True, rowdev=True, decoders=[1, 5])
    _poison(some)
    nm.JobSet([some]).forward_endtoend(compact=True)
    s = _snap(some)
    assert torch.equal(s["row"], f["row"]) and torch.equal(s["out_logits"][:N], f["out_logits"][:N])
    for m in range(6):
        if m in (1, 5):
            assert torch.equal(s["out_loc"][m], f["out_loc"][m]) and torch.equal(s["out_rowdev"][m], f["out_rowdev"][m])
        else:
            assert torch.isnan(s["out_loc"][m]).all() and torch.isnan(s["out_sqerr"][m]).all() and torch.isnan(s["out_rowdev"][m]).all()
    bare = _job(dims, hidden, Z, cd, layers, classes, N, seed=2)
    bare.cls_use_mu = True
    bare.enable_endtoend_exports(rows=False, loc=False, sqerr=False, rowdev=False)
    nm.JobSet([bare]).forward_endtoend(compact=True)
    torch.cuda.synchronize()
    assert bare.e2e_row is None and torch.equal(bare.out_logits[:N].cpu(), f["out_logits"][:N])
    # predict(): forward + head_classifier on the joint mean, eval mode -- the existing route
    ref = _job(dims, hidden, Z, cd, layers, classes, N, seed=2)
    ref.cls_train, ref.cls_use_mu = False, True
    ref.enable_exports(loc=False, sqerr=False, rowdev=False, latent=True)
    rs = nm.JobSet([ref])
    rs.forward()
    rs.head_classifier(backward=False, tile0=0, n_tiles=ref.tables[0].n_tiles)
    torch.cuda.synchronize()
    assert torch.equal(ref.out_logits[:N].cpu(), f["out_logits"][:N])


@pytest.mark.parametrize("hidden,layers", [([40, 32], (256, 128)), ([300, 160], (32, 16))])
def test_refused_shapes_take_the_two_launch_route(hidden, layers):
    """A tiled classifier and a trunk on the general-shape path: nm_e2e_pass_ok refuses them, forward_endtoend runs them on
    forward + head_classifier and fills the same table; compact=True names the refusal."""
    N = 150
    job = _job([17, 23, 29], hidden, 16, 5, layers, 2, N, seed=4)
    job.enable_endtoend_exports(rows=True, rowdev=True)
    assert not job.e2e_ok()
    js = nm.JobSet([job])
    with pytest.raises(ValueError, match="nm_e2e_pass"):
        js.forward_endtoend(compact=True)
    _poison(job)
    js.forward_endtoend(latent="mean")
    s = _snap(job)
    _check_table(job, s, N, {})
    assert float(s["row"][:N, COLS.index("dev_health")].min()) > 0 and torch.isfinite(s["row"]).all()
