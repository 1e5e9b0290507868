"""Head models (cVAE_multimodal_regression, cVAE_multimodal_endtoend) in the persistent launch with one workgroup per decoder
(nm_train_steps_head_split; regression: 3 parts, end-to-end: 6 = two decoder banks, the head on part 0) against the
one-workgroup launch (nm_train_steps_head).  The bound is zero: every parameter's arithmetic is the same whichever workgroup
runs it, as for nm_launch_split (tests/test_gpu_parity.py: test_split_launch_equals_single_workgroup_bit_for_bit).  One
logged number is exempt, for a cause that is not the split's ("the hinge's logged value"): the per-subject
deviation out_rowdev is summed over a row's four waves by LDS float atomics in arrival order, so the contrastive hinge's
LOGGED mean (loss_log column NM_LOSS_CONTRAST) moves in its last bit between two runs of the SAME form, the one-workgroup
launch included (measured: whole against whole 3 of 5 rows differ by one ulp, parameters equal).  That column is held to
the project's bound for "the same operands, another association of the fp32 sums", 2e-5 of its largest value; every other
column and every other tensor stays torch.equal.  Every comparison prints its largest difference before it asserts."""
import numpy as np
import pytest
import torch

import multi_modal_normative_modeling_amd as nm
from multi_modal_normative_modeling_amd import _lib, engine, prep, sweep
from tests.golden_util import Golden
from tests.hip_harness import make_job

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DIMS, HIDDEN = [379, 379, 379], [110, 110]
HINGE = _lib.NM_LOSS_CONTRAST


# ---- jobs ------------------------------------------------------------------------------------------------------------
def golden_job(kind, layers=None, dropout=0.0):
    """reg3_gpoe / e2e3: the golden shapes, weights and draws of the reference classes' own trajectories."""
    if kind == "regression":
        g = Golden("reg3_gpoe")
        job = make_job(g, 0, kind="regression")
        job.set_fi(g.t("fi")[0])
        return job
    g = Golden("e2e3")
    layers = [int(v) for v in g.z["layers"]] if layers is None else layers
    spec = nm.ModelSpec(g.dims, g.hidden, g.Z, g.c_dim, True, "endtoend", tuple(layers), 2)
    state = None
    if layers == [int(v) for v in g.z["layers"]]:
        state = {k: v for k, v in g.weights("w0").items() if not k.endswith("num_batches_tracked")}
    tables = [nm.Table(g.xs(0)[m], g.t("c")[0], DEV) for m in range(g.M)]
    job = nm.Job(spec, tables, combine="poe", state=state, kl_weight=0.1, ll_weight=0.1, single_bypass=False)
    job.cls_margin, job.cls_w_contrast, job.cls_dropout = 1.0, 1.0, dropout
    job.set_labels(g.t("labels")[0])
    job.set_eps(g.t("eps")[0])
    return job


def baseline_job(kind, rows=600, seed=0, init_seed=42, dropout=0.0, dims=DIMS, hidden=HIDDEN):
    """BASELINE sizes (3 x 379 ROI, H = [110, 110]; regression: Z = 10, two raw covariates, gPoE; end-to-end = config 5:
    Z = 64, 29 covariates, classifier [128, 64, 32] or the five-block stack), in-kernel draws keyed by `seed`."""
    g = torch.Generator().manual_seed(1234 + rows)
    xes = [torch.randn(rows, d, generator=g) for d in dims]
    fi = torch.randn(rows, generator=g) * 0.5 + 1.0
    labels = (torch.rand(rows, generator=g) < 0.4).long()
    if kind == "regression":
        c = torch.rand(rows, 2, generator=g)
        spec = nm.ModelSpec(dims, hidden, 10, 2, True, "regression")
        job = nm.Job(spec, [nm.Table(x, c, DEV) for x in xes], combine="gpoe", seed=seed, init_seed=init_seed, loss_cap=8)
        job.set_fi(fi)
        return job
    layers = [128, 96, 64, 32, 16] if kind == "endtoend-deep" else [128, 64, 32]
    c = torch.rand(rows, 29, generator=g)
    spec = nm.ModelSpec(dims, hidden, 64, 29, True, "endtoend", tuple(layers), 2)
    job = nm.Job(spec, [nm.Table(x, c, DEV) for x in xes], combine="poe", kl_weight=0.1, ll_weight=0.1, seed=seed,
                 init_seed=init_seed, loss_cap=8, single_bypass=False)
    job.cls_margin, job.cls_w_contrast, job.cls_dropout = 0.5, 0.7, dropout
    job.set_labels(labels)
    return job


def train(js, kind, n, **kw):
    (js.train_regression if kind == "regression" else js.train_endtoend)(n, **kw)


def snapshot(job):
    """Everything a training launch leaves behind: parameters (the BatchNorm running statistics are part of the parameter
    buffer: state_dict names them), moments, loss rows, the head's predictions."""
    torch.cuda.synchronize()
    out = {"params": job.params, "adam_m": job.adam_m, "adam_v": job.adam_v, "loss_log": job.loss_log}
    if job.out_fi_pred is not None:
        out["out_fi_pred"] = job.out_fi_pred
    if job.out_logits is not None:
        out["out_logits"] = job.out_logits
    out = {k: v.detach().cpu().clone() for k, v in out.items()}
    for k, v in job.state_dict().items():
        if "running" in k:
            out["bn:" + k] = v.clone()
    return out


def assert_same(a, b, what):
    assert a.keys() == b.keys(), (what, sorted(a.keys() ^ b.keys()))
    worst = {k: float((a[k].double() - b[k].double()).abs().max()) for k in a}
    print(f"[head split] {what}: largest |difference| per tensor {worst}")
    for k in a:
        x, y = a[k], b[k]
        if k == "loss_log":                      # the hinge's logged mean: see the module docstring
            hx, hy = x[:, HINGE], y[:, HINGE]
            assert float((hx - hy).abs().max()) <= 2e-5 * float(hy.abs().max()), (what, "hinge column", hx.tolist(), hy.tolist())
            x, y = x.clone(), y.clone()
            x[:, HINGE] = y[:, HINGE] = 0.0
        assert torch.equal(x, y), (what, k, worst[k], int((x != y).sum()))


def whole_vs_split(make, kind, n_steps, what, grads=False):
    res = {}
    for split in (False, True):
        job = make()
        js = nm.JobSet([job])
        if grads:
            js.grads_head(0, split=split)
            torch.cuda.synchronize()
            res[split, "grads"] = {"grads": job.grads.detach().cpu().clone()}
        train(js, kind, n_steps, split=split)
        js.assert_finite()
        res[split] = snapshot(job)
    if grads:
        assert float(res[False, "grads"]["grads"].abs().max()) > 0.0
        assert_same(res[False, "grads"], res[True, "grads"], what + " grads_head")
    assert_same(res[False], res[True], what + f" {n_steps} steps")
    return res[True]


# ---- 1: golden sizes -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["regression", "endtoend"])
def test_golden_sizes_bit_for_bit(kind):
    """reg3_gpoe / e2e3: grads_head(0) whole against split -> job.grads equal; then 4 steps of train_regression /
    train_endtoend whole against split -> parameters, moments, loss rows, BatchNorm running statistics and the head's
    predictions equal."""
    assert nm.JobSet([golden_job(kind)]).head_split_parts() == (3 if kind == "regression" else 6)
    got = whole_vs_split(lambda: golden_job(kind), kind, 4, f"golden {kind}", grads=True)
    assert ("out_fi_pred" if kind == "regression" else "out_logits") in got
    if kind == "endtoend":
        assert any(k.startswith("bn:") for k in got)


# ---- 2: BASELINE sizes -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["regression", "endtoend", "endtoend-deep"])
def test_baseline_sizes_bit_for_bit(kind):
    """The shapes of test_head_models_one_launch_full_size_trajectory_vs_oracle on a 600-row table (batches of 256, 256
    and 88 rows), 5 steps in ONE launch: whole against split, and split in one launch against split step by step."""
    k = "regression" if kind == "regression" else "endtoend"
    one = whole_vs_split(lambda: baseline_job(kind), k, 5, f"BASELINE {kind}")
    job = baseline_job(kind)
    assert job.batches_per_epoch == 3
    js = nm.JobSet([job])
    for _ in range(5):
        train(js, k, 1, split=True)
    assert_same(one, snapshot(job), f"BASELINE {kind}: one launch against step by step")


# ---- 3: dropout ------------------------------------------------------------------------------------------------------
def test_dropout_on_bit_for_bit():
    """Dropout p = 0.5 in the classifier: the mask is a counter hash of (seed, step, block, row, feature group), so it does
    not depend on which workgroup draws it."""
    on = whole_vs_split(lambda: baseline_job("endtoend", dropout=0.5), "endtoend", 4, "dropout 0.5")
    off = baseline_job("endtoend", dropout=0.0)
    train(nm.JobSet([off]), "endtoend", 4, split=True)
    assert not torch.equal(on["params"], snapshot(off)["params"])          # the mask did something


# ---- 4: many models ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,n", [("regression", 5), ("regression", 20), ("endtoend", 5), ("endtoend", 20)])
def test_many_models_in_one_launch(kind, n):
    """n models with their own weights and in-kernel draws as 3 / 6 workgroups each in ONE launch: each equals the same
    model trained alone on the one-workgroup form; the models differ from each other."""
    make = lambda i: baseline_job(kind, rows=256, seed=100 + i, init_seed=7 + i)
    jobs = [make(i) for i in range(n)]
    js = nm.JobSet(jobs)
    assert js.head_split_parts() == (3 if kind == "regression" else 6)
    train(js, kind, 3)                                                     # (the automatic pick)
    assert js._pending_kinds == {"split"} or js._err_kinds == {"split"}   # ... was the split launch
    js.assert_finite()
    together = [snapshot(j) for j in jobs]
    for i in range(n):
        alone = make(i)
        train(nm.JobSet([alone]), kind, 3, split=False)
        assert_same(snapshot(alone), together[i], f"{kind} model {i} of {n}: alone (whole) against together (split)")
    assert not torch.equal(together[0]["params"], together[1]["params"])
    assert not torch.equal(together[0]["loss_log"], together[n - 1]["loss_log"])


def test_pick_and_residency():
    """A set too large for all its workgroups to be resident picks 1, and the C entry point refuses it."""
    job = golden_job("regression")
    small = nm.JobSet([job])
    assert small.head_split_parts() == 3
    cus = small._cus
    n_big = (cus // 3 // 8 + 1) * 8                                        # ceil(n / 8) * 8 * 3 > CUs
    big = nm.JobSet([job] * n_big)
    assert big.split_parts() == 1 and big.head_split_parts() == 1
    with pytest.raises(ValueError, match="resident"):
        big._head_parts(True)
    ptr = small._upload(1)                                                 # (the refusal comes before the array is read)
    st = small.lib.nm_train_steps_head_split(ptr, n_big, 3, 0, 1, 0, engine._stream_ptr(DEV))
    assert st == _lib.NM_E_RESIDENCY, st
    torch.cuda.synchronize()


# ---- 5: refusals ------------------------------------------------------------------------------------------------------
def _runs_on_old_form(js, kind, **kw):
    assert js.head_split_parts(**{k: v for k, v in kw.items() if k == "fused"}) == 1
    train(js, kind, 2, **kw)
    js.assert_finite()
    assert not js._pending_kinds and not js._err_kinds                     # no launch with hand-offs ran
    with pytest.raises(ValueError, match="split=True"):
        train(js, kind, 1, split=True, **kw)
    assert all(j.step == 2 for j in js.jobs)                               # the refused call trained nothing


def test_refusal_wide_trunk():
    job = baseline_job("regression", rows=256, dims=[70, 55, 61], hidden=[160, 144])
    assert job.spec.wide
    _runs_on_old_form(nm.JobSet([job]), "regression")


def test_refusal_tiled_classifier():
    job = golden_job("endtoend", layers=[256, 128, 64])
    _runs_on_old_form(nm.JobSet([job]), "endtoend")


def test_refusal_three_launch_form():
    _runs_on_old_form(nm.JobSet([golden_job("endtoend")]), "endtoend", fused=False)


def test_refusal_mixed_modality_counts():
    a = baseline_job("regression", rows=256)
    b = baseline_job("regression", rows=256, dims=[379, 379], seed=3)
    assert len(a.kmods) == 3 and len(b.kmods) == 2
    _runs_on_old_form(nm.JobSet([a, b]), "regression")


def test_job_listed_with_the_wrong_parts_is_refused_by_the_kernel():
    """Through the C ABI: a 3-decoder job listed with parts = 2 trains nothing and reports NM_SYNC_ERR_SHAPE."""
    job = golden_job("regression")
    js = nm.JobSet([job])
    ptr = js._upload(1)
    stream = engine._stream_ptr(DEV)
    torch.cuda.synchronize()
    before = {k: getattr(job, k).clone() for k in ("params", "adam_m", "adam_v", "loss_log")}
    st = js.lib.nm_train_steps_head_split(ptr, 1, 2, 0, 2, 0, stream)
    assert st == _lib.NM_OK, st
    err = torch.zeros(1, dtype=torch.int32, device=DEV)
    assert js.lib.nm_split_errors(ptr, 1, err.data_ptr(), 1, stream) == _lib.NM_OK
    torch.cuda.synchronize()
    assert int(err[0]) == _lib.NM_SYNC_ERR_SHAPE
    for k, v in before.items():
        assert torch.equal(getattr(job, k), v), k
    # listed correctly, the same job trains and leaves no error word
    st = js.lib.nm_train_steps_head_split(ptr, 1, 3, 0, 2, 0, stream)
    assert st == _lib.NM_OK, st
    assert js.lib.nm_split_errors(ptr, 1, err.data_ptr(), 1, stream) == _lib.NM_OK
    torch.cuda.synchronize()
    assert int(err[0]) == 0
    assert not torch.equal(job.params, before["params"])


# ---- 6: the sweeps ----------------------------------------------------------------------------------------------------
def test_sweeps_write_the_same_files_with_and_without_the_split(tmp_path, monkeypatch):
    """`sweep regression` and `sweep endtoend` on a small synthetic cohort, NMHIP_SPLIT=0 against unset: the ROI-wise
    deviation CSVs and FI predictions of the regression driver byte for byte; the end-to-end driver's metrics CSV equal in
    every column but steps_per_s (a wall-clock rate)."""
    import pandas as pd
    seen = []
    real = engine.JobSet._train_head

    def spy(self, step0, n_steps, flags=0, parts=1):
        seen.append(parts)
        return real(self, step0, n_steps, flags, parts)

    monkeypatch.setattr(engine.JobSet, "_train_head", spy)
    outs = {}
    for mode in ("0", None):
        if mode is None:
            monkeypatch.delenv("NMHIP_SPLIT", raising=False)
        else:
            monkeypatch.setenv("NMHIP_SPLIT", mode)
        d = tmp_path / ("off" if mode == "0" else "auto")
        common = ["-K", "5", "--folds", "0", "2", "--subjects", "320", "--out-dir", str(d)]
        sweep.main_regression(["-E", "3"] + common)
        sweep.main_endtoend(["-E", "3", "-Dropout", "0.5"] + common)
        outs[mode] = d
    n_reg = len(prep.datasets_name("HCPimage", "UCA-gPoE"))                  # the regression driver's default procedure: 4 tables
    assert seen == [1, 1, n_reg, 6], seen                                   # the drivers inherit the pick
    files = sorted(p.relative_to(outs["0"]) for p in outs["0"].rglob("*") if p.is_file())
    assert files == sorted(p.relative_to(outs[None]) for p in outs[None].rglob("*") if p.is_file())
    assert sum(f.name.endswith("_roiwise.csv") for f in files) == 2 * n_reg and any("endtoend_metrics" in f.name for f in files)
    for f in files:
        a, b = outs["0"] / f, outs[None] / f
        if "endtoend_metrics" in f.name:
            ta, tb = pd.read_csv(a).drop(columns=["steps_per_s"]), pd.read_csv(b).drop(columns=["steps_per_s"])
            ha, hb = ta.pop("final_contrastive").to_numpy(), tb.pop("final_contrastive").to_numpy()   # (module docstring)
            assert np.abs(ha - hb).max() <= 2e-5 * np.abs(hb).max(), (ha, hb)
            assert ta.equals(tb), (f, ta, tb)
            assert np.isfinite(ta["final_ce"].to_numpy()).all() and len(ta) == 2
        else:
            assert a.read_bytes() == b.read_bytes(), f
