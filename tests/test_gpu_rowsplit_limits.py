"""Row-split launch (nm_launch_rowsplit) at the Adam sweep's table limits and at the metric's full size.

The sweep (csrc/nm_rowsplit.hip: rs_sweep) is the only place where a row-split model's gradient partials are summed and
its parameters updated; its tables have a fixed capacity (NM_RS_MAX_PASSES weight passes, NM_RS_MAX_VSEGS vector segments,
SW_NV * KH * 512 vector elements).  Here:

  * the host gate (Job.rowsplit_ok, layout.rowsplit_limit) equals nm_rowsplit_ok on real jobs, a refused job is never
    launched (explicit rowsplit= included) and the automatic pick falls back to the whole-batch launch;
  * the kernel's own guard refuses a C-ABI launch it cannot hold (error word, nothing written) and admits the real
    capacity of k = 4;
  * at the accepted edge -- alpha the last element the sweep covers -- every gradient and moment element against the
    whole-batch launch and the oracle;
  * the metric's shape over 8 steps on every path (k, helpers, one launch vs stepwise), the shadow images the sweep leaves
    behind against ones rebuilt from the master, mixed modality widths, and the bench's five-model leg.

Every element check covers the real parameters (grads_dict / adam_dicts / state_dict), not layout padding.
Reference: the train step of cVAE.py:1166-1196 / multimodal_kfold_train_cvae_supervised.py:177-199."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

import multi_modal_normative_modeling_amd as nm
from multi_modal_normative_modeling_amd import _lib
from oracle import cvae_ref as R
from tests.hip_harness import DEV

H2, Z10, C29 = [110, 110], 10, 29
LR = 1e-4


def _onehot(gen, B, c_dim=C29):
    c = torch.zeros(B, c_dim)
    c[torch.arange(B), torch.randint(0, c_dim - 2, (B,), generator=gen)] = 1
    c[torch.arange(B), c_dim - 2 + torch.randint(0, 2, (B,), generator=gen)] = 1
    return c


class Case:
    """Seeded data of one model shape: tables, covariates, draws [n_eps, 256, Z], reference-rule weights."""

    def __init__(self, dims, hidden=H2, Z=Z10, combine="gpoe", n_rows=256, seed=0, n_eps=1):
        gen = torch.Generator().manual_seed(seed)
        self.dims, self.hidden, self.Z, self.combine, self.n_rows = list(dims), list(hidden), Z, combine, n_rows
        self.spec = nm.ModelSpec(self.dims, self.hidden, Z, C29, True)
        self.P = nm.ParamLayout(self.spec).init_reference_rule(seed)
        self.xs = [torch.randn(n_rows, d, generator=gen) * 1.2 for d in self.dims]
        self.c = _onehot(gen, n_rows)
        self.eps = torch.randn(n_eps, 256, Z, generator=gen)
        self._tables = None

    def tables(self):
        if self._tables is None:
            self._tables = [nm.Table(x, self.c, DEV) for x in self.xs]
        return self._tables

    def job(self, state=None):
        j = nm.Job(self.spec, self.tables(), combine=self.combine, state=state if state is not None else self.P)
        j.set_eps(self.eps)
        return j

    def batch(self, s):
        b = s % ((self.n_rows + 255) // 256)
        r0, r1 = b * 256, min(self.n_rows, b * 256 + 256)
        return [x[r0:r1] for x in self.xs], self.c[r0:r1], self.eps[s % self.eps.shape[0]][:r1 - r0]

    def oracle_grads(self, mode):
        """loss and gradients of step 0 with fp32 or bf16 operand rounding."""
        rs = R.Spec(self.dims, self.hidden, self.Z, C29, True)
        xs, c, eps = self.batch(0)
        R.set_operand_rounding(mode)
        try:
            leaves = {k: v.clone().requires_grad_(True) for k, v in self.P.items()}
            fwd = R.forward_multimodal(leaves, rs, xs, [c.long()] * len(xs), self.combine, eps)
            loss = R.loss_multimodal(rs, xs, fwd)
            loss["total"].sum().backward()
            return loss, {k: (v.grad if v.grad is not None else torch.zeros_like(v)) for k, v in leaves.items()}
        finally:
            R.set_operand_rounding("fp32")

    def oracle_trajectory(self, n_steps, mode="bf16"):
        """Reconstruction loss of every step of the reference's own train loop (R.train_step)."""
        rs = R.Spec(self.dims, self.hidden, self.Z, C29, True)
        P = {k: v.clone() for k, v in self.P.items()}
        opt = R.Adam(P, R.optimizer_param_names(rs), lr=LR)
        lls = []
        R.set_operand_rounding(mode)
        try:
            for s in range(n_steps):
                xs, c, eps = self.batch(s)
                loss, _, _ = R.train_step(P, opt, rs, xs, [c.long()] * len(xs), self.combine, eps)
                lls.append(float(loss["ll"]))
        finally:
            R.set_operand_rounding("fp32")
        return lls


def _sync(js):
    js.check_split_errors(block=True)
    torch.cuda.synchronize()


def _rel_l2(a, r):
    return float((a - r).norm()) / (float(r.norm()) + 1e-30)


def _assert_close_per_element(got, want, what):
    """Per tensor: max |got - want| <= 2e-5 max |want| (fp32 summation order only; test_rowsplit_gradients_and_loss).
    Gradient buffers are NaN-poisoned before both launches: a tensor the whole-batch launch leaves untouched (a parameter
    the step does not use: alpha of a single expert behind the bypass) must stay untouched; every other element written."""
    for key, w in want.items():
        a = got[key]
        if bool(torch.isnan(w).all()):
            assert bool(torch.isnan(a).all()), (what, key, "written, but the whole-batch launch leaves it untouched")
            continue
        assert bool(torch.isfinite(a).all()), (what, key, "not finite")
        err = float((a - w).abs().max())
        assert err <= 2e-5 * float(w.abs().max()) + 1e-9, (what, key, err, float(w.abs().max()))


def _assert_vs_oracle(job, case, res):
    """run_case's bounds (tests/test_gpu_fullsize.py): reconstruction loss within 1e-4 of the fp32 oracle, every gradient
    within 4e-2 relative L2 of the bf16-operand oracle, and as close to the fp32 gradient (cosine) as the bf16 restatement."""
    (l32, g32), (_, g16) = res["fp32"], res["bf16"]
    row = job.loss_log[0].cpu()
    ll32 = float(l32["ll"].detach())
    assert abs(float(row[2]) - ll32) <= 1e-4 * abs(ll32), (float(row[2]), ll32)
    got = job.grads_dict()
    for k, r32 in g32.items():
        if float(r32.abs().max()) == 0:
            continue
        a, r16 = got[k].flatten(), g16[k].flatten()
        if a.numel() >= 8:
            cos = float(torch.nn.functional.cosine_similarity(a, r32.flatten(), dim=0))
            cos16 = float(torch.nn.functional.cosine_similarity(r16, r32.flatten(), dim=0))
            assert cos > min(0.985, cos16 - 0.005), (k, cos, cos16)
        assert float((a - r16).norm()) <= 4e-2 * float(r16.norm()) + 1e-9, k


def _snapshot(job):
    return (job.params.cpu().clone(), job.adam_m.cpu().clone(), job.adam_v.cpu().clone(), job.loss_log.cpu().clone())


# -- the host gate ---------------------------------------------------------------------------------------------------------
GATE_SHAPES = [
    ([1305], H2, Z10), ([1306], H2, Z10), ([1090], [127, 127, 127], 64), ([1091], [127, 127, 127], 64),
    ([379, 1305, 379], H2, Z10), ([379, 1306, 379], H2, Z10), ([1400], H2, Z10), ([379, 379, 379], H2, Z10),
    ([379, 379, 379, 1137], H2, Z10), ([1500], [16], 4), ([1530], [16], 4), ([2000, 50], [32, 16], 8),
]


def test_rowsplit_gate_equals_c_check_and_refuses_before_launch():
    """Job.rowsplit_ok() == (nm_rowsplit_ok == 0) on both sides of every table edge; a refused job gets k = 1 from the
    automatic pick, and an explicit row-split train / grads raises ValueError before anything runs."""
    lib = _lib.load()
    n_ref = 0
    for dims, hidden, Z in GATE_SHAPES:
        case = Case(dims, hidden, Z)
        job = case.job()
        job._ensure_rowsplit(2)
        ok_c = lib.nm_rowsplit_ok(C.byref(job.struct())) == 0
        assert job.rowsplit_ok() == ok_c, (dims, hidden, Z)
        assert nm.layout.rowsplit_fits(case.spec, [t.Kx for t in case.tables()]) == ok_c
        if ok_c:
            continue
        n_ref += 1
        js = nm.JobSet([job])
        assert js.rowsplit_k() == 1
        before = _snapshot(job)
        with pytest.raises(ValueError, match="vector elements"):
            js.train(1, rowsplit=2)
        with pytest.raises(ValueError, match="cannot run row-split"):
            js.grads(0, rowsplit=2)
        torch.cuda.synchronize()
        assert job.t == 0 and job.step == 0
        for a, b in zip(before, _snapshot(job)):
            assert torch.equal(a, b)
    assert n_ref == 6


def test_rowsplit_auto_pick_falls_back_past_the_tables():
    """100 single-modality models of 1400 ROI (-H 110 110, Z = 10): 104 groups would give k = 2 without helpers, where the
    sweep covers 3 072 of the 3 260 vector elements -- the set must train whole-batch instead, and a model of it equals
    the same model trained alone.  One over-limit model among five metric-shape ones also sends the set to k = 1."""
    case = Case([1400], n_rows=256, seed=3)
    jobs = []
    for i in range(100):
        j = case.job()
        j.seed = i
        j.set_eps(None)                                   # in-kernel draw, keyed by (seed, step, row, z)
        jobs.append(j)
    js = nm.JobSet(jobs)
    assert js.rowsplit_k() == 1
    js.train(2)
    _sync(js)
    alone = case.job()
    alone.seed = 7
    alone.set_eps(None)
    nm.JobSet([alone]).train(2, rowsplit=1, split=False)
    torch.cuda.synchronize()
    assert torch.equal(jobs[7].params.cpu(), alone.params.cpu())
    assert torch.equal(jobs[7].adam_v.cpu(), alone.adam_v.cpu())
    js.assert_finite()
    five = [Case([379, 379, 379], seed=i).job() for i in range(5)]
    assert nm.JobSet(five).rowsplit_k() == 4
    assert nm.JobSet(five + [Case([379, 1400, 379]).job()]).rowsplit_k() == 1


def test_rowsplit_kernel_guard_for_c_abi_callers():
    """A C-ABI caller that skips nm_rowsplit_ok: at k = 2 without helpers (3 072 vector elements) the kernel refuses a
    1400-ROI model -- every workgroup leaves before its first hand-off, the error word says why, nothing is written; at
    k = 4 (6 144 elements) the kernel holds it, and every gradient matches the whole-batch launch."""
    case = Case([1400], seed=4)
    lib = _lib.load()
    st = torch.cuda.current_stream().cuda_stream
    job = case.job()
    js = nm.JobSet([job])
    job._ensure_rowsplit(2)
    before = _snapshot(job)
    ptr = js._upload(2)
    assert lib.nm_launch_rowsplit(ptr, 1, 1, 2, 0, 0, 1, _lib.NM_F_BACKWARD | _lib.NM_F_ADAM, 0, st) == 0
    js._split_pending = True
    js._pending_kinds.add("rowsplit")
    torch.cuda.synchronize()
    with pytest.raises(nm.NmError, match="refused by the kernel"):
        js.check_split_errors(block=True)
    for a, b in zip(before, _snapshot(job)):
        assert torch.equal(a, b)
    js.check_split_errors(block=True)                     # read and cleared
    whole = case.job()
    whole.grads.fill_(float("nan"))
    nm.JobSet([whole]).grads(0)
    job.grads.fill_(float("nan"))
    job._ensure_rowsplit(4)
    ptr = js._upload(4)
    assert lib.nm_launch_rowsplit(ptr, 1, 1, 4, 0, 0, 1, _lib.NM_F_BACKWARD | _lib.NM_F_GRADS, 0, st) == 0
    js._split_pending = True
    _sync(js)
    _assert_close_per_element(job.grads_dict(), whole.grads_dict(), "k=4 C-ABI")


# -- the accepted edge, every element ---------------------------------------------------------------------------------------
EDGE_CASES = {
    "gpoe2_1305": dict(dims=[1305, 1305]),                                   # vtot = 3 071: alpha is the last element at KH = 2
    "se_1305": dict(dims=[1305]),
    "se_1090_h127x3_z64": dict(dims=[1090], hidden=[127, 127, 127], Z=64),
}


@pytest.mark.parametrize("name", list(EDGE_CASES))
def test_rowsplit_at_the_accepted_edge_every_element(name):
    """Gradients (NaN-poisoned before the launch) and one Adam step at k in {2, 4} x helpers in {0, auto}: per element
    against the whole-batch launch, and against the oracle at run_case's bounds.  An element the sweep skipped would stay
    NaN in the gradient and keep m = v = 0."""
    case = Case(seed=21, **EDGE_CASES[name])
    res = {mode: case.oracle_grads(mode) for mode in ("fp32", "bf16")}
    whole = case.job()
    whole.grads.fill_(float("nan"))
    nm.JobSet([whole]).grads(0)
    wtrain = case.job()
    nm.JobSet([wtrain]).train(1, rowsplit=1, split=False)
    torch.cuda.synchronize()
    wg = whole.grads_dict()
    wm, wv = wtrain.adam_dicts()
    for k in (2, 4):
        for h in (0, None):
            job = case.job()
            job.grads.fill_(float("nan"))
            js = nm.JobSet([job])
            js.grads(0, rowsplit=k, helpers=h)
            _sync(js)
            _assert_close_per_element(job.grads_dict(), wg, (name, k, h, "grads"))
            _assert_vs_oracle(job, case, res)
            tj = case.job()
            ts = nm.JobSet([tj])
            ts.train(1, rowsplit=k, helpers=h)
            _sync(ts)
            m, v = tj.adam_dicts()
            _assert_close_per_element(m, wm, (name, k, h, "adam_m"))
            _assert_close_per_element(v, wv, (name, k, h, "adam_v"))
            for key in wv:
                assert torch.equal(v[key] == 0, wv[key] == 0), (name, k, h, key)


def test_rowsplit_refuses_just_past_the_edge():
    """D = 1400 (3 260 vector elements, 3 261 as nm_rowsplit_ok counts them: alpha always; > 3 072): the explicit launch of
    test_rowsplit_at_the_accepted_edge_every_element is refused."""
    job = Case([1400], seed=21).job()
    js = nm.JobSet([job])
    with pytest.raises(ValueError, match="3261 vector elements > NM_RS_MAX_VEC = 3072"):
        js.grads(0, rowsplit=2, helpers=0)


# -- the metric's shape, several steps ---------------------------------------------------------------------------------------
N_STEPS = 8
METRIC = dict(dims=[379, 379, 379], n_rows=600, seed=5, n_eps=N_STEPS)    # batches 256 / 256 / 88


def _assert_trajectory_vs_whole(res, whole, n_steps, moment_bound, what):
    """test_rowsplit_one_launch_equals_stepwise_and_is_reproducible's bounds: parameters within 2 lr steps (at most 2 % of
    them beyond 0.05 lr), loss rows to rtol 2e-4; Adam moments per tensor in relative L2."""
    p, m, v, log = res
    d = (p - whole.params.cpu()).abs()
    assert float(d.max()) <= 2.0 * LR * n_steps + 1e-6, (what, float(d.max()))
    assert int((d > 0.05 * LR).sum()) <= 0.02 * d.numel() + 2, (what, int((d > 0.05 * LR).sum()))
    assert torch.allclose(log[:n_steps, :3], whole.loss_log[:n_steps, :3].cpu(), rtol=2e-4, atol=1e-5), what
    lay = whole.layout
    errs = {}
    for name, mine, ref in (("m", m, whole.adam_m), ("v", v, whole.adam_v)):
        got, want = lay.unflatten(mine), lay.unflatten(ref.cpu())
        for key, w in want.items():
            if float(w.norm()) != 0.0:
                errs[(name, key)] = _rel_l2(got[key], w)
    worst = max(errs, key=errs.get)
    print(f"[{what}] worst per-tensor relative L2 of the Adam moments vs the whole-batch launch: {errs[worst]:.3e} {worst}")
    for key, e in errs.items():
        assert e <= moment_bound, (what, key, e)


def test_rowsplit_metric_shape_eight_steps_every_path():
    """SE-gPoE 3 x 379, 600 rows (at k = 4 the last batch's slices hold 64 / 24 / 0 / 0 rows), draws injected, 8 steps at
    k in {2, 4} x helpers in {0, auto}: one launch of 8 == 8 launches of 1 == helpers 0 == a second run, bit for bit
    (params, moments, loss log); against the whole-batch launch on the same batches; every step's reconstruction loss
    within 1e-4 of the bf16-operand oracle's own trajectory; and the shadow images the last sweep left (bf16 tiles, fp32
    vector pieces, published by hand-off D) equal the ones nm_sync_shadow rebuilds from the master.

    Adam moments vs the whole-batch launch, per-tensor relative L2: worst measured on the MI355X 2.1e-6 (k = 2) and 2.4e-6
    (k = 4), both alpha's m; bound 7e-6 (< 3x)."""
    case = Case(**METRIC)
    whole = case.job()
    nm.JobSet([whole]).train(N_STEPS, rowsplit=1, split=False)
    torch.cuda.synchronize()
    ref_ll = case.oracle_trajectory(N_STEPS)
    for k in (2, 4):
        runs = {}
        for mode in ("fused auto", "stepwise auto", "fused 0", "fused auto again"):
            job = case.job()
            js = nm.JobSet([job])
            h = 0 if mode == "fused 0" else None
            if mode.startswith("stepwise"):
                for _ in range(N_STEPS):
                    js.train(1, rowsplit=k, helpers=h)
            else:
                js.train(N_STEPS, rowsplit=k, helpers=h)
            _sync(js)
            runs[mode] = (_snapshot(job), job)
        base = runs["fused auto"][0]
        for mode, (snap, _) in runs.items():
            for a, b, t in zip(base, snap, ("params", "adam_m", "adam_v", "loss_log")):
                assert torch.equal(a, b), (k, mode, t, float((a - b).abs().max()))
        _assert_trajectory_vs_whole(base, whole, N_STEPS, 7e-6, f"k={k}")
        log = base[3]
        for s in range(N_STEPS):
            assert abs(float(log[s, 2]) - ref_ll[s]) <= 1e-4 * abs(ref_ll[s]), (k, s, float(log[s, 2]), ref_ll[s])
        # shadow images: a forward of the trained job (its images as the sweep left them) == a fresh job loaded from its
        # state_dict (images rebuilt from the master by nm_sync_shadow), bit for bit
        trained = runs["fused auto"][1]
        fresh = case.job(state=trained.state_dict())
        fresh.step, fresh.t = trained.step, trained.t
        outs = []
        for j in (trained, fresh):
            j.enable_exports(rowdev=False)
            nm.JobSet([j]).forward()
            torch.cuda.synchronize()
            outs.append(([x[:case.n_rows].cpu() for x in j.out_loc], [x[:case.n_rows].cpu() for x in j.out_sqerr],
                         j.out_mu[:case.n_rows].cpu()))
        for m in range(3):
            assert torch.equal(outs[0][0][m], outs[1][0][m]), (k, "out_loc", m)
            assert torch.equal(outs[0][1][m], outs[1][1][m]), (k, "out_sqerr", m)
        assert torch.equal(outs[0][2], outs[1][2]), (k, "out_mu")


def test_rowsplit_mixed_widths_uca():
    """UCA at full size -- 4 modalities, D = [379, 379, 379, 1137], gPoE -- so the modalities' sweep tables differ in size:
    gradients at k = 4 with helpers per element against the whole-batch launch and the oracle, then 3 train steps against
    the whole-batch launch (Adam moments, per-tensor relative L2: worst measured on the MI355X 9.2e-6, alpha's v; bound
    2.7e-5, < 3x)."""
    case = Case([379, 379, 379, 1137], n_rows=600, seed=14, n_eps=3)
    res = {mode: case.oracle_grads(mode) for mode in ("fp32", "bf16")}
    whole = case.job()
    whole.grads.fill_(float("nan"))
    nm.JobSet([whole]).grads(0)
    job = case.job()
    job.grads.fill_(float("nan"))
    js = nm.JobSet([job])
    js.grads(0, rowsplit=4)
    _sync(js)
    _assert_close_per_element(job.grads_dict(), whole.grads_dict(), "uca grads")
    _assert_vs_oracle(job, case, res)
    wtrain = case.job()
    nm.JobSet([wtrain]).train(3, rowsplit=1, split=False)
    tj = case.job()
    ts = nm.JobSet([tj])
    ts.train(3, rowsplit=4)
    _sync(ts)
    _assert_trajectory_vs_whole(_snapshot(tj), wtrain, 3, 2.7e-5, "uca")


def test_rowsplit_five_metric_models_bench_leg():
    """The bench's small-sweep leg at size: five 3 x 379 models (k = 4, 12 helpers each) == the same five without
    helpers == model 3 trained alone, bit for bit."""
    case = Case(**METRIC)

    def five():
        jobs = []
        for i in range(5):
            j = case.job()
            j.seed = i
            j.set_eps(None)
            jobs.append(j)
        return jobs

    a = five()
    sa = nm.JobSet(a)
    assert sa.rowsplit_k() == 4 and sa.rowsplit_helpers(4) == 12
    sa.train(4)
    _sync(sa)
    b = five()
    sb = nm.JobSet(b)
    sb.train(4, rowsplit=4, helpers=0)
    _sync(sb)
    alone = case.job()
    alone.seed = 3
    alone.set_eps(None)
    sl = nm.JobSet([alone])
    sl.train(4, rowsplit=4)
    _sync(sl)
    for x, y in zip(a, b):
        for p, q in zip(_snapshot(x), _snapshot(y)):
            assert torch.equal(p, q)
    for p, q in zip(_snapshot(a[3]), _snapshot(alone)):
        assert torch.equal(p, q)
    assert not torch.equal(a[3].params.cpu(), a[4].params.cpu())
