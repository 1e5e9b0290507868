"""GPU parity tests proper: the HIP path (through the C ABI of libnmhip.so) against the CPU
oracle and the committed golden vectors.

Tolerances.  The kernels compute every contraction with bf16 operands and fp32 accumulation
(north star: "MFMA bf16 GEMMs"), everything else in fp32:
  * reconstruction loss (LL):  <= 1e-4 relative  -- the tolerance BASELINE.json states
  * per-element activations / gradients: bf16 operand rounding, ~2^-9 relative per product ->
    a few 1e-3 of the tensor's max after accumulation; bounds below are ~3x the observed error
  * parameters after k Adam steps: Adam's update is ~lr*sign(g) early on, so a bf16-induced sign
    flip of a near-zero gradient moves a weight by up to 2*lr per step; bounded accordingly
  * ROI / row indexing: bit-exact (checked through exports addressed by absolute row and ROI)
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import multi_modal_normative_modeling_amd as nm
from multi_modal_normative_modeling_amd import _lib
from oracle import cvae_ref as R
from tests.golden_util import Golden
from tests.hip_harness import DEV, make_job, swap_batch, oracle_step0, rel_err

MM_CASES = ["mm1_small", "mm1_h1", "mm3_poe", "mm3_gpoe", "mm3_moe", "mm3_mopoe", "mm4_uca_gpoe", "mm2_z64",
            "cfgA_T1w", "cfgA_T1w_tail83"]


def bf(t):
    return t.bfloat16().float()


@pytest.mark.parametrize("mode", [0, 1, 2, 3])
def test_gemm_forms(mode):
    """The three MFMA GEMM forms of the kernel (fragment loaders + lane maps) on exact data."""
    lib = _lib.load()
    g = torch.Generator().manual_seed(mode)
    st = torch.cuda.current_stream().cuda_stream
    if mode == 0:
        M, N, K = 256, 110, 77
        A = bf(torch.randn(M, K, generator=g)); B = bf(torch.randn(N, K, generator=g))
        ref = A @ B.T
        out = torch.zeros(M, N, device=DEV)
    elif mode == 1:
        M, N, K = 256, 110, 39            # C[r][k] = sum_n A[r][n] B[n][k]
        A = bf(torch.randn(M, N, generator=g)); B = bf(torch.randn(N, K, generator=g))
        ref = A @ B
        out = torch.zeros(M, K, device=DEV)
    else:
        M, N, K = 256, 110, 111           # C[n][k] = sum_r A[r][n] B[r][k]
        A = bf(torch.randn(M, N, generator=g)); B = bf(torch.randn(M, K, generator=g))
        ref = A.T @ B
        out = torch.zeros(N, K, device=DEV)
    if mode in (0, 1):                    # weight operand in the flat-buffer format: 16 x 16 tiles, zero padded
        nt, kt = (B.shape[0] + 15) // 16, (B.shape[1] + 15) // 16
        Bp = torch.zeros(nt * 16, kt * 16)
        Bp[:B.shape[0], :B.shape[1]] = B
        B = Bp.view(nt, 16, kt, 16).permute(0, 2, 1, 3).contiguous()
    Ad, Bd = A.to(DEV).contiguous(), B.to(DEV).contiguous()
    _lib.check(lib.nm_test_gemm(mode, Ad.data_ptr(), Bd.data_ptr(), out.data_ptr(), M, N, K, st))
    torch.cuda.synchronize()
    err = rel_err(out.cpu(), ref)
    assert err < 2e-6, err               # bf16-exact inputs, fp32 accumulate: only summation order differs


def rel_l2(a, r):
    return float((a - r).norm()) / (float(r.norm()) + 1e-30)


def oracle_in_mode(g, mode):
    R.set_operand_rounding(mode)
    try:
        return oracle_step0(g)
    finally:
        R.set_operand_rounding("fp32")


@pytest.mark.parametrize("name", MM_CASES)
def test_forward_loss_and_grads(name):
    """One forward+backward of the HIP path against
      (a) the reference's own fp32 numbers (golden): north-star bound on the reconstruction loss,
          bf16-operand tolerance on tensors, direction/size of every gradient;
      (b) the oracle restated with bf16 GEMM operands (the arithmetic the kernel is specified to
          do): tight agreement -- only fp32 summation order differs.
    LeakyReLU makes the gradient discontinuous in the pre-activations, so (a) sees isolated
    sign flips; max-abs gradient errors are therefore checked only in (b)."""
    g = Golden(name)
    job = make_job(g, 0)
    job.enable_exports()
    js = nm.JobSet([job])
    js.grads(0)
    torch.cuda.synchronize()
    fwd16, loss16, grads16 = oracle_in_mode(g, "bf16")
    _, _, grads32 = oracle_in_mode(g, "fp32")
    B = g.B
    mu = job.out_mu[:B].cpu()
    lv = job.out_logvar[:B].cpu()
    assert rel_err(mu, g.t("mu")) < 2e-2
    assert rel_err(lv, g.t("logvar")) < 2e-2
    assert rel_err(mu, fwd16["mu"].detach()) < 2e-3
    assert rel_err(lv, fwd16["logvar"].detach()) < 2e-3
    for m in range(g.M):
        loc = job.out_loc[m][:B].cpu()
        assert rel_err(loc, g.t(f"loc{m}")) < 2e-2, m
        assert rel_err(loc, fwd16["locs"][m].detach()) < 2e-3, m
        # exports are addressed by absolute row / ROI: consistent with the fp32 inputs => indexing exact
        x = g.xs(0)[m]
        np.testing.assert_allclose(job.out_sqerr[m][:B].cpu().numpy(), ((x - loc) ** 2).numpy(), rtol=1e-5, atol=1e-7)
        np.testing.assert_allclose(job.out_rowdev[m][:B].cpu().numpy(), ((x - loc) ** 2).sum(1).numpy() / x.shape[1],
                                   rtol=1e-4, atol=1e-7)
    row = job.loss_log[0].cpu()
    ref = g.z["loss0"]                                   # total, kl, ll from the reference itself
    assert abs(float(row[2]) - ref[2]) <= 1e-4 * abs(ref[2]), ("ll", float(row[2]), ref[2])      # north star
    assert abs(float(row[0]) - ref[0]) <= 1e-4 * abs(ref[0]), ("total", float(row[0]), ref[0])
    assert abs(float(row[1]) - ref[1]) <= 5e-3 * abs(ref[1]) + 1e-5, ("kl", float(row[1]), ref[1])
    assert abs(float(row[2]) - float(loss16["ll"])) <= 2e-6 * abs(ref[2])
    assert abs(float(row[1]) - float(loss16["kl"])) <= 1e-4 * abs(ref[1]) + 1e-6
    got = job.grads_dict()
    for k in got:
        a, r32, r16 = got[k].flatten(), grads32[k].flatten(), grads16[k].flatten()
        if float(r32.abs().max()) == 0.0:                # e.g. alpha when the combiner ignores it
            assert float(a.abs().max()) == 0.0, k
            continue
        assert rel_l2(a, r16) < 5e-3, (k, "bf16-oracle", rel_l2(a, r16))      # (measured <= 4e-4 on every case)
        assert rel_l2(a, r32) < 0.15, (k, "fp32", rel_l2(a, r32))
        if a.numel() >= 8:
            cos = float(torch.nn.functional.cosine_similarity(a, r32, dim=0))
            assert cos > 0.99, (k, cos)
        if B <= 48:                                      # short contractions: summation order rarely flips a sign
            assert rel_err(a, r16) < 2e-3, (k, rel_err(a, r16))


@pytest.mark.parametrize("name", ["mm1_small", "mm3_gpoe", "mm2_z64"])
def test_tr_read_matches_scalar_loader(name):
    """ds_read_b64_tr_b16 wgrad operands == scalar LDS loader, bit for bit."""
    g = Golden(name)
    out = []
    for scalar in (False, True):
        job = make_job(g, 0)
        js = nm.JobSet([job])
        js.grads(0, export=False, scalar_tr=scalar)
        torch.cuda.synchronize()
        out.append(job.grads.cpu().clone())
    assert torch.equal(out[0], out[1])


@pytest.mark.parametrize("name", MM_CASES)
def test_adam_trajectory(name):
    """n fused train steps (fwd + ELBO + bwd + Adam inside the kernel) against the reference's own
    trajectory (golden, fp32) and against the oracle with bf16 GEMM operands."""
    g = Golden(name)
    job = make_job(g, 0)
    js = nm.JobSet([job])
    lr = 1e-4
    rs = R.Spec(g.dims, g.hidden, g.Z, g.c_dim)
    P16 = g.weights("w0")
    opt16 = R.Adam(P16, R.param_names(rs), lr=lr)
    for s in range(g.n_steps):
        if s > 0:
            swap_batch(job, g, s)
        js.train(1)
        torch.cuda.synchronize()
        R.set_operand_rounding("bf16")
        try:
            R.train_step(P16, opt16, rs, g.xs(s), [g.t("c")[s].long()] * g.M, g.combine, g.t("eps")[s])
        finally:
            R.set_operand_rounding("fp32")
        sd16 = job.state_dict()
        n_tot = sum(v.numel() for v in P16.values())
        n_off = sum(int(((sd16[k] - P16[k]).abs() > 0.05 * lr).sum()) for k in P16)
        assert n_off <= 0.02 * (s + 1) * n_tot + 2, ("bf16-oracle", s, n_off, n_tot)
        # Adam's moments against the oracle that does the kernel's arithmetic (bf16 GEMM operands, fp32 everything else):
        # measured <= 1.3e-3 relative L2 on every tensor of every case and step (the bounds against the fp32 reference
        # below are 0.15 / 0.30 -- that distance is the operand rounding, not the kernel)
        m16, v16 = job.adam_dicts()
        for k in opt16.m:
            if float(opt16.m[k].abs().max()) == 0.0 or opt16.m[k].numel() < 8:
                continue
            assert rel_l2(m16[k], opt16.m[k]) < 5e-3, ("bf16-oracle exp_avg", k, s)
            assert rel_l2(v16[k], opt16.v[k]) < 1e-2, ("bf16-oracle exp_avg_sq", k, s)
        row = job.loss_log[0].cpu()
        ref = g.z[f"loss{s}"]
        assert abs(float(row[2]) - ref[2]) <= 1e-4 * abs(ref[2]), (s, float(row[2]), ref[2])
        wref = g.weights(f"w{s + 1}")
        if wref:
            sd = job.state_dict()
            n_tot = n_bad = 0
            for k, v in wref.items():
                d = (sd[k] - v).abs()
                assert float(d.max()) <= 2.0 * lr * (s + 1) + 1e-6, (k, s, float(d.max()))
                n_tot += d.numel()
                n_bad += int((d > 0.25 * lr).sum())
            assert n_bad <= (0.03 + 0.01 * s) * n_tot + 2, (n_bad, n_tot)
            mref, vref = g.adam(f"a{s + 1}")
            m_hip, v_hip = job.adam_dicts()
            for k in mref:
                if float(mref[k].abs().max()) == 0.0 or mref[k].numel() < 8:
                    continue
                assert rel_l2(m_hip[k], mref[k]) < 0.15, k
                assert rel_l2(v_hip[k], vref[k]) < 0.30, k


def test_multi_step_single_launch_equals_stepwise():
    """n steps in ONE persistent launch == n launches of one step (same batches, same draws)."""
    g = Golden("mm1_small")
    xs = torch.cat([g.xs(s)[0] for s in range(g.n_steps)])          # 5 x 19 rows -> one 95-row table
    # use a table of 600 rows so that batches are 256, 256, 88 (ragged tail) and several epochs wrap
    reps = 7
    x = torch.cat([xs] * reps)[:600]
    c = torch.cat([g.t("c")[s] for s in range(g.n_steps)] * reps)[:600]
    eps = torch.randn(7, 256, g.Z, generator=torch.Generator().manual_seed(5))
    res = []
    for mode in ("fused", "stepwise"):
        spec = nm.ModelSpec(g.dims, g.hidden, g.Z, g.c_dim)
        job = nm.Job(spec, [nm.Table(x, c, DEV)], combine=g.combine, state=g.weights("w0"))
        job.set_eps(eps)
        js = nm.JobSet([job])
        if mode == "fused":
            js.train(7)
        else:
            for _ in range(7):
                js.train(1)
        torch.cuda.synchronize()
        res.append((job.params.cpu().clone(), job.loss_log[:7].cpu().clone(), job.adam_m.cpu().clone(), job.adam_v.cpu().clone()))
    for a, b, what in zip(res[0], res[1], ("params", "loss_log", "adam_m", "adam_v")):
        assert torch.equal(a, b), what


def test_many_jobs_one_launch_are_independent():
    """A set of jobs in one launch gives each job exactly what it gets alone."""
    g = Golden("mm3_gpoe")
    alone = make_job(g, 0)
    nm.JobSet([alone]).train(1)
    jobs = [make_job(g, 0) for _ in range(5)]
    other = Golden("mm1_small")
    jobs.insert(2, make_job(other, 0))
    nm.JobSet(jobs).train(1)
    torch.cuda.synchronize()
    for j in (jobs[0], jobs[1], jobs[3], jobs[5]):
        assert torch.equal(j.params.cpu(), alone.params.cpu())


def test_deviation_passes():
    """(i) unimodal sampled-z deviation of the regression script; (ii) joint pred_recon."""
    g = Golden("dev_small")
    N = g.B
    P = g.weights("w0")
    xs = g.xs()
    spec_full = nm.ModelSpec(g.dims, g.hidden, g.Z, g.c_dim)
    full_layout = nm.ParamLayout(spec_full)
    for m in range(g.M):
        # single-modality view of the same weights (encode(x, c, m) / decode(z, c, m))
        spec1 = nm.ModelSpec([g.dims[m]], g.hidden, g.Z, g.c_dim)
        st = {}
        for k in nm.ParamLayout(spec1).names:
            src = k.replace("_list.0.", f"_list.{m}.")
            st[k] = P[src]
        job = nm.Job(spec1, [nm.Table(xs[m], g.t("c_raw"), DEV)], combine="poe", state=st)
        job.set_eps(g.t("eps_uni")[m])
        job.enable_exports()
        nm.JobSet([job]).forward()
        torch.cuda.synchronize()
        ref = torch.from_numpy(g.z[f"uni_dev{m}"])
        got = job.out_sqerr[0][:N].cpu()
        # squared residual of O(1) residuals with ~1e-3 absolute error in x_hat
        assert float((got - ref).abs().max()) < 2e-2 * float(ref.max()), m
        assert rel_err(job.out_loc[0][:N].cpu(), torch.from_numpy(g.z[f"uni_loc{m}"])) < 2e-2
        # the bound that carries weight: the distance between the reference's fp32 numbers and the oracle with bf16
        # GEMM operands (the arithmetic the kernel is specified to do) is the scale of the allowed error
        rs1 = R.Spec([g.dims[m]], g.hidden, g.Z, g.c_dim)
        R.set_operand_rounding("bf16")
        try:
            loc16 = R.forward_multimodal(st, rs1, [xs[m]], [g.t("c_raw")], "poe", g.t("eps_uni")[m])["locs"][0].detach()
        finally:
            R.set_operand_rounding("fp32")
        sq16 = (xs[m] - loc16) ** 2
        noise = float((sq16 - ref).abs().max())
        assert float((got - sq16).abs().max()) <= 1.5 * noise + 1e-5, (m, float((got - sq16).abs().max()), noise)
        assert float((got - ref).abs().max()) <= 3.0 * noise + 1e-5, m
    job = nm.Job(spec_full, [nm.Table(xs[m], g.t("c_onehot"), DEV) for m in range(g.M)], combine=g.combine, state=P)
    job.set_eps(g.t("eps_joint"))
    job.enable_exports()
    nm.JobSet([job]).forward()
    torch.cuda.synchronize()
    for m in range(g.M):
        assert rel_err(job.out_loc[m][:N].cpu(), torch.from_numpy(g.z[f"joint_pred{m}"])) < 2e-2
        ref = torch.from_numpy(g.z[f"joint_dev{m}"]).float()
        assert float((job.out_rowdev[m][:N].cpu() - ref).abs().max()) < 1e-2 * float(ref.max())


@pytest.mark.parametrize("name", ["mm3_gpoe", "mm3_poe", "mm3_moe", "mm3_mopoe", "mm4_uca_gpoe", "mm2_z64"])
def test_split_launch_equals_single_workgroup_bit_for_bit(name):
    """nm_launch_split (one workgroup per modality, two hand-offs per step) against the one-workgroup launch: the
    same gradients, and after 4 fused Adam steps the same parameters, moments and loss log, bit for bit."""
    g = Golden(name)
    out = []
    for split in (False, True):
        job = make_job(g, 0)
        js = nm.JobSet([job])
        js.grads(0, export=False, split=split)
        torch.cuda.synchronize()
        grads = job.grads.cpu().clone()
        js.train(4, split=split)
        torch.cuda.synchronize()
        out.append((grads, job.params.cpu().clone(), job.adam_m.cpu().clone(), job.adam_v.cpu().clone(),
                    job.loss_log.cpu().clone()))
    for a, b, what in zip(out[0], out[1], ("grads", "params", "adam_m", "adam_v", "loss_log")):
        assert torch.equal(a, b), (what, float((a - b).abs().max()))


def test_split_launch_many_small_models_and_refusal():
    """Twenty 3-modality models as 3 workgroups each (the reference's real sweep width, 5 folds x 4 procedures):
    identical to the one-workgroup launch; a set that cannot be resident all at once is refused."""
    g = Golden("mm3_gpoe")
    res = []
    for split in (False, True):
        jobs = [make_job(g, 0) for _ in range(20)]
        for i, j in enumerate(jobs):
            j.seed = i
            j.set_eps(None)                       # in-kernel draw, keyed by (seed, step, row, z)
        js = nm.JobSet(jobs)
        js.train(3, split=split)
        torch.cuda.synchronize()
        res.append(torch.stack([j.params for j in jobs]).cpu())
    assert torch.equal(res[0], res[1])
    assert not torch.equal(res[0][0], res[0][1])          # different draws -> different models
    lib = _lib.load()
    big = nm.JobSet([make_job(g, 0) for _ in range(96)])  # 96 x 3 = 288 workgroups > 256 CUs
    ptr = big._upload(1)
    st = torch.cuda.current_stream().cuda_stream
    assert lib.nm_launch_split(ptr, 96, 3, 0, 1, _lib.NM_F_BACKWARD | _lib.NM_F_GRADS, st) == _lib.NM_E_RESIDENCY
    assert big.split_parts() == 1


def test_per_step_learning_rate_table_matches_oracle():
    """The cyclic schedule of multimodal_kfold_cvae_nmmlp.py:376-381 as nm_job_t.lr_table: 6 fused Adam steps with a
    different learning rate each, against the oracle stepping with the same rates (bf16-operand mode), and against a
    constant-rate run (must differ)."""
    from multi_modal_normative_modeling_amd import prep as P_
    g = Golden("mm3_gpoe")
    lrs = P_.cyclic_lr(6, 512, 256, 1e-5, 4e-4, 0.9)
    assert len(set(lrs.tolist())) >= 4          # triangular: rises for 4 steps, then retraces
    job = make_job(g, 0)
    job.set_lr_table(lrs)
    js = nm.JobSet([job])
    const = make_job(g, 0)
    cj = nm.JobSet([const])
    rs = R.Spec(g.dims, g.hidden, g.Z, g.c_dim)
    Pw = {k: v.clone() for k, v in g.weights("w0").items()}
    opt = R.Adam(Pw, R.param_names(rs))
    xes, c, eps = g.xs(0), g.t("c")[0], g.t("eps")[0]
    R.set_operand_rounding("bf16")
    try:
        for i in range(6):
            opt.lr = float(lrs[i])
            R.train_step(Pw, opt, rs, xes, [c.long()] * g.M, g.combine, eps)
    finally:
        R.set_operand_rounding("fp32")
    js.train(6); cj.train(6)
    torch.cuda.synchronize()
    got, cst = job.state_dict(), const.state_dict()
    moved = max(float((got[k] - g.weights("w0")[k]).abs().max()) for k in got)
    worst = max(float((got[k] - Pw[k]).abs().max()) for k in got)
    assert worst <= 0.05 * moved + 1e-7, (worst, moved)         # same trajectory as the oracle under the same schedule
    assert max(float((got[k] - cst[k]).abs().max()) for k in got) > 0.2 * moved      # and not the constant-rate one
