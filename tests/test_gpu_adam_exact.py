"""Every fused Adam update pinned to its own gradient, element by element (tests/adam_check.py holds the bounds and where
they come from).

For ONE optimizer step the test takes p, m, v (and the bf16 shadow images) before, g from a gradient launch at that state
-- the kernels store the gradient they consume at the same flat index as the parameter -- and p', m', v' after train(1) in
the SAME form of the launch, pinned explicitly.  assert_adam_step then holds every element of the flat buffers, tile
padding and alignment gaps included, to fp32 Adam on those inputs: m' to 2 eps (|m| + |g|), v' to 4 eps v' + 2^-126, p' to
2 eps |p'| + 12 eps |u| (eps = 2^-24), untouched elements (g = m = v = 0) bit for bit.  The gradient launch itself must leave
parameters, moments and shadow images as they were.  After the steps: every element that belongs to no tensor is exactly
zero in all three buffers, and the shadow images equal what nm_sync_shadow rebuilds from the master, byte for byte.

Together with the bit-for-bit tests (a multi-step launch == stepwise, split / row-split / head-split == one workgroup) and
the gradient's own comparison with the oracle this closes the chain: each single step is Adam on the gradient it consumed.

  a. nm_adam_step (the flat kernel behind the eager classes), n in {1, 255, 256, 4099, 1 000 003}, t in {1, 2, 1000},
     gradients with exact zeros, 1e-30 and 1e15 entries.
  b. 8 isolated steps on every training form -- whole, scalar_tr, split, rowsplit 2 / 4 with 0, 3 and the default number of
     helpers, the general-shape path -- on six goldens (a fresh batch per step), six fuzz shapes over a 531-row table
     (walking batch index, ragged 19-row tail), two general-shape fuzz shapes, the full size 3 x 379 / [110, 110] / B = 256,
     mvtCAE and the DMVAE family from the zoo (partly private, all private, learnable loss weights), and 3 steps on the general-shape path at its limits (W1, W3, W4 of tests/grad_check.py: width
     4096 with latent 128, the block boundaries, eight layers).  A mixed set (one- and three-modality model in one launch) runs the mixed row-split entry:
     grads() drives it whenever the set's modality counts differ.
  c. the flat-buffer invariants above, after those 8 steps.
  d. optimizer step 1001.. (job.t = 1000) and the cyclic learning-rate table: the checker is given t and the step's rate.
  e. head models: grads_head(s) then train_regression(1) / train_endtoend(1), dropout 0 and 0.5, whole and one workgroup
     per decoder, trunk and head parameters alike.  The BatchNorm running statistics live in `params` but are no optimizer
     parameters: they must carry no gradient and no moment (`frozen`); their values are BatchNorm's business.
  f. NM_F_ADAM | NM_F_GRADS in one launch (the C ABI accepts the pair; Python never sends it): job.grads equal to the
     gradient launch's and p', m', v' equal to train(1)'s, bit for bit.

Result on the MI355X: every element of every form inside its bound, the flag pair included; no kernel was changed.  Worst
error / bound per form (m' / v' / p'; 1.0 = at the bound; the CPU emulation peaks at 0.51 / 0.63 / 0.51):
    flat kernel 0.25 / 0.50 / 0.50      whole 0.46 / 0.69 / 0.50          scalar_tr 0.46 / 0.69 / 0.50
    split 0.46 / 0.69 / 0.50            row-split 2 0.45 / 0.71 / 0.50    row-split 4 0.46 / 0.73 / 0.50   (any helpers)
    general-shape 0.47 / 0.68 / 0.50    head models, whole and split, 0.46 / 0.69 / 0.50
The DMVAE-family jobs (whole, scalar_tr, split) lie inside the same figures: the learnable weights move on their own
gradient, an all-private fc_logvar keeps every bit.
(p' sits at 0.50: the half-ulp rounding of p' itself is 1 eps |p'| of the 2 eps allowed.)  The module prints the table of
the run at hand when it finishes (pytest -s).
"""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import multi_modal_normative_modeling_amd as nm
from multi_modal_normative_modeling_amd import _lib, engine, prep
from multi_modal_normative_modeling_amd.layout import rowsplit_fits
from tests import adam_check as A
from tests.golden_util import Golden
from tests.hip_harness import DEV, make_job, swap_batch
from tests.test_gpu_fullsize import onehot
from tests.test_gpu_fuzz import _draw, _draw_wide
from tests.test_gpu_head_split import baseline_job, golden_job

N_STEPS = 8
_WORST = {}


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    print("\n[adam exact] worst error / bound per form (m', v', p'):")
    for form, w in sorted(_WORST.items()):
        print(f"[adam exact]   {form:<12} {w[0]:.3f} {w[1]:.3f} {w[2]:.3f}")


def _note(form, r):
    w = _WORST.setdefault(form, [0.0, 0.0, 0.0])
    for i, k in enumerate(("m", "v", "p")):
        w[i] = max(w[i], r[k])


# ---- a: the flat kernel ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("t", [1, 2, 1000])
@pytest.mark.parametrize("n", [1, 255, 256, 4099, 1_000_003])
def test_flat_kernel(n, t):
    rng = np.random.default_rng(n + t)
    F = np.float32
    g = (rng.standard_normal(n) * 10.0 ** rng.integers(-3, 4, n)).astype(F)
    if n > 1:
        g[0::5] = 0
        g[1::5] = 1e-30
        g[2::5] = 1e15
    p = (rng.standard_normal(n) * 0.1).astype(F)
    if t == 1:
        m, v = np.zeros(n, F), np.zeros(n, F)
    else:
        m = (0.3 * np.abs(g) * rng.standard_normal(n)).astype(F)
        v = (g.astype(np.float64) ** 2 * rng.uniform(0.05, 1.0, n)).astype(F)
        m[3::10] = 0
        v[3::10] = 0
    for lr in (1e-4, 1e-3):
        before = tuple(torch.from_numpy(a.copy()) for a in (p, m, v))
        dev = [b.to(DEV) for b in before]
        gd = torch.from_numpy(g).to(DEV)
        engine.adam_step(dev[0], gd, dev[1], dev[2], t, lr=lr, betas=(0.9, 0.999), eps=1e-8)
        torch.cuda.synchronize()
        assert torch.equal(gd.cpu(), torch.from_numpy(g))
        r = A.assert_adam_step(before, torch.from_numpy(g), tuple(d.cpu() for d in dev), t, lr, (0.9, 0.999), 1e-8,
                               what=f"nm_adam_step n={n} t={t}")
        print(f"[adam exact] flat n={n} t={t} lr={lr}: {r}")
        _note("flat", r)


# ---- b, c: one step, isolated, on every training form -----------------------------------------------------------------
FORMS = {
    "whole": dict(split=False, rowsplit=1),
    "scalar_tr": dict(scalar_tr=True, split=False, rowsplit=1),
    "split": dict(split=True, rowsplit=1),
    "rs2": dict(rowsplit=2), "rs2_h0": dict(rowsplit=2, helpers=0), "rs2_h3": dict(rowsplit=2, helpers=3),
    "rs4": dict(rowsplit=4), "rs4_h0": dict(rowsplit=4, helpers=0), "rs4_h3": dict(rowsplit=4, helpers=3),
}
RS_FORMS = [f for f in FORMS if f.startswith("rs")]


def forms_for(M, wide=False, rowsplit=True, split=True):
    if wide:
        return ["whole"]                           # the general-shape path has the one form
    return ["whole", "scalar_tr"] + (["split"] if M > 1 and split else []) + (RS_FORMS if rowsplit else [])


def _state(job):
    return tuple(t.detach().cpu().clone() for t in (job.params, job.adam_m, job.adam_v))


def _frozen(job):
    names = [n for n in job.layout.names if "running" in n]
    if not names:
        return None
    fr = torch.zeros(job.layout.total, dtype=torch.bool)
    for n in names:
        o = job.layout.offsets[n]
        fr[o:o + job.layout.numel(n)] = True
    return fr.numpy()


def _rate(job, t):
    return float(job.lr) if job.lr_table is None else float(job.lr_table[(t - 1) % job.lr_table.numel()])


def isolated_steps(js, form, what, n_steps=N_STEPS, next_batch=None, grads=None, train=None, label=None):
    """n_steps times: state before; gradient launch; state unchanged; train(1) in the same form; assert_adam_step on every
    job of the set.  Then the flat-buffer invariants."""
    kw = FORMS.get(form, {})
    label = label or form
    grads = grads or (lambda s: js.grads(s, export=False, **kw))
    train = train or (lambda: js.train(1, **kw))
    js._upload()                                               # (a fresh job's shadow images are built before its first launch)
    for i in range(n_steps):
        if next_batch is not None:
            next_batch(i)
        s = js.jobs[0].step
        torch.cuda.synchronize()
        before = [_state(j) for j in js.jobs]
        shadow = [j._wsh.clone() for j in js.jobs]
        grads(s)
        js.check_split_errors(block=True)
        torch.cuda.synchronize()
        g = [j.grads.detach().cpu().clone() for j in js.jobs]
        for j, b, sh in zip(js.jobs, before, shadow):          # a gradient launch changes no state
            for name, x, y in zip(("params", "adam_m", "adam_v"), _state(j), b):
                assert torch.equal(x, y), (what, i, f"the gradient launch changed {name}")
            assert torch.equal(j._wsh, sh), (what, i, "the gradient launch changed the shadow images")
        ts = [j.t + 1 for j in js.jobs]
        train()
        js.check_split_errors(block=True)
        torch.cuda.synchronize()
        for k, j in enumerate(js.jobs):
            assert float(g[k].abs().max()) > 0.0
            r = A.assert_adam_step(before[k], g[k], _state(j), ts[k], _rate(j, ts[k]), j.betas, j.adam_eps, layout=j.layout,
                                   frozen=_frozen(j), what=f"{what} [{form}] job {k} step {i}")
            assert r["moved"] > 0.2 * j.layout.n_params, (what, i, r)          # the launch did train
            print(f"[adam exact] {what} [{form}] job {k} step {i} t={ts[k]}: m' {r['m']:.3f} v' {r['v']:.3f} p' {r['p']:.3f} "
                  f"moved {r['moved']} idle {r['idle']} of {r['n']}")
            _note(label, r)
    invariants(js, what + f" [{form}]")


def invariants(js, what):
    """(c) No element outside every tensor ever leaves zero; the shadow images are the master's."""
    torch.cuda.synchronize()
    for k, j in enumerate(js.jobs):
        gap = ~A.tensor_mask(j.layout)
        assert int(gap.sum()) > 0
        for name, buf in (("params", j.params), ("adam_m", j.adam_m), ("adam_v", j.adam_v)):
            bits = buf.detach().cpu().view(torch.int32)
            bad = (gap & (bits != 0)).nonzero().flatten()
            assert bad.numel() == 0, (what, k, name, f"{bad.numel()} pad elements left zero, first at flat index "
                                      f"{int(bad[0])} = {A.locate(j.layout, int(bad[0]))}")
    snaps = [j._wsh.clone() for j in js.jobs]
    for j in js.jobs:
        j.shadow_dirty = True
    js._upload()                                               # nm_sync_shadow rebuilds the images from the fp32 master
    torch.cuda.synchronize()
    for k, (j, snap) in enumerate(zip(js.jobs, snaps)):
        diff = (j._wsh != snap).nonzero().flatten()
        assert diff.numel() == 0, (what, k, f"shadow image differs from the master's in {diff.numel()} bytes, first at {int(diff[0])}")


GOLDENS = ["mm1_h1", "mm3_gpoe", "mm3_poe", "mm4_uca_gpoe", "mm2_z64", "cfgA_T1w_tail83"]
GOLDEN_M = {"mm1_h1": 1, "mm3_gpoe": 3, "mm3_poe": 3, "mm4_uca_gpoe": 4, "mm2_z64": 2, "cfgA_T1w_tail83": 1}


def golden_run(name, form, t0=None, lr_table=None):
    g = Golden(name)
    assert g.M == GOLDEN_M[name]
    job = make_job(g, 0)
    if t0 is not None:
        job.t = t0
        job.touch()
    if lr_table is not None:
        job.set_lr_table(lr_table)
    js = nm.JobSet([job])
    isolated_steps(js, form, name, next_batch=lambda i: swap_batch(job, g, i % g.n_steps))
    return job


@pytest.mark.parametrize("name,form", [(n, f) for n in GOLDENS for f in forms_for(GOLDEN_M[n])])
def test_golden_shapes(name, form):
    """A fresh batch per step (swap_batch); mm3_poe: the alpha gradient is exactly zero, alpha must not move."""
    job = golden_run(name, form)
    assert job.t == N_STEPS
    if name == "mm3_poe":
        g = Golden(name)
        for m in range(g.M):
            assert torch.equal(job.state_dict()[f"alpha_m_list.{m}"], g.weights("w0")[f"alpha_m_list.{m}"])


def table_job(dims, hidden, Z, c_dim, combine, non_linear, N, seed, kind="multimodal"):
    gen = torch.Generator().manual_seed(seed)
    spec = nm.ModelSpec(list(dims), list(hidden), Z, c_dim, non_linear, kind)
    P = nm.ParamLayout(spec).init_reference_rule(seed)
    xs = [torch.randn(N, d, generator=gen) * 1.2 for d in dims]
    c = onehot(gen, N, c_dim)
    job = nm.Job(spec, [nm.Table(x, c, DEV) for x in xs], combine=combine, state=P)
    job.set_eps(torch.randn(N_STEPS, 256, Z, generator=gen))
    return job


def _fuzz_spec(seed):
    dims, Z, combine, _, hidden, c_dim, non_linear = _draw(seed)
    return nm.ModelSpec(list(dims), list(hidden), Z, c_dim, non_linear)


FUZZ = [(s, f) for s in range(6) for f in forms_for(len(_fuzz_spec(s).input_dims), rowsplit=rowsplit_fits(_fuzz_spec(s)))]


@pytest.mark.parametrize("seed,form", FUZZ)
def test_fuzz_shapes_walking_batches(seed, form):
    """Six shapes of test_gpu_fuzz._draw on a 531-row table: batches of 256, 256 and 19 rows, the batch index walking."""
    dims, Z, combine, _, hidden, c_dim, non_linear = _draw(seed)
    job = table_job(dims, hidden, Z, c_dim, combine, non_linear, 531, seed)
    assert job.batches_per_epoch == 3 and not job.spec.wide
    isolated_steps(nm.JobSet([job]), form, f"fuzz {seed} {dims} {hidden} Z={Z} {combine}")
    assert job.step == N_STEPS


@pytest.mark.parametrize("seed", [0, 1])
def test_general_shape_path(seed):
    """Two shapes of the general-shape fuzz over a 531-row table."""
    dims, Z, combine, _, hidden, c_dim, non_linear = _draw_wide(seed)
    job = table_job(dims, hidden, Z, c_dim, combine, non_linear, 531, seed)
    assert job.spec.wide
    isolated_steps(nm.JobSet([job]), "whole", f"wide {seed} {dims} {hidden} Z={Z} {combine}", label="general")


@pytest.mark.parametrize("cid", ["W1", "W3", "W4"])
def test_general_shape_path_at_limits(cid):
    """The cases of tests/test_gpu_grad_exact.py at the path's limits (W1: width 4096 and latent 128; W3: the block
    boundaries, latent 65; W4: eight layers): there the update is pinned to the very gradient that module pins to the
    oracle.  Three steps, not eight: a case carries ONE batch of draws, so every step sees the same data and only the Adam
    state moves on -- first step (zero moments), second and third (bias corrections, moments in use) are the distinct
    states; and the fp64 restatement of W1's flat buffers takes its time per step.  (W2 is left out: the restatement of
    its 2 x 4096 x 4096 buffers is slow.)"""
    from tests import grad_check as G
    job = G.data(cid).job(True, DEV)
    job.grads.zero_()
    assert job.spec.wide
    isolated_steps(nm.JobSet([job]), "whole", f"wide {cid}", n_steps=3, label="general")
    G.clear_cache()


@pytest.mark.parametrize("form", forms_for(3))
def test_full_size(form):
    """3 x 379 ROI, hidden [110, 110], B = 256, 29 covariates."""
    job = table_job([379, 379, 379], [110, 110], 10, 29, "gpoe", True, 256, 11)
    isolated_steps(nm.JobSet([job]), form, "3x379")


@pytest.mark.parametrize("form", ["whole", "split"])
def test_zoo_mvtcae(form):
    """mvtCAE (variance clamp, total-correlation term, its own fusion rule): the same Adam behind another loss."""
    job = table_job([40, 55, 33], [32, 24], 6, 5, "poe", True, 300, 5, kind="mvtcae")
    isolated_steps(nm.JobSet([job]), form, "mvtCAE")


ZOO_DM = {"private 4 of 12": ("dmvae", 4), "all private": ("dmvae", 29), "weighted": ("weighted_dmvae", 4)}


@pytest.mark.parametrize("form", ["whole", "scalar_tr", "split"])
@pytest.mark.parametrize("which", list(ZOO_DM))
def test_zoo_dm(which, form):
    """The DMVAE family (ReLU, sigmoid output, private latent columns, learnable loss weights) over a 300-row table, in
    every form the library admits for it: whole, scalar_tr and split (one workgroup per modality).  The row-split launch
    and the plain-training instantiation refuse these kinds -- asked of Job.rowsplit_ok / nm_rowsplit_ok and Job.plain_ok
    / nm_plain_ok below, and of JobSet, whose automatic pick stays at one slice -- and the general-shape path has the one
    form that test_general_shape_path covers.  The learnable `weights` are updated by Adam on their own gradient like every
    other element (assert_adam_step covers the whole flat buffer) and do move; with every column private no element of
    any fc_logvar ever sees a gradient, a moment or a changed bit."""
    kind, c_dim = ZOO_DM[which]
    dims, hidden, Z, N = [61, 90, 47], [64, 48], 12, 300
    gen = torch.Generator().manual_seed(23)
    spec = nm.ModelSpec(dims, hidden, Z, c_dim, True, kind)
    P = nm.ParamLayout(spec).init_reference_rule(23)
    if kind == "weighted_dmvae":
        P["weights"] = torch.tensor([0.8, 1.1, 1.3])
    job = nm.Job(spec, [nm.Table(torch.rand(N, d, generator=gen), torch.zeros(N, 0), DEV) for d in dims], combine="poe", state=P)
    job.set_eps(torch.randn(N_STEPS, 256, Z, generator=gen))
    js = nm.JobSet([job])
    st = job.struct()
    assert not job.spec.wide and job.batches_per_epoch == 2
    assert not job.rowsplit_ok() and js.lib.nm_rowsplit_ok(C.byref(st)) != 0 and js.rowsplit_k() == 1
    assert not job.plain_ok() and js.lib.nm_plain_ok(C.byref(st)) != 0
    before = job.params.detach().cpu().clone()
    lay = job.layout

    def flat(name):
        n = lay.tiles[name][0] * lay.tiles[name][1] * 256 if name in lay.tiles else lay.numel(name)
        return slice(lay.offsets[name], lay.offsets[name] + n)

    seen_weight_grads = []
    if kind == "weighted_dmvae":
        grads = lambda s: (js.grads(s, export=False, **FORMS[form]), seen_weight_grads.append(job.grads[flat("weights")].cpu().clone()))
    else:
        grads = None
    isolated_steps(js, form, f"zoo {which}", grads=grads)
    assert job.t == N_STEPS
    after = job.params.detach().cpu()
    if kind == "weighted_dmvae":
        assert all(bool((g != 0).all()) for g in seen_weight_grads) and len(seen_weight_grads) == N_STEPS
        assert bool((after[flat("weights")] != before[flat("weights")]).all())          # each weight is learned
    if c_dim >= Z:
        for m in range(len(dims)):
            for t in ("weight", "bias"):
                sl = flat(f"encoder_list.{m}.fc_logvar.{t}")
                for buf in (job.grads, job.adam_m, job.adam_v):
                    assert not bool(buf[sl].cpu().view(torch.int32).any()), (m, t)
                assert torch.equal(after[sl].view(torch.int32), before[sl].view(torch.int32)), (m, t)


@pytest.mark.parametrize("form", ["rs2", "rs4"])
def test_mixed_set_rowsplit(form):
    """A one-modality and a three-modality model in ONE row-split launch (nm_launch_rowsplit_mixed: grads() and train()
    reach it whenever the set's modality counts differ); test_each_model_gets_what_it_gets_alone ties that entry bit for
    bit to the uniform one, this ties it to Adam directly."""
    ga, gb = Golden("mm1_h1"), Golden("mm3_gpoe")
    a, b = make_job(ga, 0), make_job(gb, 0)
    js = nm.JobSet([a, b])

    def next_batch(i):
        swap_batch(a, ga, i % ga.n_steps)
        swap_batch(b, gb, i % gb.n_steps)

    isolated_steps(js, form, "mixed 1+3", next_batch=next_batch)


# ---- d: step count and schedule ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", forms_for(3))
def test_late_optimizer_step(form):
    """Optimizer steps 1001 .. 1008: the second bias correction (1 - 0.999^t = 0.632, 3e-4 relative per step) is visible
    there; at t ~ 20000 it rounds to 1 in fp32 and no one-step check could see it (tests/adam_check.py)."""
    job = golden_run("mm3_gpoe", form, t0=1000)
    assert job.t == 1000 + N_STEPS


@pytest.mark.parametrize("form", forms_for(3))
def test_cyclic_learning_rate_table(form):
    lrs = prep.cyclic_lr(6, 512, 256, 1e-5, 4e-4, 0.9)
    assert len(set(lrs.tolist())) >= 4
    golden_run("mm3_gpoe", form, lr_table=lrs)                  # 8 steps over a table of 6: it wraps


# ---- e: head models -----------------------------------------------------------------------------------------------------
HEADS = [("regression", 0.0), ("endtoend", 0.0), ("endtoend", 0.5)]


@pytest.mark.parametrize("split", [False, True])
@pytest.mark.parametrize("source", ["baseline", "golden"])
@pytest.mark.parametrize("kind,dropout", HEADS)
def test_head_models(kind, dropout, source, split):
    """grads_head(s), then train_regression(1) / train_endtoend(1): trunk, regressor and classifier parameters in one flat
    buffer, one check.  The dropout mask is a hash of (seed, step): the same in both launches."""
    if source == "golden":
        job = golden_job(kind) if kind == "regression" else golden_job(kind, dropout=dropout)
    else:
        job = baseline_job(kind, rows=600, dropout=dropout)
    job.cls_train, job.cls_use_mu = True, False                # as train_endtoend sets them: both launches see one classifier
    js = nm.JobSet([job])
    train = (lambda: js.train_regression(1, split=split)) if kind == "regression" else (lambda: js.train_endtoend(1, split=split))
    form = "head_split" if split else "head"
    isolated_steps(js, form, f"{source} {kind} dropout {dropout}", n_steps=4, grads=lambda s: js.grads_head(s, split=split),
                   train=train)
    assert job.t == 4
    if kind == "endtoend":                                      # BatchNorm did move its running statistics meanwhile
        sd = job.state_dict()
        assert any(float(v.abs().max()) > 0.0 for k, v in sd.items() if k.endswith("running_mean"))


# ---- f: both flags in one launch -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["whole", "rs2", "rs4"])
@pytest.mark.parametrize("shape", ["mm3_gpoe", "3x379"])
def test_adam_and_grads_in_one_launch(shape, form):
    """NM_F_BACKWARD | NM_F_ADAM | NM_F_GRADS through JobSet._launch_form: the gradients of the gradient launch and the
    update of train(1), bit for bit (the counted waits of wgrad_adam / rs_sweep budget the extra store)."""
    make = (lambda: make_job(Golden("mm3_gpoe"), 0)) if shape == "mm3_gpoe" else \
           (lambda: table_job([379, 379, 379], [110, 110], 10, 29, "gpoe", True, 256, 11))
    kw = FORMS[form]
    ref = make()
    rs = nm.JobSet([ref])
    rs.grads(0, export=False, **kw)
    rs.check_split_errors(block=True)
    torch.cuda.synchronize()
    g_ref = ref.grads.cpu().clone()
    rs.train(1, **kw)
    rs.check_split_errors(block=True)
    job = make()
    js = nm.JobSet([job])
    both = _lib.NM_F_BACKWARD | _lib.NM_F_ADAM | _lib.NM_F_GRADS
    js._launch_form(js._training_form(kw.get("split"), kw["rowsplit"]), 0, 1, both, kw.get("helpers"), False)
    js.check_split_errors(block=True)
    torch.cuda.synchronize()
    assert float(g_ref.abs().max()) > 0.0
    for name, x, y in (("grads", job.grads.cpu(), g_ref), *zip(("params", "adam_m", "adam_v"), _state(job), _state(ref))):
        assert torch.equal(x, y), (shape, form, name, int((x != y).sum()), float((x - y).abs().max()))
    assert not torch.equal(job.params.cpu(), make().params.cpu())

