"""The posterior-predictive pass (nm_devpass_draws: encoders once per 128-row tile, then S times fusion, draw and decoders,
the S reconstructions folded in the kernel) against the passes it repeats and the numpy restatement of its definition
(tests/predictive_ref.py):
  anchor        S = 1 IS the existing pass: pred_mean / pred_msq equal out_loc / out_sqerr bit for bit, pred_var is zeros
  fold          S separate existing launches (seed or eps of draw s), their out_loc folded in numpy: pred_mean / pred_var bit
                for bit; pred_msq bit for bit from the kernel's own mean / variance / x; pred_z within 1e-6; row means 2e-6
  stale memory  exports pre-filled with NaN: finite on the table's rows, zeros on pad columns and dead rows
  independence  20 jobs in one launch against each alone, a tile sub-range, two runs, exports left out
  sense         S = 64 in-kernel draws: positive variance, the mean near the noise-free reconstruction
Shapes A, B, C of tests/test_gpu_devpass_multi.py and D, one expert (bypass on and off)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import multi_modal_normative_modeling_amd as nm
from multi_modal_normative_modeling_amd import engine
from tests import predictive_ref as PR
from tests import twin_cases as T

DEV = "cuda:0"

# N, D per modality, hidden, Z, c_dim
SHAPES = {
    "A": (300, (61, 90, 47), (64, 48), 12, 3),        # two full 128-row tiles, a 44-row one, an empty half
    "B": (129, (40, 40, 40, 120), (112,), 32, 5),     # four experts, width and latent at the limits, one row in tile 2
    "C": (40, (116, 50), (110, 110), 10, 2),          # fewer rows than one tile; Z not a multiple of 4: the scalar fusion path
    "D": (140, (70,), (112,), 32, 3),                 # one expert, a full tile and a 12-row one
}
EXPORTS = ("pred_mean", "pred_var", "pred_msq", "pred_z", "pred_rowdev", "pred_rowz2")


class Setup:
    """Tables, weights and injected draws of one shape, built once per module and shared (never written to)."""

    def __init__(self, shape, seed=21, non_linear=True, state=None, xs=None, cs=None):
        self.N, self.dims, self.hidden, self.Z, self.c_dim = SHAPES[shape]
        g = torch.Generator().manual_seed(seed)
        if xs is None:
            xs = [torch.randn(self.N, d, generator=g) * 1.1 for d in self.dims]
            c = torch.zeros(self.N, self.c_dim)
            c[torch.arange(self.N), torch.randint(0, self.c_dim, (self.N,), generator=g)] = 1
            cs = [c] * len(self.dims)
        self.xs = xs
        self.tables = [nm.Table(x, c, DEV) for x, c in zip(xs, cs)]
        self.nt = self.tables[0].n_tiles
        self.spec = nm.ModelSpec(list(self.dims), list(self.hidden), self.Z, self.c_dim, non_linear, "multimodal")
        self.P = state if state is not None else nm.ParamLayout(self.spec).init_reference_rule(seed + 1)
        # logvar_out away from its constant initial value: the noise variance differs per ROI
        for k in self.P:
            if k.endswith("logvar_out"):
                self.P[k] = -3.0 + 0.5 * torch.randn(self.P[k].shape, generator=g)
        self.eps = [torch.randn(self.nt, 256, self.Z, generator=g) for _ in range(16)]

    def job(self, combine, seed=11, eps=None, bypass=True):
        job = nm.Job(self.spec, self.tables, combine=combine, state=self.P, seed=seed, single_bypass=bypass, n_tiles_ws=self.nt)
        if eps is not None:
            job.set_eps(eps)
        job.enable_exports(loc=True, sqerr=True, rowdev=True, latent=False)
        return job


_SETUPS = {}


def setup_of(shape):
    if shape not in _SETUPS:
        _SETUPS[shape] = Setup(shape)
    return _SETUPS[shape]


def existing_pass(job):
    """The pass the job otherwise runs on: nm_devpass_multi for several experts, forward(loss=False) for one (nm_devpass with
    the bypass, the general kernel without).  -> per modality (out_loc, out_sqerr, out_rowdev), on the host."""
    js = nm.JobSet([job])
    if len(job.kmods) > 1:
        js.forward(loss=False, compact=True)
    else:
        js.forward(loss=False)
    torch.cuda.synchronize()
    return [(job.out_loc[m].cpu().clone(), job.out_sqerr[m].cpu().clone(), job.out_rowdev[m].cpu().clone())
            for m in range(len(job.kmods))]


def nan_fill(job):
    for name in EXPORTS:
        for t in getattr(job, name):
            if t is not None:
                t._base.fill_(float("nan")) if t._base is not None else t.fill_(float("nan"))


def run_draws(job, S, seeds=None, eps=None, tile0=0, n_tiles=None, fill=True, **kw):
    job.enable_predictive_exports(S, seeds=seeds, eps=eps, **kw)
    if fill:
        nan_fill(job)
    nm.JobSet([job]).forward_draws(tile0=tile0, n_tiles=n_tiles)
    torch.cuda.synchronize()
    return job


def pred(job, name, m):
    t = getattr(job, name)[m]
    return None if t is None else t.cpu().clone()


# ---------------------------------------------------------------------------------------------------------------------
# anchor
# ---------------------------------------------------------------------------------------------------------------------
def _anchor(job_existing, job_draws, eps1, what):
    ref = existing_pass(job_existing)
    run_draws(job_draws, 1, eps=eps1)
    N = job_draws.tables[0].N
    for m, (loc, sq, rd) in enumerate(ref):
        mean, var, msq, rdev = (pred(job_draws, n, m) for n in ("pred_mean", "pred_var", "pred_msq", "pred_rowdev"))
        assert torch.equal(mean, loc), (what, m, "pred_mean", float((mean - loc).abs().max()))
        assert torch.equal(msq, sq), (what, m, "pred_msq", float((msq - sq).abs().max()))
        assert float(var.abs().max()) == 0.0, (what, m, "pred_var")
        assert torch.allclose(rdev, rd, rtol=2e-6, atol=1e-9), (what, m, "pred_rowdev")
        assert float(loc[:N].abs().max()) > 0 and float(sq[:N].abs().max()) > 0


@pytest.mark.parametrize("shape,combine,inject,bypass", [
    ("A", "poe", True, True), ("A", "gpoe", True, True), ("A", "moe", True, True), ("A", "mopoe", True, True),
    ("A", "gpoe", False, True), ("B", "gpoe", True, True), ("B", "mopoe", False, True), ("C", "poe", True, True),
    ("C", "gpoe", False, True), ("D", "poe", False, True), ("D", "poe", True, True), ("D", "gpoe", False, False),
    ("D", "poe", True, False),
])
def test_one_draw_is_the_existing_pass(shape, combine, inject, bypass):
    su = setup_of(shape)
    eps = su.eps[0] if inject else None
    _anchor(su.job(combine, eps=eps, bypass=bypass), su.job(combine, bypass=bypass), [eps] if inject else None,
            (shape, combine, inject, bypass))


def _twin_cases():
    return T.cases("devpass_multi") + T.cases("devpass") + [c for c in T.cases("latent") if c.M == 1]


@pytest.mark.parametrize("cs", _twin_cases(), ids=lambda cs: cs.id)
def test_one_draw_is_the_existing_pass_over_the_twin_cases(cs):
    """The whole admitted domain, as the twin fuzz draws it: the several-expert cases, the one-expert cases with the bypass,
    and the encoder-only twin's one-expert cases (bypass on or off)."""
    gen = torch.Generator().manual_seed(cs.data_seed)
    spec = nm.ModelSpec(list(cs.dims), list(cs.hidden), cs.Z, cs.c_dim, cs.non_linear, cs.kind)
    P = nm.ParamLayout(spec).init_reference_rule(cs.init_seed)
    xs = [torch.randn(cs.N, d, generator=gen) * 1.2 for d in cs.dims]
    covs = []
    for _ in range(1 if cs.shared_cov else cs.M):
        c = torch.zeros(cs.N, cs.c_dim)
        c[torch.arange(cs.N), torch.randint(0, cs.c_dim, (cs.N,), generator=gen)] = 1
        covs.append(c)
    covs = covs * cs.M if cs.shared_cov else covs
    tables = [nm.Table(x, c, DEV) for x, c in zip(xs, covs)]
    nt = tables[0].n_tiles
    eps = torch.randn(nt, 256, cs.Z, generator=gen) if cs.inject else None

    def job(own_eps):
        j = nm.Job(spec, tables, combine=cs.combine, state=P, seed=cs.job_seed, single_bypass=cs.single_bypass, n_tiles_ws=nt)
        if own_eps is not None:
            j.set_eps(own_eps)
        j.enable_exports(loc=True, sqerr=True, rowdev=True, latent=False)
        return j
    _anchor(job(eps), job(None), [eps] if cs.inject else None, cs.id)


# ---------------------------------------------------------------------------------------------------------------------
# fold
# ---------------------------------------------------------------------------------------------------------------------
FOLD_CASES = [("A", "gpoe", False, True), ("A", "mopoe", True, True), ("B", "gpoe", True, True), ("C", "poe", False, True),
              ("D", "poe", False, True), ("D", "gpoe", True, False)]
_SEPARATE = {}


def separate_launches(case):
    """out_loc of 16 separate existing launches, draw s under seeds[s] (or eps[s] injected): computed once per case, shared by
    the S of the fold test (their prefixes), never written to."""
    if case not in _SEPARATE:
        shape, combine, inject, bypass = case
        su = setup_of(shape)
        seeds = engine.draw_seeds(11, 16)
        locs = []
        for s in range(16):
            job = su.job(combine, seed=seeds[s], eps=su.eps[s] if inject else None, bypass=bypass)
            locs.append([loc.numpy() for loc, _, _ in existing_pass(job)])
        _SEPARATE[case] = locs
    return _SEPARATE[case]


@pytest.mark.parametrize("S", [2, 5, 16])
@pytest.mark.parametrize("case", FOLD_CASES, ids=lambda c: f"{c[0]}-{c[1]}-{'eps' if c[2] else 'seed'}-{'bypass' if c[3] else 'fused'}")
def test_fold_of_separate_launches(case, S):
    shape, combine, inject, bypass = case
    su = setup_of(shape)
    locs = separate_launches(case)
    job = run_draws(su.job(combine, seed=11, bypass=bypass), S, eps=su.eps[:S] if inject else None)
    assert inject or job.pred_seeds == engine.draw_seeds(11, S)
    N = su.N
    for m, D in enumerate(su.dims):
        mean_ref, m2_ref = PR.fold(np.stack([locs[s][m] for s in range(S)]))
        var_ref = PR.variance(m2_ref, S)
        mean, var, msq, z = (pred(job, n, m).numpy() for n in ("pred_mean", "pred_var", "pred_msq", "pred_z"))
        assert np.array_equal(mean, mean_ref), (m, "pred_mean", float(np.abs(mean - mean_ref).max()))
        assert np.array_equal(var, var_ref), (m, "pred_var", float(np.abs(var - var_ref).max()))
        assert float(var[:N].min()) > 0
        # the derived exports from the kernel's OWN mean / variance and x
        x = np.zeros_like(mean)
        x[:N] = su.xs[m].numpy()
        msq_ref = PR.msq(x, mean, var, S)
        assert np.array_equal(msq[:N], msq_ref[:N]), (m, "pred_msq", float(np.abs(msq[:N] - msq_ref[:N]).max()))
        nv = job.noise_var[m][:D].cpu().numpy()
        want_nv = np.exp(su.P[[k for k in su.P if k.endswith("logvar_out")][m]].numpy().reshape(-1).astype(np.float32))
        np.testing.assert_allclose(nv, want_nv, rtol=1e-6)
        z_ref = PR.zscore(x[:N], mean[:N], var[:N], nv[None])
        err = np.abs(z[:N] - z_ref) / np.maximum(np.abs(z_ref), 1e-30)
        print(f"{case} S={S} modality {m}: pred_z worst relative error {float(err.max()):.3e}")
        assert float(err.max()) <= 1e-6, (m, "pred_z")
        rdev, rz2 = pred(job, "pred_rowdev", m).numpy(), pred(job, "pred_rowz2", m).numpy()
        np.testing.assert_allclose(rdev[:N], msq[:N].astype(np.float64).mean(axis=1), rtol=2e-6, atol=1e-9)
        np.testing.assert_allclose(rz2[:N], (z[:N].astype(np.float64) ** 2).mean(axis=1), rtol=2e-6, atol=1e-9)


# ---------------------------------------------------------------------------------------------------------------------
# stale memory
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,S", [("A", 1), ("A", 3), ("B", 2), ("C", 3), ("D", 2)])
def test_stale_buffer_contents_never_enter_a_result(shape, S):
    """Every export holds NaN before the launch (pad columns and the rows past the table included): finite on the table's
    rows, zeros on the pad columns and on every row from the table's end to the end of its last 256-row tile."""
    su = setup_of(shape)
    job = run_draws(su.job("gpoe"), S)
    N = su.N
    for m, D in enumerate(su.dims):
        for name in ("pred_mean", "pred_var", "pred_msq", "pred_z"):
            full = getattr(job, name)[m]._base.cpu()                  # [rows_alloc, x_pitch]: the pad columns too
            assert bool(torch.isfinite(full).all()), (m, name)
            assert float(full[:N, :D].abs().max()) > 0 or (name == "pred_var" and S == 1), (m, name)
            assert float(full[:, D:].abs().max() if full.shape[1] > D else 0.0) == 0.0, (m, name, "pad columns")
            assert float(full[N:].abs().max()) == 0.0, (m, name, "dead rows")
        for name in ("pred_rowdev", "pred_rowz2"):
            row = getattr(job, name)[m].cpu()
            assert bool(torch.isfinite(row).all()) and float(row[:N].min()) > 0, (m, name)
            assert float(row[N:].abs().max()) == 0.0, (m, name, "dead rows")


# ---------------------------------------------------------------------------------------------------------------------
# independence
# ---------------------------------------------------------------------------------------------------------------------
def _all_exports(job):
    return {f"{n}[{m}]": pred(job, n, m) for n in EXPORTS for m in range(len(job.kmods)) if getattr(job, n)[m] is not None}


def test_twenty_jobs_in_one_launch_equal_each_alone():
    su = setup_of("A")
    combs = ("gpoe", "poe", "moe", "mopoe")
    jobs = [su.job(combs[j % 4], seed=100 + j) for j in range(20)]
    for j in jobs:
        j.enable_predictive_exports(3)
        nan_fill(j)
    nm.JobSet(jobs).forward_draws()
    torch.cuda.synchronize()
    for j in range(20):
        alone = run_draws(su.job(combs[j % 4], seed=100 + j), 3)
        T.assert_same(_all_exports(alone), _all_exports(jobs[j]), f"job {j}")


def test_a_tile_sub_range_equals_the_full_launch_on_its_rows():
    """517 rows would need a larger table: shape A has two 256-row batches -- batch 1 alone (rows 256..299 and its dead rows)
    against the full launch; the rows of batch 0 keep what the buffers held."""
    su = setup_of("A")
    full = run_draws(su.job("mopoe"), 4)
    part = run_draws(su.job("mopoe"), 4, tile0=1, n_tiles=1)
    for name, t in _all_exports(part).items():
        f = _all_exports(full)[name]
        assert torch.equal(t[256:], f[256:]), name
        assert bool(torch.isnan(t[:256]).all()), name                 # untouched: still the fill


def test_two_runs_give_the_same_bytes():
    su = setup_of("B")
    a, b = run_draws(su.job("gpoe"), 5), run_draws(su.job("gpoe"), 5)
    T.assert_same(_all_exports(a), _all_exports(b), "run 1 against run 2")
    nm.JobSet([a]).forward_draws()                                    # ... and again over its own results
    torch.cuda.synchronize()
    T.assert_same(_all_exports(a), _all_exports(b), "second launch over the first's results")


@pytest.mark.parametrize("kw", [{"msq": False}, {"z": False}, {"rowdev": False}, {"rowz2": False},
                                {"msq": False, "z": False, "rowdev": False, "rowz2": False}], ids=lambda kw: "-".join(kw))
def test_exports_left_out_are_skipped_without_touching_the_others(kw):
    su = setup_of("A")
    want = _all_exports(run_draws(su.job("gpoe"), 4))
    job = run_draws(su.job("gpoe"), 4, **kw)
    got = _all_exports(job)
    for name in ("pred_msq", "pred_z", "pred_rowdev", "pred_rowz2"):
        short = name[len("pred_"):]
        assert (getattr(job, name)[0] is None) == (kw.get(short) is False), name
    assert set(got) < set(want)
    T.assert_same(got, {k: want[k] for k in got}, str(kw))
    assert (job.noise_var[0] is None) == (kw.get("z") is False and kw.get("rowz2") is False)


def test_trace_records_the_phases_and_changes_no_result():
    """NM_F_TRACE as in the siblings: workgroup (0, 0) records interval cycles per wave and tag (nm_trace_read_dv); the exports
    are the untraced launch's."""
    import ctypes as C
    lib = nm._lib.load()
    su = setup_of("A")
    plain = run_draws(su.job("gpoe"), 3)
    job = su.job("gpoe")
    job.enable_predictive_exports(3)
    nan_fill(job)
    buf = (C.c_ulonglong * 512)()
    lib.nm_trace_read_dv(buf, 1)                                      # (cleared)
    nm.JobSet([job]).forward_draws(trace=True)
    torch.cuda.synchronize()
    assert lib.nm_trace_read_dv(buf, 1) == 0
    cycles = np.array(buf[:], dtype=np.uint64).reshape(8, 64)
    for tag in (1, 3, 5, 7, 8):                                       # encoders, fusion, decoder layers, chunk epilogue, decoder end
        assert (cycles[:, tag] > 0).all(), (tag, cycles[:, tag])
    T.assert_same(_all_exports(job), _all_exports(plain), "traced against untraced")


# ---------------------------------------------------------------------------------------------------------------------
# the drop-in classes
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cls", ["cVAE_multimodal", "mmJSD", "cVAE_multimodal_regression", "cVAE"])
def test_pred_recon_draws_of_the_drop_in_classes(cls):
    """pred_recon_draws: per modality mean / var / msq / z as numpy; the same seed gives the same bytes, another seed another
    table; msq restated from mean, var and x bit for bit; one draw with a seed is that seed's single-draw squared error."""
    import pandas as pd
    su = setup_of("D" if cls == "cVAE" else "A")
    N, S = su.N, 6
    g = torch.Generator().manual_seed(3)
    cov = torch.zeros(N, su.c_dim)
    cov[torch.arange(N), torch.randint(0, su.c_dim, (N,), generator=g)] = 1
    frames = [pd.DataFrame(x.numpy()) for x in su.xs]
    if cls == "cVAE":
        model = nm.cVAE(su.dims[0], list(su.hidden), su.Z, su.c_dim, non_linear=True)
        call = lambda S, seed: [model.pred_recon_draws(frames[0], cov.long().numpy(), DEV, n_draws=S, seed=seed)]
    else:
        model = getattr(nm, cls)(list(su.dims), list(su.hidden), su.Z, su.c_dim, modalities=len(su.dims), non_linear=True)
        call = lambda S, seed: model.pred_recon_draws(frames, cov.long().numpy(), DEV, "gpoe", S, seed=seed)
    model.to(DEV)
    a, b, other = call(S, 5), call(S, 5), call(S, 6)
    assert len(a) == len(su.dims)
    for m, D in enumerate(su.dims):
        x = su.xs[m].numpy()
        for k in ("mean", "var", "msq", "z"):
            assert a[m][k].shape == (N, D) and a[m][k].dtype == np.float32 and np.isfinite(a[m][k]).all(), (m, k)
            assert np.array_equal(a[m][k], b[m][k]), (m, k)
        assert not np.array_equal(a[m]["mean"], other[m]["mean"])
        assert float(a[m]["var"].min()) > 0
        assert np.array_equal(a[m]["msq"], PR.msq(x, a[m]["mean"], a[m]["var"], S)), m
    one = call(1, 5)
    for m in range(len(su.dims)):
        d = su.xs[m].numpy() - one[m]["mean"]
        assert float(np.abs(one[m]["var"]).max()) == 0.0 and np.array_equal(one[m]["msq"], d * d), m
    with pytest.raises(ValueError, match="1 to 64"):
        call(65, 5)


# ---------------------------------------------------------------------------------------------------------------------
# sense
# ---------------------------------------------------------------------------------------------------------------------
def test_sixty_four_draws_average_towards_the_noise_free_reconstruction():
    """In-kernel draws, S = 64: the variance is positive on every live element, and R -- the Frobenius distance of pred_mean
    to the eps = 0 reconstruction over the same distance for draw 0 alone -- is below 0.5 (independent draws: about 1 / 8;
    the CPU oracle's own R for these weights is below 0.25, tests/test_predictive_ref_cpu.py)."""
    c = PR.SENSE
    xs, cs, P = PR.sense_inputs()
    tables = [nm.Table(x, cv, DEV) for x, cv in zip(xs, cs)]
    nt, N = tables[0].n_tiles, c["N"]
    spec = nm.ModelSpec(list(c["dims"]), list(c["hidden"]), c["Z"], c["c_dim"], c["non_linear"], "multimodal")

    def job(eps=None):
        j = nm.Job(spec, tables, combine=c["combine"], state=P, seed=5, n_tiles_ws=nt)
        if eps is not None:
            j.set_eps(eps)
        j.enable_exports(loc=True, sqerr=True, rowdev=True, latent=False)
        return j
    clean = existing_pass(job(torch.zeros(nt, 256, c["Z"])))
    first = existing_pass(job())
    many = run_draws(job(), 64)
    for m in range(len(c["dims"])):
        mean, var = pred(many, "pred_mean", m)[:N], pred(many, "pred_var", m)[:N]
        assert float(var.min()) > 0, m
        ratio = float(torch.linalg.norm(mean - clean[m][0][:N]) / torch.linalg.norm(first[m][0][:N] - clean[m][0][:N]))
        print(f"modality {m}: R = {ratio:.4f}")
        assert ratio < 0.5, (m, ratio)
