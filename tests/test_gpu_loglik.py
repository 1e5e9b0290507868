"""The likelihood pass (nm_devpass_iw: encoders once per 128-row tile, then S times fusion, draw and decoders, the importance
weights log w_s = log p(x | z_s, c) + log p(z_s) - log q(z_s | x, c) folded per subject in the kernel) against the general
kernel's exports fed to the fp64 restatement of its definition (tests/loglik_ref.py), every column within the bound the
restatement derives:
  weights       S = 1, injected eps: log_px, elbo, kl, kl_mc, recon_ll[m] within their bounds; ess == 1 and logw_max ==
                logw_min == log_px exactly
  fold          S = 16 injected draws against 16 separate general-kernel launches, every column, every combiner
  seeds         seeded draws: draw s is the general kernel's draw under key s (its out_z, out_loc; eps recovered from z in
                fp64), every column within its bound; the S-draw launch's logw_max / logw_min and elbo equal, bit for bit, the
                fp32 max / min / running mean of S single-draw launches under the same keys
  decoder mask  recon_ll[m] of the full request against the request for {m}; kl / kl_mc bit-identical across masks
  stale memory  exports pre-filled with NaN: finite on the table's rows, zeros on dead rows
  independence  20 jobs in one launch against each alone, a tile sub-range, two runs: bit for bit
  many draws    S = 1024: finite, 1 <= ess <= S, elbo <= log_px <= logw_max within the bound
  spread        logvar_out = -8: log-weights hundreds of nats apart, nothing inf or NaN, ess near 1
Shapes A-D and the Setup of tests/test_gpu_devpass_draws.py."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import multi_modal_normative_modeling_amd as nm
from multi_modal_normative_modeling_amd import engine
from multi_modal_normative_modeling_amd.metrics import LOGLIK_ROW_COLUMNS
from tests import loglik_ref as LR
from tests import twin_cases as T
from tests.test_gpu_devpass_draws import DEV, setup_of

COL = {n: i for i, n in enumerate(LOGLIK_ROW_COLUMNS)}


def logvar_out(su, P=None):
    P = su.P if P is None else P
    return [P[k].numpy().reshape(-1) for k in P if k.endswith("logvar_out")]


def general(su, combine, seed=11, eps=None, bypass=True, P=None):
    """One launch of the general kernel with every export on: out_loc per modality, out_mu, out_logvar, out_z on the host."""
    job = nm.Job(su.spec, su.tables, combine=combine, state=su.P if P is None else P, seed=seed, single_bypass=bypass,
                 n_tiles_ws=su.nt)
    if eps is not None:
        job.set_eps(eps)
    job.enable_exports(loc=True, sqerr=False, rowdev=False, latent=True)
    nm.JobSet([job]).forward(loss=False)
    torch.cuda.synchronize()
    N = su.N
    return ([t[:N].cpu().numpy() for t in job.out_loc], job.out_mu[:N].cpu().numpy(), job.out_logvar[:N].cpu().numpy(),
            job.out_z[:N].cpu().numpy())


def iw_job(su, combine, seed=11, bypass=True, P=None):
    return nm.Job(su.spec, su.tables, combine=combine, state=su.P if P is None else P, seed=seed, single_bypass=bypass,
                  n_tiles_ws=su.nt)


def nan_fill(job):
    job.iw_row.fill_(float("nan"))
    for t in job.iw_recon_ll:
        if t is not None:
            t.fill_(float("nan"))


def run_iw(job, S, seeds=None, eps=None, decoders=None, per_modality=True, tile0=0, n_tiles=None):
    job.enable_likelihood_exports(S, seeds=seeds, eps=eps, decoders=decoders, per_modality=per_modality)
    nan_fill(job)
    nm.JobSet([job]).forward_loglik(tile0=tile0, n_tiles=n_tiles)
    torch.cuda.synchronize()
    return job


def exports(job):
    out = {"row": job.iw_row.cpu().clone()}
    for m, t in enumerate(job.iw_recon_ll):
        if t is not None:
            out[f"recon_ll[{m}]"] = t.cpu().clone()
    return out


def check_columns(job, su, val, bnd, what, columns=LOGLIK_ROW_COLUMNS, decoders=None):
    """Every asked column of the kernel within the restatement's bound; prints the worst |kernel - restatement| / bound."""
    row = job.iw_row[: su.N].cpu().numpy()
    worst = {}
    for name in columns:
        worst[name] = LR.worst_ratio(row[:, COL[name]], val[name], bnd[name])
    for m in (range(len(su.dims)) if decoders is None else decoders):
        if job.iw_recon_ll[m] is not None:
            worst[f"recon_ll_{m}"] = LR.worst_ratio(job.iw_recon_ll[m][: su.N].cpu().numpy(), val[f"recon_ll_{m}"],
                                                    bnd[f"recon_ll_{m}"])
    print(what, "worst |kernel - restatement| / bound:", {k: f"{v:.3e}" for k, v in worst.items()})
    assert np.isfinite(row).all(), what
    for name, r in worst.items():
        assert r <= 1.0, (what, name, r)


# ---------------------------------------------------------------------------------------------------------------------
# weights
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,combine,bypass", [
    ("A", "poe", True), ("A", "gpoe", True), ("A", "moe", True), ("A", "mopoe", True), ("B", "gpoe", True), ("B", "mopoe", True),
    ("C", "poe", True), ("C", "gpoe", True), ("D", "poe", True), ("D", "poe", False), ("D", "gpoe", False),
])
def test_one_draw_weight_is_the_definition_on_the_general_kernels_exports(shape, combine, bypass):
    su = setup_of(shape)
    eps = su.eps[0]
    loc, mu, lv, z = general(su, combine, eps=eps, bypass=bypass)
    e = eps.reshape(-1, su.Z)[: su.N].numpy()
    val, bnd = LR.loglik([x.numpy() for x in su.xs], [l[None] for l in loc], mu, lv, e[None], z[None], logvar_out(su))
    job = run_iw(iw_job(su, combine, bypass=bypass), 1, eps=[eps])
    check_columns(job, su, val, bnd, (shape, combine, bypass), columns=("log_px", "elbo", "kl", "kl_mc", "recon_ll"))
    row = job.iw_row[: su.N].cpu().numpy()
    assert np.array_equal(row[:, COL["ess"]], np.ones(su.N, np.float32))
    assert np.array_equal(row[:, COL["logw_max"]], row[:, COL["log_px"]])
    assert np.array_equal(row[:, COL["logw_min"]], row[:, COL["log_px"]])


# ---------------------------------------------------------------------------------------------------------------------
# fold
# ---------------------------------------------------------------------------------------------------------------------
FOLD_CASES = [("A", "poe", True), ("A", "gpoe", True), ("A", "moe", True), ("A", "mopoe", True), ("B", "gpoe", True),
              ("C", "poe", True), ("D", "poe", True), ("D", "gpoe", False)]
_SEPARATE = {}


def separate_launches(case, inject):
    """16 separate general-kernel launches, draw s under eps[s] injected or under key draw_seeds(11, 16)[s]: computed once
    per case, shared, never written to.  -> x_hat per modality [16, N, D], mu, lv, eps [16, N, Z], z [16, N, Z]."""
    key = (case, inject)
    if key not in _SEPARATE:
        shape, combine, bypass = case
        su = setup_of(shape)
        seeds = engine.draw_seeds(11, 16)
        locs, zs = [], []
        for s in range(16):
            loc, mu, lv, z = general(su, combine, seed=seeds[s], eps=su.eps[s] if inject else None, bypass=bypass)
            locs.append(loc)
            zs.append(z)
        z = np.stack(zs)
        if inject:
            eps = np.stack([su.eps[s].reshape(-1, su.Z)[: su.N].numpy() for s in range(16)])
        else:        # the generator's draw, recovered from z = mu + eps exp(lv / 2) in fp64
            eps = (z.astype(np.float64) - mu.astype(np.float64)[None]) * np.exp(-0.5 * lv.astype(np.float64))[None]
        _SEPARATE[key] = ([np.stack([locs[s][m] for s in range(16)]) for m in range(len(su.dims))], mu, lv, eps, z)
    return _SEPARATE[key]


@pytest.mark.parametrize("case", FOLD_CASES, ids=lambda c: f"{c[0]}-{c[1]}-{'bypass' if c[2] else 'fused'}")
def test_fold_of_sixteen_separate_launches(case):
    shape, combine, bypass = case
    su = setup_of(shape)
    xh, mu, lv, eps, z = separate_launches(case, True)
    val, bnd = LR.loglik([x.numpy() for x in su.xs], xh, mu, lv, eps, z, logvar_out(su))
    job = run_iw(iw_job(su, combine, bypass=bypass), 16, eps=su.eps[:16])
    check_columns(job, su, val, bnd, case)
    row = job.iw_row[: su.N].cpu().numpy()
    assert (row[:, COL["ess"]] >= 1.0).all() and (row[:, COL["ess"]] <= 16.0).all()


# ---------------------------------------------------------------------------------------------------------------------
# seeds
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [("A", "gpoe", True), ("C", "poe", True), ("D", "poe", True), ("D", "gpoe", False)],
                         ids=lambda c: f"{c[0]}-{c[1]}-{'bypass' if c[2] else 'fused'}")
def test_seeded_draws_are_the_general_kernels_draws_under_the_same_keys(case):
    shape, combine, bypass = case
    su = setup_of(shape)
    S = 16
    seeds = engine.draw_seeds(11, S)
    xh, mu, lv, eps, z = separate_launches(case, False)
    val, bnd = LR.loglik([x.numpy() for x in su.xs], xh, mu, lv, eps, z, logvar_out(su))
    job = run_iw(iw_job(su, combine, seed=11, bypass=bypass), S)
    assert job.iw_seeds == seeds
    check_columns(job, su, val, bnd, case)
    row = job.iw_row[: su.N].cpu().numpy()
    # one draw at a time under the same keys: the S log-weights themselves, as fp32
    lw = np.stack([run_iw(iw_job(su, combine, bypass=bypass), 1, seeds=[seeds[s]]).iw_row[: su.N, COL["log_px"]].cpu().numpy()
                   for s in range(S)])
    assert np.array_equal(row[:, COL["logw_max"]], lw.max(axis=0))
    assert np.array_equal(row[:, COL["logw_min"]], lw.min(axis=0))
    acc = np.zeros(su.N, np.float32)
    for s in range(S):
        acc = (acc + lw[s]).astype(np.float32)
    assert np.array_equal(row[:, COL["elbo"]], (acc / np.float32(S)).astype(np.float32))
    given = run_iw(iw_job(su, combine, seed=5, bypass=bypass), S, seeds=seeds)      # the keys, not the job's seed, decide
    T.assert_same(exports(given), exports(job), "seeds given against seeds derived")


# ---------------------------------------------------------------------------------------------------------------------
# decoder mask
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["A", "B"])
def test_decoder_mask(shape):
    su = setup_of(shape)
    M, N, S = len(su.dims), su.N, 4
    xh, mu, lv, eps, z = separate_launches((shape, "gpoe", True), True)
    full = run_iw(iw_job(su, "gpoe"), S, eps=su.eps[:S])
    frow = full.iw_row[:N].cpu().numpy()
    for m in range(M):
        one = run_iw(iw_job(su, "gpoe"), S, eps=su.eps[:S], decoders=[m])
        assert [t is not None for t in one.iw_recon_ll] == [k == m for k in range(M)]
        orow = one.iw_row[:N].cpu().numpy()
        val, bnd = LR.loglik([x.numpy() for x in su.xs], [h[:S] for h in xh], mu, lv, eps[:S], z[:S], logvar_out(su), decoders=[m])
        check_columns(one, su, val, bnd, (shape, "mask", m), decoders=[m])
        # the same decoder's term, whichever request it is part of
        a, b = full.iw_recon_ll[m][:N].cpu().numpy(), orow[:, COL["recon_ll"]]
        assert (np.abs(a.astype(np.float64) - b) <= bnd[f"recon_ll_{m}"]).all(), m
        assert np.array_equal(one.iw_recon_ll[m][:N].cpu().numpy(), a), m
        for name in ("kl", "kl_mc"):
            assert np.array_equal(orow[:, COL[name]], frow[:, COL[name]]), (m, name)
    with pytest.raises(ValueError, match="decoders"):
        iw_job(su, "gpoe").enable_likelihood_exports(2, decoders=[M])
    with pytest.raises(ValueError, match="decoders"):
        iw_job(su, "gpoe").enable_likelihood_exports(2, decoders=[])


# ---------------------------------------------------------------------------------------------------------------------
# stale memory
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,S", [("A", 1), ("A", 3), ("B", 2), ("C", 3), ("D", 2)])
def test_stale_buffer_contents_never_enter_a_result(shape, S):
    su = setup_of(shape)
    job = run_iw(iw_job(su, "gpoe"), S)
    for name, t in exports(job).items():
        assert bool(torch.isfinite(t).all()), name
        assert float(t[: su.N].abs().min()) > 0 or name == "row", name
        assert float(t[su.N:].abs().max()) == 0.0, (name, "dead rows")
    assert float(job.iw_row[: su.N, COL["log_px"]].abs().min()) > 0


# ---------------------------------------------------------------------------------------------------------------------
# independence
# ---------------------------------------------------------------------------------------------------------------------
def test_twenty_jobs_in_one_launch_equal_each_alone():
    su = setup_of("A")
    combs = ("gpoe", "poe", "moe", "mopoe")
    jobs = [iw_job(su, combs[j % 4], seed=100 + j) for j in range(20)]
    for j in jobs:
        j.enable_likelihood_exports(3, per_modality=True)
        nan_fill(j)
    nm.JobSet(jobs).forward_loglik()
    torch.cuda.synchronize()
    for j in range(20):
        alone = run_iw(iw_job(su, combs[j % 4], seed=100 + j), 3)
        T.assert_same(exports(alone), exports(jobs[j]), f"job {j}")


def test_a_tile_sub_range_equals_the_full_launch_on_its_rows():
    su = setup_of("A")
    full = exports(run_iw(iw_job(su, "mopoe"), 4))
    part = exports(run_iw(iw_job(su, "mopoe"), 4, tile0=1, n_tiles=1))
    for name, t in part.items():
        assert torch.equal(t[256:], full[name][256:]), name
        assert bool(torch.isnan(t[:256]).all()), name                 # untouched: still the fill


def test_two_runs_give_the_same_bytes():
    su = setup_of("B")
    a, b = run_iw(iw_job(su, "gpoe"), 5), run_iw(iw_job(su, "gpoe"), 5)
    T.assert_same(exports(a), exports(b), "run 1 against run 2")
    nm.JobSet([a]).forward_loglik()                                   # ... and again over its own results
    torch.cuda.synchronize()
    T.assert_same(exports(a), exports(b), "second launch over the first's results")


# ---------------------------------------------------------------------------------------------------------------------
# many draws, spread
# ---------------------------------------------------------------------------------------------------------------------
def lipschitz_slack(su, row):
    """The bound of a value that is 1-Lipschitz in the log-weights, with the log-weight bound taken at its largest magnitude:
    n = sum D + Z + M terms whose absolute sum is at least |log w|."""
    n = sum(su.dims) + su.Z + len(su.dims)
    big = np.maximum(np.abs(row[:, COL["logw_min"]]), np.abs(row[:, COL["logw_max"]]))
    return (n + 8) * LR.U * big + 2.0 ** -17 * (1 + np.abs(row[:, COL["log_px"]]))


def test_a_thousand_and_twenty_four_draws():
    su = setup_of("C")
    S = engine._lib.NM_MAX_IW_DRAWS
    row = run_iw(iw_job(su, "gpoe"), S).iw_row[: su.N].cpu().numpy().astype(np.float64)
    assert np.isfinite(row).all()
    ess, elbo, lpx, top = (row[:, COL[n]] for n in ("ess", "elbo", "log_px", "logw_max"))
    assert (ess >= 1.0).all() and (ess <= S).all()
    slack = lipschitz_slack(su, row)
    assert (elbo <= lpx + slack).all() and (lpx <= top + slack).all()
    with pytest.raises(ValueError, match="1 to 1024"):
        iw_job(su, "gpoe").enable_likelihood_exports(S + 1)


def test_log_weights_hundreds_of_nats_apart_stay_finite():
    su = setup_of("C")
    P = {k: (torch.full_like(v, -8.0) if k.endswith("logvar_out") else v) for k, v in su.P.items()}
    S = 16
    job = run_iw(iw_job(su, "gpoe", P=P), S, eps=su.eps[:S])
    row = job.iw_row[: su.N].cpu().numpy().astype(np.float64)
    assert np.isfinite(row).all()
    spread = row[:, COL["logw_max"]] - row[:, COL["logw_min"]]
    print(f"log-weight spread: median {np.median(spread):.1f} nats, ess median {np.median(row[:, COL['ess']]):.4f}")
    assert float(np.median(spread)) > 100.0
    assert (row[:, COL["ess"]] >= 1.0).all() and float(np.median(row[:, COL["ess"]])) < 1.5
    # log S below the largest weight at the most, at the least the largest weight itself: to the two roundings of
    # (mx + log s1) - log S at this magnitude (2 ulp)
    ulp2 = 2.0 ** -22 * np.abs(row[:, COL["logw_max"]])
    assert (row[:, COL["log_px"]] <= row[:, COL["logw_max"]] + ulp2).all()
    assert (row[:, COL["log_px"]] >= row[:, COL["logw_max"]] - np.log(S) - ulp2).all()


# ---------------------------------------------------------------------------------------------------------------------
# the drop-in classes
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cls", ["cVAE_multimodal", "mmJSD", "cVAE_multimodal_regression", "cVAE"])
def test_pred_loglik_of_the_drop_in_classes(cls):
    import pandas as pd
    su = setup_of("D" if cls == "cVAE" else "A")
    N, S, M = su.N, 8, len(su.dims)
    g = torch.Generator().manual_seed(3)
    cov = torch.zeros(N, su.c_dim)
    cov[torch.arange(N), torch.randint(0, su.c_dim, (N,), generator=g)] = 1
    frames = [pd.DataFrame(x.numpy()) for x in su.xs]
    if cls == "cVAE":
        model = nm.cVAE(su.dims[0], list(su.hidden), su.Z, su.c_dim, non_linear=True)
        call = lambda S, seed, **kw: model.pred_loglik(frames[0], cov.long().numpy(), DEV, n_draws=S, seed=seed, **kw)
    else:
        model = getattr(nm, cls)(list(su.dims), list(su.hidden), su.Z, su.c_dim, modalities=M, non_linear=True)
        call = lambda S, seed, **kw: model.pred_loglik(frames, cov.long().numpy(), DEV, "gpoe", S, seed=seed, **kw)
    model.to(DEV)
    a, b, other = call(S, 5), call(S, 5), call(S, 6)
    assert list(a.columns) == list(LOGLIK_ROW_COLUMNS) + [f"recon_ll_{m}" for m in range(M)] and len(a) == N
    assert np.isfinite(a.to_numpy()).all()
    assert a.equals(b) and not a["log_px"].equals(other["log_px"])
    assert np.array_equal(a["kl"].to_numpy(), other["kl"].to_numpy())            # the analytic KL does not see the draws
    assert (a["log_px"].to_numpy() >= a["elbo"].to_numpy() - lipschitz_slack(su, a.to_numpy().astype(np.float64))).all()
    assert ((a["ess"] >= 1) & (a["ess"] <= S)).all()
    one = call(1, 5)
    assert np.array_equal(one["log_px"].to_numpy(), one["elbo"].to_numpy()) and (one["ess"] == 1).all()
    if M > 1:
        sub = call(S, 5, decoders=[1])
        assert list(sub.columns) == list(LOGLIK_ROW_COLUMNS) + ["recon_ll_1"]
        assert np.array_equal(sub["recon_ll_1"].to_numpy(), a["recon_ll_1"].to_numpy())
    with pytest.raises(ValueError, match="1 to 1024"):
        call(1025, 5)
