"""tests/loglik_ref.py, the fp64 restatement of the likelihood pass, against an independent fp64 computation
(torch.distributions.Normal.log_prob, torch.logsumexp, the reference's calc_kl expression), its limiting cases and the
inequalities an importance-weighted bound obeys.  No device."""
import math

import numpy as np
import pytest
import torch
from torch.distributions import Normal

from tests import loglik_ref as LR


def _case(seed, N=23, dims=(17, 9, 30), Z=6, S=5, spread=1.0):
    rng = np.random.default_rng(seed)
    x = [rng.normal(size=(N, d)) for d in dims]
    xh = [rng.normal(size=(S, N, d)) * spread for d in dims]
    mu, lv = rng.normal(size=(N, Z)) * 0.7, rng.normal(size=(N, Z)) * 0.5 - 0.3
    eps = rng.normal(size=(S, N, Z))
    z = mu[None] + eps * np.exp(0.5 * lv)[None]
    lvo = [rng.normal(size=d) * 0.5 - 3.0 for d in dims]
    return x, xh, mu, lv, eps, z, lvo


def _independent(x, xh, mu, lv, eps, z, lvo, dec):
    t = lambda a: torch.as_tensor(np.asarray(a), dtype=torch.float64)
    mu, lv, z = t(mu), t(lv), t(z)
    S = z.shape[0]
    ll = {m: Normal(t(xh[m]), torch.exp(0.5 * t(lvo[m]))).log_prob(t(x[m])).sum(-1) for m in dec}       # [S, N]
    a = Normal(0.0, 1.0).log_prob(z).sum(-1) - Normal(mu, torch.exp(0.5 * lv)).log_prob(z).sum(-1)
    rec = sum(ll.values())
    logw = rec + a
    w = torch.softmax(logw, dim=0)
    out = {"log_px": torch.logsumexp(logw, 0) - math.log(S), "elbo": logw.mean(0), "ess": 1.0 / (w * w).sum(0),
           "kl_mc": -a.mean(0), "kl": (-0.5 * (1 + lv - mu.pow(2) - lv.exp())).sum(-1),          # calc_kl, per row
           "recon_ll": rec.mean(0), "logw_max": logw.max(0).values, "logw_min": logw.min(0).values}
    out.update({f"recon_ll_{m}": ll[m].mean(0) for m in dec})
    return {k: v.numpy() for k, v in out.items()}


@pytest.mark.parametrize("dec", [None, [0], [2], [0, 2]])
@pytest.mark.parametrize("seed", [0, 1])
def test_restatement_agrees_with_an_independent_computation(seed, dec):
    c = _case(seed)
    val, bnd = LR.loglik(*c, decoders=dec)
    ref = _independent(*c, dec=list(range(3)) if dec is None else dec)
    assert set(ref) == set(val) - {"logw"}
    for k, r in ref.items():
        np.testing.assert_allclose(val[k], r, rtol=1e-12, atol=0, err_msg=k)
        assert bnd[k].shape == r.shape and (bnd[k] > 0).all(), k


def test_one_draw_collapses_every_estimate():
    c = _case(3, S=1)
    val, _ = LR.loglik(*c)
    for k in ("elbo", "logw_max", "logw_min"):
        assert np.array_equal(val["log_px"], val[k]), k
    assert np.array_equal(val["ess"], np.ones_like(val["ess"]))


def test_the_bound_is_above_the_elbo_on_every_row_and_grows_with_the_draws():
    c = _case(4, S=64)
    val, _ = LR.loglik(*c)
    assert (val["log_px"] >= val["elbo"]).all() and (val["log_px"] <= val["logw_max"]).all()
    assert (val["ess"] >= 1.0).all() and (val["ess"] <= 64.0).all()
    x, xh, mu, lv, eps, z, lvo = c
    half, _ = LR.loglik(x, [h[:32] for h in xh], mu, lv, eps[:32], z[:32], lvo)
    both = [LR.loglik(x, [h[s:s + 32] for h in xh], mu, lv, eps[s:s + 32], z[s:s + 32], lvo)[0]["log_px"] for s in (0, 32)]
    # the 64-draw estimate is the log of the mean of the two 32-draw likelihood estimates: never below their mean log
    assert (val["log_px"] >= 0.5 * (both[0] + both[1]) - 1e-9).all()
    assert np.array_equal(half["log_px"], both[0])


def test_weights_spread_over_two_thousand_nats_stay_finite():
    c = _case(5, spread=3.0)
    x, xh, mu, lv, eps, z, lvo = c
    lvo = [np.full_like(v, -8.0) for v in lvo]
    val, bnd = LR.loglik(x, xh, mu, lv, eps, z, lvo)
    spread = val["logw_max"] - val["logw_min"]
    assert float(spread.min()) > 2000.0
    for k, v in val.items():
        assert np.isfinite(v).all(), k
        assert np.isfinite(bnd[k]).all(), k
    assert (val["ess"] >= 1.0).all() and np.allclose(val["ess"], 1.0)
    np.testing.assert_allclose(val["log_px"], val["logw_max"] - math.log(5), rtol=1e-12)


def test_ll_const_is_the_gaussian_normaliser():
    lvo = np.array([-3.0, 0.5, -1.25])
    assert LR.ll_const(lvo) == pytest.approx(float(Normal(0.0, torch.exp(0.5 * torch.tensor(lvo))).log_prob(torch.zeros(3)).sum()), rel=1e-14)
