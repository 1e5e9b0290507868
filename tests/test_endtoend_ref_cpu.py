"""tests/endtoend_ref.py -- the numpy restatement of nm_e2e_pass' row table -- against torch.softmax / torch.argmax and
against the oracle's eval-mode forward of the end-to-end model on golden e2e3; its exact columns with ==, p_disease and kl
within the bounds the restatement derives.  No GPU."""
import numpy as np
import pytest
import torch

from multi_modal_normative_modeling_amd import metrics
from oracle import cvae_ref as R
from tests import endtoend_ref as E
from tests.golden_util import Golden


def _inputs(N, C, Me, Z, seed, scale=3.0):
    rng = np.random.default_rng(seed)
    logits = (scale * rng.normal(size=(N, C))).astype(np.float32)
    dev = [rng.gamma(2.0, 0.5, size=N).astype(np.float32) for _ in range(2 * Me)]
    mu = rng.normal(size=(N, Z)).astype(np.float32)
    lv = (0.7 * rng.normal(size=(N, Z)) - 0.5).astype(np.float32)
    return logits, dev, mu, lv


def test_columns_are_the_package_constant():
    assert E.COLUMNS == metrics.ENDTOEND_ROW_COLUMNS and len(E.COLUMNS) == 8


@pytest.mark.parametrize("C", [2, 3, 4])
@pytest.mark.parametrize("Me,Z", [(1, 1), (3, 10), (3, 64), (4, 33), (2, 16)])
def test_restatement_against_torch(C, Me, Z):
    logits, dev, mu, lv = _inputs(257, C, Me, Z, seed=10 * C + Me)
    t = E.row_table(logits, dev, mu, lv)
    lg = torch.from_numpy(logits)
    sm = torch.softmax(lg.double(), dim=1)
    val, bnd = E.reference64(logits, mu, lv)
    assert np.abs(val["p_disease"] - (1.0 - sm[:, 0].numpy())).max() < 1e-14
    assert E.worst_ratio(t["p_disease"], val["p_disease"], bnd["p_disease"]) <= 1.0
    assert E.worst_ratio(t["kl"], val["kl"], bnd["kl"]) <= 1.0
    assert float(bnd["p_disease"].max()) < 1e-6                        # (the bound is a few ulp, not a tolerance in disguise)
    kl_t = -0.5 * torch.sum(1 + torch.from_numpy(lv) - torch.from_numpy(mu).pow(2) - torch.from_numpy(lv).exp(), dim=1)
    assert E.worst_ratio(kl_t.numpy(), val["kl"], bnd["kl"]) <= 1.0     # calc_kl without the batch mean, in fp32
    # the exact columns
    assert (t["pred"] == torch.argmax(lg, dim=1).numpy().astype(np.float32)).all()
    assert (t["margin"] == (lg[:, 1:].max(dim=1).values - lg[:, 0]).numpy()).all()
    d = [torch.from_numpy(x) for x in dev]
    dh, dd = d[0], d[Me]
    for m in range(1, Me):
        dh, dd = dh + d[m], dd + d[Me + m]
    dh, dd = dh / Me, dd / Me
    assert (t["dev_health"] == dh.numpy()).all() and (t["dev_disease"] == dd.numpy()).all()
    assert (t["contrast"] == (dh - dd).numpy()).all()
    assert (t["status"] == 0).all()
    assert all(v.dtype == np.float32 and v.shape == (257,) for v in t.values())


def test_exact_ties_take_the_first_index():
    logits = np.array([[1.5, 1.5, 1.5, 1.5], [0.0, 2.0, 2.0, 1.0], [-1.0, -3.0, -1.0, -1.0], [0.25, 0.5, 0.125, 0.5]], np.float32)
    _, dev, mu, lv = _inputs(4, 4, 1, 4, seed=1)
    t = E.row_table(logits, dev, mu, lv)
    assert t["pred"].tolist() == [0.0, 1.0, 0.0, 1.0]
    assert t["pred"].tolist() == torch.argmax(torch.from_numpy(logits), dim=1).float().tolist()
    assert t["margin"].tolist() == [0.0, 2.0, 0.0, 0.25]
    assert t["p_disease"][0] == np.float32(0.75)
    two = E.row_table(logits[:, :2], dev, mu, lv)
    assert two["pred"].tolist() == [0.0, 1.0, 0.0, 1.0] and two["p_disease"][0] == np.float32(0.5)


def test_logits_eighty_apart_give_no_inf_and_no_nan():
    logits = np.array([[80.0, 0.0], [0.0, 80.0], [-40.0, 40.0], [88.0, -88.0], [3.0e4, -3.0e4]], np.float32)
    _, dev, mu, lv = _inputs(5, 2, 3, 10, seed=2)
    t = E.row_table(logits, dev, mu, lv)
    assert np.isfinite(t["p_disease"]).all() and np.isfinite(t["margin"]).all()
    assert t["p_disease"][1] == 1.0 and t["p_disease"][2] == 1.0 and t["p_disease"][3] == 0.0
    assert 0.0 <= t["p_disease"][0] < 1e-30
    assert t["pred"].tolist() == [0.0, 1.0, 1.0, 0.0, 0.0] and (t["status"] == 0).all()
    val, bnd = E.reference64(logits, mu, lv)
    assert E.worst_ratio(t["p_disease"], val["p_disease"], bnd["p_disease"]) <= 1.0


def test_status_flags_every_non_finite_source():
    logits, dev, mu, lv = _inputs(6, 3, 2, 5, seed=3)
    logits[1, 2] = np.nan
    dev[3][2] = np.inf
    mu[3, 4] = np.nan
    lv[4, 0] = -np.inf
    t = E.row_table(logits, dev, mu, lv)
    assert t["status"].tolist() == [0.0, 1.0, 1.0, 1.0, 1.0, 0.0]


def test_restatement_against_the_oracle_on_golden_e2e3():
    """oracle.cvae_ref.forward_endtoend(training=False) + classifier_fwd on the joint mean (predict, cVAE.py:2202-2207): the
    restatement fed with the oracle's logits and deviations gives the oracle's own softmax, argmax, compute_deviation means
    and per-subject KL."""
    g = Golden("e2e3")
    layers = [int(v) for v in g.z["layers"]]
    spec = R.Spec(g.dims, g.hidden, g.Z, g.c_dim, True, kind="endtoend", classifier_layers=layers)
    P = {k: v for k, v in g.weights(f"w{g.n_steps}").items()}
    bn = {k: v for k, v in P.items() if "running" in k}
    xes, c = g.xs(0), g.t("c")[0]
    of = R.forward_endtoend(P, spec, xes, [c] * g.M, torch.zeros(g.B, g.Z), training=False, bn_stats=bn)
    logits = R.classifier_fwd(P, spec, of["mu"], False, bn)
    dev = [((xes[m] - of[key][m]) ** 2).mean(dim=1) for key in ("locs_h", "locs_d") for m in range(g.M)]
    t = E.row_table(logits.numpy(), [d.numpy() for d in dev], of["mu"].numpy(), of["logvar"].numpy())
    sm = torch.softmax(logits.double(), dim=1)
    val, bnd = E.reference64(logits.numpy(), of["mu"].numpy(), of["logvar"].numpy())
    assert np.abs(val["p_disease"] - sm[:, 1].numpy()).max() < 1e-14
    assert E.worst_ratio(t["p_disease"], val["p_disease"], bnd["p_disease"]) <= 1.0
    assert (t["pred"] == torch.argmax(logits, dim=1).numpy()).all()
    assert (t["margin"] == (logits[:, 1] - logits[:, 0]).numpy()).all()
    dev_h, dev_d = torch.stack(dev[: g.M]).double().mean(dim=0), torch.stack(dev[g.M:]).double().mean(dim=0)
    np.testing.assert_allclose(t["dev_health"], dev_h.numpy(), rtol=4 * 2.0 ** -24)     # (M - 1 additions and a division)
    np.testing.assert_allclose(t["dev_disease"], dev_d.numpy(), rtol=4 * 2.0 ** -24)
    assert (t["contrast"] == t["dev_health"] - t["dev_disease"]).all()
    kl = -0.5 * torch.sum(1 + of["logvar"].double() - of["mu"].double().pow(2) - of["logvar"].double().exp(), dim=1)
    assert E.worst_ratio(t["kl"], kl.numpy(), bnd["kl"]) <= 1.0
    assert (t["status"] == 0).all()
