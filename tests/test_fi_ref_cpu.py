"""tests/fi_ref.py checked without a GPU: the running fold against numpy's fp64 mean and standard deviation within the bound
the file derives, the head restated on the oracle's regression forward against golden reg3_gpoe, and seeded faults the
checker must flag -- a dropped draw, draws folded out of order, a wrong divisor, a swapped minimum / maximum."""
import numpy as np
import pytest
import torch

from oracle import cvae_ref as R
from tests import fi_ref as F
from tests.golden_util import Golden

f32 = np.float32


def _draws(N, S, seed, scale=1.0, offset=0.0):
    g = np.random.default_rng(seed)
    return (offset + scale * g.standard_normal((N, S))).astype(f32)


@pytest.mark.parametrize("S", [1, 2, 5, 64])
@pytest.mark.parametrize("scale,offset", [(1.0, 0.0), (1e-3, 40.0), (50.0, -3.0)])
def test_fold_against_fp64(S, scale, offset):
    p = _draws(257, S, 11 * S, scale, offset)
    mean, m2, lo, hi = F.fold(p)
    mean64, bm, sd64, bs = F.fold_bounds(p)
    assert (np.abs(mean.astype(np.float64) - mean64) <= bm).all()
    t = F.row_table(p, [np.ones(257, f32)], np.zeros((257, 4), f32), np.zeros((257, 4), f32), None)
    assert (np.abs(t["fi_sd"].astype(np.float64) - sd64) <= bs).all()
    share = float((np.abs(mean.astype(np.float64) - mean64) / bm).max())
    print(f"S = {S}: worst share of the mean's bound {share:.3f}")
    assert np.array_equal(lo, p.min(axis=1)) and np.array_equal(hi, p.max(axis=1))
    if S == 1:
        assert np.array_equal(mean, p[:, 0]) and not m2.any() and not t["fi_sd"].any()


def test_row_table_columns():
    N, S, Z = 40, 5, 10
    g = np.random.default_rng(3)
    p = _draws(N, S, 5)
    dev = [np.abs(g.standard_normal(N)).astype(f32) for _ in range(3)]
    mu, lv = g.standard_normal((N, Z)).astype(f32), (0.3 * g.standard_normal((N, Z))).astype(f32)
    tgt = g.random(N).astype(f32)
    t = F.row_table(p, dev, mu, lv, tgt)
    assert set(t) == set(F.COLUMNS)
    assert np.array_equal(t["err"], (t["fi_pred"] - tgt).astype(f32))
    assert np.array_equal(t["dev"], (((dev[0] + dev[1]).astype(f32) + dev[2]).astype(f32) / f32(3)).astype(f32))
    val, bnd = F.kl_reference64(mu, lv)
    assert (np.abs(t["kl"].astype(np.float64) - val) <= bnd).all()
    assert not t["status"].any()
    assert (F.row_table(p, dev, mu, lv, None)["status"] == 2).all() and not F.row_table(p, dev, mu, lv, None)["err"].any()
    p[7, 2] = np.inf
    dev[1][9] = np.nan
    st = F.row_table(p, dev, mu, lv, None)["status"]
    assert st[7] == 3 and st[9] == 3 and (np.delete(st, [7, 9]) == 2).all()


def test_head_on_the_oracle_forward_reproduces_golden_reg3():
    """The restated head on the residuals of oracle.cvae_ref's forward: golden reg3_gpoe's fi_pred at the tolerance
    tests/test_oracle_heads.py holds the oracle itself to."""
    g = Golden("reg3_gpoe")
    spec = R.Spec(g.dims, g.hidden, g.Z, g.c_dim, kind="regression")
    P = g.weights("w0")
    xes, c = g.xs(0), g.t("c")[0]
    fwd = R.forward_regression(P, spec, xes, [c] * g.M, g.combine, g.t("eps")[0])
    resid = torch.cat([xes[m] - fwd["locs"][m] for m in range(g.M)], dim=1).detach().numpy()
    got = F.head(resid, *[P[f"regressor.{i}.{k}"].numpy() for i in (0, 2, 4) for k in ("weight", "bias")])
    torch.testing.assert_close(torch.from_numpy(got), g.t("fi_pred").reshape(-1), rtol=1e-5, atol=1e-6)


def _case(S=5, N=64, Z=10):
    g = np.random.default_rng(17)
    p = _draws(N, S, 23)
    dev = [np.abs(g.standard_normal(N)).astype(f32) for _ in range(2)]
    mu, lv = g.standard_normal((N, Z)).astype(f32), (0.3 * g.standard_normal((N, Z))).astype(f32)
    tgt = g.random(N).astype(f32)
    t = F.row_table(p, dev, mu, lv, tgt)
    row = np.stack([t[n] for n in F.COLUMNS], axis=1)
    return row, p, dev, mu, lv, tgt


def test_checker_accepts_the_restatement_and_flags_seeded_faults():
    row, p, dev, mu, lv, tgt = _case()
    wrong, share = F.check_table(row, p, dev, mu, lv, tgt)
    assert not wrong and share <= 1.0
    C = F.COLUMNS.index
    S = p.shape[1]

    def table_of(mean, m2, lo, hi, div):
        bad = row.copy()
        bad[:, C("fi_pred")] = mean
        bad[:, C("fi_sd")] = np.sqrt((m2 * (f32(1.0) / f32(div))).astype(f32))
        bad[:, C("fi_min")], bad[:, C("fi_max")] = lo, hi
        bad[:, C("err")] = (mean - tgt).astype(f32)
        return bad

    # a dropped draw: the fold of the first S - 1 draws
    w, _ = F.check_table(table_of(*F.fold(p[:, :-1]), S - 2), p, dev, mu, lv, tgt)
    assert "fi_pred" in w and "fi_sd" in w
    # draws folded out of order: the same numbers, another order of operations
    m_rev, m2_rev, lo_rev, hi_rev = F.fold(p[:, ::-1])
    assert np.array_equal(lo_rev, row[:, C("fi_min")])                   # (the extremes do not depend on the order)
    w, _ = F.check_table(table_of(m_rev, m2_rev, lo_rev, hi_rev, S - 1), p, dev, mu, lv, tgt)
    assert "fi_pred" in w or "fi_sd" in w
    # a wrong divisor: the population standard deviation
    m, m2, lo, hi = F.fold(p)
    w, _ = F.check_table(table_of(m, m2, lo, hi, S), p, dev, mu, lv, tgt)
    assert w == ["fi_sd"]
    # minimum and maximum swapped
    w, _ = F.check_table(table_of(m, m2, hi, lo, S - 1), p, dev, mu, lv, tgt)
    assert w == ["fi_min", "fi_max"]
    # a kl outside its bound
    bad = row.copy()
    bad[:, C("kl")] *= f32(1.001)
    w, share = F.check_table(bad, p, dev, mu, lv, tgt)
    assert w == ["kl"] and share > 1.0
