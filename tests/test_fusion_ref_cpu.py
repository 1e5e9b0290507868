"""tests/fusion_ref.py held to the oracle and to itself, no GPU: the float64 yardstick equals oracle.cvae_ref's combine_latent /
mvt_combine and reproduces tests/golden/fusion_ops.npz; the float32 twins of the kernels stay inside the derived ceilings and
inside the working bounds on every shared case (so a correct implementation can satisfy them); every planted fault, applied to
a twin, breaks the bound (so the cases can see it); the metamorphic identities hold on the yardstick."""
import numpy as np
import pytest
import torch

from oracle import cvae_ref as R
from tests import fusion_ref as F
from tests.golden_util import GOLDEN


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN / "fusion_ops.npz")


def test_fuse_ref_equals_the_oracle_in_float64(golden):
    mus, variances = torch.from_numpy(golden["mus"]).double(), torch.from_numpy(golden["variances"]).double()
    alpha = golden["alpha"]
    alphas = [torch.tensor(float(a), dtype=torch.float64) for a in alpha]
    for comb in F.COMBINERS:
        for bypass, m_used in ((True, 3), (True, 1), (False, 1)):
            mu_o, var_o = R.combine_latent(mus[:m_used], variances[:m_used], comb, alphas[:m_used], single_bypass=bypass)
            mu, var, _ = F.fuse_ref(golden["mus"][:m_used], golden["variances"][:m_used], comb, alpha[:m_used], single_bypass=bypass)
            np.testing.assert_allclose(mu, mu_o.numpy(), rtol=1e-13, atol=0, err_msg=f"{comb} {bypass} {m_used}")
            np.testing.assert_allclose(var, var_o.numpy(), rtol=1e-13, atol=0, err_msg=f"{comb} {bypass} {m_used}")
        for scale in (1.0, 1e-8):                                          # (1e-8: the clamp at 1e-6 takes hold)
            v32 = (np.float32(scale) * golden["variances"]).astype(np.float32)
            mu_o, var_o = R.mvt_combine(mus, torch.from_numpy(v32).double(), comb, alphas)
            poe2 = comb == "poe"
            mu, var, _ = F.fuse_ref(golden["mus"], v32, comb, alpha, in_log=poe2, out_log=poe2, var_floor=R.MVT_VAR_FLOOR)
            np.testing.assert_allclose(mu, mu_o.numpy(), rtol=1e-13, atol=0, err_msg=comb)
            np.testing.assert_allclose(var, var_o.numpy(), rtol=1e-13, atol=1e-6 * 2.0 ** -24, err_msg=comb)   # (1e-6 as fp32)
    tc, _ = F.tc_ref(golden["mus"])
    want = float(R.mvt_total_correlation(list(mus), mus.mean(0), mus.shape[2]))
    assert abs(tc - want) <= 1e-13 * abs(want)


def test_fuse_ref_reproduces_the_fixture(golden):
    """Every array of fusion_ops.npz within the fixture test's own tolerance (rtol 2e-6, atol 1e-7; 2e-6 on the sum)."""
    mus, variances, alpha = golden["mus"], golden["variances"], golden["alpha"]
    seen = set()

    def close(got, key):
        seen.add(key)
        np.testing.assert_allclose(got, golden[key], rtol=2e-6, atol=1e-7, err_msg=key)

    for cname in ("cVAE_multimodal", "cVAE_multimodal_regression", "mvtCAE"):
        mvt = cname == "mvtCAE"
        for comb in F.COMBINERS:
            poe2 = mvt and comb == "poe"
            mu, var, _ = F.fuse_ref(mus, variances, comb, alpha, single_bypass=not mvt, in_log=poe2, out_log=poe2,
                                    var_floor=1e-6 if mvt else 0.0)
            close(mu, f"{cname}.combine_latent.{comb}.mu"); close(var, f"{cname}.combine_latent.{comb}.var")
        for meth, comb in (("product_of_experts", "poe"), ("mixture_of_experts", "moe"), ("mixture_of_product_of_experts", "mopoe")):
            poe2 = mvt and comb == "poe"
            mu, var, _ = F.fuse_ref(mus, variances, comb, in_log=poe2, out_log=poe2)
            close(mu, f"{cname}.{meth}.mu"); close(var, f"{cname}.{meth}.var")
        if not mvt:
            mu, var, _ = F.fuse_ref(mus[:1], variances[:1], "gpoe", alpha[:1], single_bypass=True)
            close(mu, f"{cname}.combine_latent.single.mu"); close(var, f"{cname}.combine_latent.single.var")
        else:
            mu, var, _ = F.fuse_ref(mus, np.float32(1e-8) * variances, "moe", var_floor=1e-6)
            close(mu, "mvtCAE.combine_latent.clamped.mu"); close(var, "mvtCAE.combine_latent.clamped.var")
            tc, _ = F.tc_ref(mus)
            seen.add("mvtCAE.total_correlation")
            assert abs(tc - float(golden["mvtCAE.total_correlation"])) <= 2e-6 * abs(tc)
    mu, var, _ = F.fuse_ref(mus, np.log(variances), "poe", in_log=True)
    close(mu, "mmJSD.combine_latent.mu"); close(var, "mmJSD.combine_latent.var")
    assert seen == set(golden.files) - {"meta", "mus", "variances", "alpha"}


def _twin_ratios(combine):
    """Worst (mean, variance) ratio of the twin per (in_log, out_log) group over FUSE_CASES[combine], and the case that set it."""
    worst = {}
    for case in F.FUSE_CASES[combine]:
        M, n, il, ol, bp, fl, _, _, _ = case
        mus, vin, al = F.fuse_inputs(case)
        ref = F.fuse_ref(mus, vin, combine, al, bp, il, ol, fl)
        tm, tv = F.fuse_twin(mus, vin, combine, al if combine == "gpoe" else None, bp, il, ol, fl)
        r = F.fuse_errors(tm, tv, ref, ol)
        w = worst.setdefault((il, ol), [0.0, 0.0, None])
        if max(r) > max(w[:2]):
            w[2] = case
        w[0], w[1] = max(w[0], r[0]), max(w[1], r[1])
    return worst


@pytest.mark.parametrize("combine", F.COMBINERS)
def test_fuse_twin_stays_within_the_bounds(combine):
    """The kernel's arithmetic in float32 against the yardstick: inside the a-priori ceiling, a quarter of the working k, and
    where the recorded constants say (5 % for another build of numpy's expf / logf)."""
    for (il, ol), (r_mu, r_var, _) in sorted(_twin_ratios(combine).items()):
        rec, k = F.TWIN_FUSE[(combine, il, ol)], F.k_fuse(combine, il, ol)
        print(f"{combine} in_log={il} out_log={ol}: twin mean {r_mu:.2f} var {r_var:.2f} (recorded {rec[0]}, {rec[1]}), k = {k:.1f}")
        assert F.K_FLOOR <= k <= F.K_CEILING
        assert max(r_mu, r_var) <= F.K_CEILING and 4.0 * max(r_mu, r_var) <= 1.05 * k
        assert r_mu <= 1.05 * rec[0] and r_var <= 1.05 * rec[1]
        assert max(r_mu, r_var) >= 0.5 * max(rec), "the recorded ratio is far from what the twin gives"


@pytest.mark.parametrize("combine", F.COMBINERS)
def test_fuse_twin_on_non_finite_inputs(combine):
    """float32 arithmetic in the kernel's order yields the yardstick's NaN / +-inf at the same elements, for every flag."""
    for il in (0, 1):
        for ol in (0, 1):
            for fl in (0.0, 1e-6):
                mus, vin, al = F.nonfinite_inputs(il)
                ref = F.fuse_ref(mus, vin, combine, al, False, il, ol, fl)
                assert not np.isfinite(ref[0]).all() and np.isfinite(ref[0]).any() and np.isnan(ref[1][6])
                r = F.fuse_errors(*F.fuse_twin(mus, vin, combine, al if combine == "gpoe" else None, False, il, ol, fl), ref, ol)
                assert F.within(r, F.k_fuse(combine, il, ol)), (il, ol, fl, r)


@pytest.mark.parametrize("combine", F.COMBINERS)
def test_a_nan_or_an_infinity_where_the_yardstick_is_finite_breaks_the_bound(combine):
    """The comparator itself: one NaN, +inf or -inf planted in either output of the sound twin, at an element where the
    yardstick is finite, leaves the bound -- also in the second ratio, also at the last element of several blocks, also when
    it replaces a whole output; and a finite value where the yardstick is NaN does."""
    case = next(c for c in F.FUSE_CASES[combine] if c[0] == 8 and c[1] == 4099 and c[3] == 1 and c[5] > 0)
    M, n, il, ol, bp, fl, _, _, _ = case
    mus, vin, al = F.fuse_inputs(case)
    ref = F.fuse_ref(mus, vin, combine, al, bp, il, ol, fl)
    k = F.k_fuse(combine, il, ol)
    sound = F.fuse_twin(mus, vin, combine, al if combine == "gpoe" else None, bp, il, ol, fl)
    assert F.within(F.fuse_errors(*sound, ref, ol), k)
    for which in (0, 1):
        for bad in (np.nan, np.inf, -np.inf):
            for at in (0, n - 1, slice(None)):
                out = [sound[0].copy(), sound[1].copy()]
                out[which][at] = bad
                r = F.fuse_errors(*out, ref, ol)
                assert not np.isnan(r[0]) and not np.isnan(r[1]) and r[which] == np.inf, (which, bad, at, r)
                assert not F.within(r, k) and not max(r) <= k and not max(r[::-1]) <= k
    mus, vin, al = F.nonfinite_inputs(0)
    ref = F.fuse_ref(mus, vin, combine, al, False, 0, 0, 1e-6)
    mu, var = F.fuse_twin(mus, vin, combine, al if combine == "gpoe" else None, False, 0, 0, 1e-6)
    assert np.isnan(ref[1][6]) and np.isnan(var[6]) and F.within(F.fuse_errors(mu, var, ref, 0), F.k_fuse(combine, 0, 0))
    var[6] = np.float32(1e-6)                                              # what a clamp by fmaxf makes of the NaN variance
    assert not F.within(F.fuse_errors(mu, var, ref, 0), F.k_fuse(combine, 0, 0))


@pytest.mark.parametrize("fault,combine,named", [
    ("loop_bound", "poe", lambda c: c[0] == 8), ("loop_bound", "moe", lambda c: c[0] == 8),
    ("alpha_swap", "gpoe", lambda c: c[0] >= 2),
    ("mopoe_div", "mopoe", lambda c: c[0] >= 2),
    ("floor_before_log", "poe", lambda c: c[3] == 1 and c[5] > 0 and c[0] >= 2),
])
def test_planted_faults_break_the_fuse_bound(fault, combine, named):
    """Each mistake of the list, planted in the twin, leaves the bound on the cases named for it (and on no case it cannot
    touch: the sound twin passes all of them above)."""
    hit = 0
    for case in filter(named, F.FUSE_CASES[combine]):
        M, n, il, ol, bp, fl, _, _, _ = case
        mus, vin, al = F.fuse_inputs(case)
        ref = F.fuse_ref(mus, vin, combine, al, bp, il, ol, fl)
        r = F.fuse_errors(*F.fuse_twin(mus, vin, combine, al if combine == "gpoe" else None, bp, il, ol, fl, fault=fault), ref, ol)
        hit += not F.within(r, F.k_fuse(combine, il, ol))
        if n >= 255:                                                       # (with a few elements a fault may land on none)
            assert not F.within(r, F.k_fuse(combine, il, ol)), (fault, case, r)
    assert hit


def test_tc_twin_stays_within_the_bound_and_faults_break_it():
    worst, caught = 0.0, {f: [] for f in F.TC_FAULTS}
    for case in F.TC_CASES:
        q = F.tc_inputs(case)
        ref, A = F.tc_ref(q)
        worst = max(worst, abs(F.tc_twin(q) - ref) / (F.EPS32 * A))
        for f in F.TC_FAULTS:
            if not abs(F.tc_twin(q, fault=f) - ref) <= F.K_TC * F.EPS32 * A:
                caught[f].append(case[:4])
    print(f"tc twin: worst ratio {worst:.2f} (recorded {F.TWIN_TC_RATIO}), k = {F.K_TC:.1f}")
    assert 0.5 * F.TWIN_TC_RATIO <= worst <= 1.05 * F.TWIN_TC_RATIO and 4.0 * worst <= 1.05 * F.K_TC
    # the truncated row loop drops rows whenever B is no multiple of 64; a zero start of the max shows on the -90 offset only
    assert {c[1] for c in caught["row_loop_trunc"]} == {1, 63, 65, 200, 1000}
    # (... and on single far-negative rows of the widest spread, whose expf leaves the normal range the same way)
    kinds = {c[3] for c in caught["max_init_zero"]}
    assert "minus90" in kinds and kinds <= {"minus90", "spread30"}
    # every entry equal to c: exactly -Z (c + log B)
    for c, B, Z in ((0.75, 200, 6), (-90.0, 65, 128), (30.0, 1, 1)):
        q = np.full((3, B, Z), c, np.float32)
        ref, A = F.tc_ref(q)
        assert abs(ref + Z * (c + np.log(B))) <= 1e-13 * A
        assert abs(F.tc_twin(q) - ref) <= F.K_TC * F.EPS32 * A


def test_stats_twin_is_correctly_rounded_and_faults_break_it():
    """The chunked two-pass sums and the Chan merge in float64, rounded once: within 1 ulp of np.mean / np.var on every case
    (in fact the nearest fp32).  The two planted faults show on every case that crosses a round boundary (cnt) or has more
    than one chunk (the index), and only there."""
    for n, Z in F.LATENT_CASES:
        per, nch = 256 // Z, (n + 127) // 128
        for kind in F.LATENT_KINDS:
            x = F.latent_inputs(n, Z, kind)
            x64 = x.astype(np.float64)
            mean, var = F.stats_twin(x)
            assert F.ulps32(mean, x64.mean(0)).max() <= 1 and F.ulps32(var, x64.var(0)).max() <= 1, (n, Z, kind)
            for fault, expect in (("cnt_not_carried", nch > per), ("merge_per_index", nch > 1 and per != Z)):
                mf, vf = F.stats_twin(x, fault=fault)
                bad = F.ulps32(mf, x64.mean(0)).max() > 1 or F.ulps32(vf, x64.var(0)).max() > 1
                assert bad == expect, (n, Z, kind, fault)
    m0, v0 = F.stats_twin(np.zeros((0, 5), np.float32))
    assert np.isnan(m0).all() and np.isnan(v0).all()
    one = F.latent_inputs(1, 64, "offset1e4")
    m1, v1 = F.stats_twin(one)
    assert np.array_equal(m1, one[0]) and not v1.any()


@pytest.mark.parametrize("M", [2, 3, 8])
def test_metamorphic_identities_on_the_yardstick(M):
    rng = np.random.default_rng(M)
    mus = rng.standard_normal((M, 257)).astype(np.float32)
    var = np.exp(0.7 * rng.standard_normal((M, 257))).astype(np.float32)
    alpha = (3 * rng.standard_normal(M)).astype(np.float32)
    poe = F.fuse_ref(mus, var, "poe")
    moe = F.fuse_ref(mus, var, "moe")
    # equal alpha_raw: PoE's mean, M x PoE's variance
    g = F.fuse_ref(mus, var, "gpoe", np.full(M, 1.25, np.float32))
    np.testing.assert_allclose(g[0], poe[0], rtol=0, atol=1e-14 * poe[2].max())
    np.testing.assert_allclose(g[1], M * poe[1], rtol=1e-14)
    # a permutation of the experts, with their alphas
    p = rng.permutation(M)
    for comb in F.COMBINERS:
        a, b = F.fuse_ref(mus, var, comb, alpha), F.fuse_ref(mus[p], var[p], comb, alpha[p])
        np.testing.assert_allclose(b[0], a[0], rtol=0, atol=1e-14 * a[2].max())
        np.testing.assert_allclose(b[1], a[1], rtol=1e-14)
        np.testing.assert_allclose(b[2], a[2], rtol=1e-14)
    # MoPoE = (M moe + poe) / (M + 1)
    mo = F.fuse_ref(mus, var, "mopoe")
    np.testing.assert_allclose(mo[0], (M * moe[0] + poe[0]) / (M + 1), rtol=0, atol=1e-14 * mo[2].max())
    np.testing.assert_allclose(mo[1], (M * moe[1] + poe[1]) / (M + 1), rtol=1e-14)
