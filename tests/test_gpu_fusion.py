"""nm_combine_latent / nm_total_correlation (csrc/nm_fusion.hip) on the GPU against the float64 yardstick of
tests/fusion_ref.py, through the C ABI: every combiner, expert count, flag combination and block edge, the bypass bit for bit,
non-finite inputs, the shapes the classes accept, the autograd branch of _ExpertOps._fuse, the strided row loop and the whole
lse array of the total-correlation kernel.  The bounds are the ones derived and measured on the CPU twins (tests/fusion_ref.py);
every buffer a kernel writes carries one slack element holding a canary inside the same allocation."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import multi_modal_normative_modeling_amd.api as api
from multi_modal_normative_modeling_amd import _lib
from tests import fusion_ref as F

DEV = "cuda:0"
CANARY = -12345.678
EPS = F.EPS32


def _padded(a):
    """The array on the device, flat, with one slack element behind it in the same allocation."""
    t = torch.full((a.size + 1,), CANARY, dtype=torch.float32)
    t[:a.size] = torch.from_numpy(np.ascontiguousarray(a, np.float32).ravel())
    return t.to(DEV)


def _combine(mus, vin, combine, alpha=None, bypass=0, in_log=0, out_log=0, floor=0.0):
    """The flat call: mus / vin [M, n] numpy -> (mu, var) numpy [n].  Asserts that the canaries behind both outputs stand."""
    M, n = mus.shape
    d_mu, d_v = _padded(mus), _padded(vin)
    d_al = torch.from_numpy(np.asarray(alpha, np.float32)).to(DEV) if alpha is not None else None
    out = torch.full((2, n + 1), CANARY, dtype=torch.float32, device=DEV)
    st = torch.cuda.current_stream().cuda_stream
    _lib.check(_lib.load().nm_combine_latent(d_mu.data_ptr(), d_v.data_ptr(), M, n, _lib.NM_COMBINE[combine],
                                             d_al.data_ptr() if d_al is not None else None, int(bypass), int(in_log), int(out_log),
                                             float(floor), out[0].data_ptr(), out[1].data_ptr(), st), "nm_combine_latent")
    o = out.cpu().numpy()
    assert o[0, n] == np.float32(CANARY) and o[1, n] == np.float32(CANARY), "a write behind the end of an output"
    return o[0, :n].copy(), o[1, :n].copy()


def _alpha_for(combine, al):
    return al if combine == "gpoe" else None


@pytest.mark.parametrize("combine", F.COMBINERS)
def test_combine_latent_every_case(combine):
    worst, failed = {}, []
    for case in F.FUSE_CASES[combine]:
        M, n, il, ol, bp, fl, _, _, _ = case
        mus, vin, al = F.fuse_inputs(case)
        ref = F.fuse_ref(mus, vin, combine, al, bp, il, ol, fl)
        mu, var = _combine(mus, vin, combine, _alpha_for(combine, al), bp, il, ol, fl)
        r = F.fuse_errors(mu, var, ref, ol)
        w = worst.setdefault((il, ol), [0.0, 0.0])
        w[0], w[1] = max(w[0], r[0]), max(w[1], r[1])
        if not F.within(r, F.k_fuse(combine, il, ol)):
            failed.append((case, r))
    for (il, ol), w in sorted(worst.items()):
        print(f"nm_combine_latent {combine} in_log={il} out_log={ol}: device mean {w[0]:.2f} var {w[1]:.2f} "
              f"(twin {F.TWIN_FUSE[(combine, il, ol)]}), k = {F.k_fuse(combine, il, ol):.1f}")
    assert not failed, failed[:5]


@pytest.mark.parametrize("n", [1, 257, 4099])
def test_single_expert_bypass_is_the_input_bit_for_bit(n):
    rng = np.random.default_rng(n)
    mus = (rng.standard_normal((1, n)) * 1e3).astype(np.float32)
    lv = (8.0 * rng.standard_normal((1, n))).astype(np.float32)
    var = np.exp(lv.astype(np.float64)).astype(np.float32)
    for combine in F.COMBINERS:
        al = np.array([0.3], np.float32) if combine == "gpoe" else None
        mu, v = _combine(mus, var, combine, al, bypass=1)
        assert np.array_equal(mu.view(np.uint32), mus[0].view(np.uint32)) and np.array_equal(v.view(np.uint32), var[0].view(np.uint32))
        mu, v = _combine(mus, lv, combine, al, bypass=1, in_log=1)
        assert np.array_equal(mu.view(np.uint32), mus[0].view(np.uint32))
        assert F.ulps32(v, np.exp(lv[0].astype(np.float64))).max() <= 1.0                          # expf: 1 ulp


@pytest.mark.parametrize("combine", F.COMBINERS)
def test_non_finite_inputs_give_the_yardsticks_non_finite_outputs(combine):
    """Zero and infinite variances, an infinite mean, a NaN variance: non-finite exactly where the yardstick is, the same
    kind and sign; everywhere else inside the bound.  (With the floor a NaN variance stays NaN, as torch.clamp leaves it.)"""
    for il in (0, 1):
        for ol in (0, 1):
            for fl in (0.0, 1e-6):
                mus, vin, al = F.nonfinite_inputs(il)
                ref = F.fuse_ref(mus, vin, combine, al, False, il, ol, fl)
                assert not np.isfinite(ref[0]).all() and np.isfinite(ref[0]).any()
                mu, var = _combine(mus, vin, combine, _alpha_for(combine, al), 0, il, ol, fl)
                r = F.fuse_errors(mu, var, ref, ol)
                assert F.within(r, F.k_fuse(combine, il, ol)), (il, ol, fl, r, mu, ref[0], var, ref[1])
                # the NaN variance (element 6) stays NaN through the floor, as torch.clamp leaves it: fmaxf made it the floor
                assert np.isnan(ref[1][6]) and np.isnan(var[6]), (il, ol, fl, var[6])


@pytest.mark.parametrize("M", [2, 3, 8])
def test_metamorphic_identities_on_the_device(M):
    rng = np.random.default_rng(40 + M)
    n = 4099
    mus = rng.standard_normal((M, n)).astype(np.float32)
    var = np.exp(0.7 * rng.standard_normal((M, n))).astype(np.float32)
    alpha = (3 * rng.standard_normal(M)).astype(np.float32)
    k = {c: F.k_fuse(c, 0, 0) for c in F.COMBINERS}
    refs = {c: F.fuse_ref(mus, var, c, alpha) for c in F.COMBINERS}
    poe, moe, mopoe = (_combine(mus, var, c) for c in ("poe", "moe", "mopoe"))
    # equal alpha_raw: PoE's mean, M x PoE's variance
    g = _combine(mus, var, "gpoe", np.full(M, 1.25, np.float32))
    assert np.all(np.abs(g[0].astype(np.float64) - poe[0]) <= (k["gpoe"] + k["poe"]) * EPS * refs["poe"][2])
    assert np.all(np.abs(g[1].astype(np.float64) - M * poe[1].astype(np.float64)) <= (k["gpoe"] + k["poe"]) * EPS * M * refs["poe"][1])
    # a permutation of the experts, with their alphas
    p = rng.permutation(M)
    for c in F.COMBINERS:
        a, b = _combine(mus, var, c, _alpha_for(c, alpha)), _combine(mus[p], var[p], c, _alpha_for(c, alpha[p]))
        assert np.all(np.abs(a[0].astype(np.float64) - b[0]) <= 2 * k[c] * EPS * refs[c][2]), c
        assert np.all(np.abs(a[1].astype(np.float64) - b[1]) <= 2 * k[c] * EPS * refs[c][1]), c
    # MoPoE = (M moe + poe) / (M + 1)
    both = [(M * moe[i].astype(np.float64) + poe[i]) / (M + 1) for i in (0, 1)]
    ksum = k["mopoe"] + k["moe"] + k["poe"]
    assert np.all(np.abs(mopoe[0] - both[0]) <= ksum * EPS * refs["mopoe"][2])
    assert np.all(np.abs(mopoe[1] - both[1]) <= ksum * EPS * refs["mopoe"][1])


def _model(cname, M, Z, alpha=None):
    model = getattr(api, cname)([5] * M, [8, 8], Z, 2, modalities=M)
    if alpha is not None:
        sd = model.state_dict()
        for m in range(M):
            sd[f"alpha_m_list.{m}"] = torch.from_numpy(alpha[m:m + 1].copy())
        model.load_state_dict(sd)
    return model


def test_shapes_through_the_classes_equal_the_flat_call():
    M = 3
    rng = np.random.default_rng(77)
    alpha = (3 * rng.standard_normal(M)).astype(np.float32)
    model, mvt = _model("cVAE_multimodal", M, 5, alpha), _model("mvtCAE", M, 5, alpha)
    for shape in ((M, 37), (M, 19, 6), (M, 2, 3, 5)):
        mus = rng.standard_normal(shape).astype(np.float32)
        var = np.exp(0.7 * rng.standard_normal(shape)).astype(np.float32)
        flat_mu, flat_var = mus.reshape(M, -1), var.reshape(M, -1)
        for comb in F.COMBINERS:
            want = _combine(flat_mu, flat_var, comb, _alpha_for(comb, alpha), bypass=1)
            for form in ("cpu", "fp64", "strided"):
                if form == "cpu":
                    a, b = torch.from_numpy(mus), torch.from_numpy(var)
                elif form == "fp64":
                    a, b = torch.from_numpy(mus).double().to(DEV), torch.from_numpy(var).double().to(DEV)
                else:                                                  # every second element of a buffer twice as wide
                    wide = [torch.zeros(shape[:-1] + (2 * shape[-1],), device=DEV) for _ in range(2)]
                    a, b = wide[0][..., ::2], wide[1][..., ::2]
                    a.copy_(torch.from_numpy(mus)); b.copy_(torch.from_numpy(var))
                    assert not a.is_contiguous()
                mu, v = model.combine_latent(a, b, comb)
                assert tuple(mu.shape) == shape[1:] and tuple(v.shape) == shape[1:] and mu.dtype == torch.float32
                assert not mu.requires_grad and not v.requires_grad
                assert np.array_equal(mu.cpu().numpy().ravel(), want[0]) and np.array_equal(v.cpu().numpy().ravel(), want[1]), (shape, comb, form)
        # mvtCAE: ProductOfExperts2 on what it is given, the clamp
        want = _combine(flat_mu, flat_var, "poe", in_log=1, out_log=1, floor=1e-6)
        mu, v = mvt.combine_latent(torch.from_numpy(mus), torch.from_numpy(var), "poe")
        assert tuple(v.shape) == shape[1:]
        assert np.array_equal(mu.cpu().numpy().ravel(), want[0]) and np.array_equal(v.cpu().numpy().ravel(), want[1])
    # on a side stream, read back after that stream's sync
    mus, var = rng.standard_normal((M, 300, 7)).astype(np.float32), np.exp(0.7 * rng.standard_normal((M, 300, 7))).astype(np.float32)
    want = _combine(mus.reshape(M, -1), var.reshape(M, -1), "mopoe")
    a, b = torch.from_numpy(mus).to(DEV), torch.from_numpy(var).to(DEV)
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        mu, v = model.mixture_of_product_of_experts(a, b)
    side.synchronize()
    assert np.array_equal(mu.cpu().numpy().ravel(), want[0]) and np.array_equal(v.cpu().numpy().ravel(), want[1])


AUTOGRAD = [("cVAE_multimodal", c, 0, 0, 0.0) for c in F.COMBINERS] + [("mvtCAE", "poe", 1, 1, 1e-6), ("mvtCAE", "moe", 0, 0, 1e-6)]


@pytest.mark.parametrize("cname,comb,il,ol,fl", AUTOGRAD)
def test_autograd_branch_equals_the_kernel_and_float64_autograd(cname, comb, il, ol, fl):
    """Inputs that carry a graph take the torch expression: its values within the kernel's own bound of the yardstick and of
    the kernel, both input gradients against float64 autograd of the yardstick's expression at 16 eps32 of each gradient
    tensor's max; without a graph the launch returns tensors that require no gradient."""
    M, B, Z = 3, 19, 6
    rng = np.random.default_rng(5)
    alpha = (3 * rng.standard_normal(M)).astype(np.float32)
    mus = rng.standard_normal((M, B, Z)).astype(np.float32)
    var = np.exp(0.7 * rng.standard_normal((M, B, Z))).astype(np.float32)
    if il:
        var = (var * 2.0).astype(np.float32)          # read as log-variances: joint log-variance on both sides of the floor
    g_mu, g_var = rng.standard_normal((B, Z)), rng.standard_normal((B, Z))
    model = _model(cname, M, Z, alpha)
    k = F.k_fuse(comb, il, ol)
    ref = F.fuse_ref(mus, var, comb, alpha, False, il, ol, fl)

    k_mu, k_var = model.combine_latent(torch.from_numpy(mus), torch.from_numpy(var), comb)
    assert not k_mu.requires_grad and not k_var.requires_grad
    a = torch.from_numpy(mus).to(DEV).requires_grad_(True)
    b = torch.from_numpy(var).to(DEV).requires_grad_(True)
    t_mu, t_var = model.combine_latent(a, b, comb)
    assert t_mu.requires_grad and t_var.requires_grad and tuple(t_mu.shape) == (B, Z)
    for got in ((t_mu.detach().cpu().numpy(), t_var.detach().cpu().numpy()), (k_mu.cpu().numpy(), k_var.cpu().numpy())):
        r = F.fuse_errors(got[0], got[1], ref, ol)
        print(f"{cname} {comb}: ratios {r[0]:.2f} {r[1]:.2f} (k = {k:.1f})")
        assert F.within(r, k), r
    assert np.all(np.abs(t_mu.detach().cpu().numpy().astype(np.float64) - k_mu.cpu().numpy()) <= 2 * k * EPS * ref[2])
    loss = (t_mu.double() * torch.from_numpy(g_mu).to(DEV)).sum() + (t_var.double() * torch.from_numpy(g_var).to(DEV)).sum()
    loss.backward()

    a64 = torch.from_numpy(mus).double().requires_grad_(True)
    b64 = torch.from_numpy(var).double().requires_grad_(True)
    al = torch.softmax(torch.from_numpy(alpha).double(), 0)
    r_mu, r_var, _ = F.fuse_expr(a64, b64, comb, al, False, il, ol, fl)
    ((r_mu * torch.from_numpy(g_mu)).sum() + (r_var * torch.from_numpy(g_var)).sum()).backward()
    for name, got, want in (("mus", a.grad, a64.grad), ("variances", b.grad, b64.grad)):
        err = float((got.cpu().double() - want).abs().max()) / float(want.abs().max())
        print(f"{cname} {comb}: d/d{name} off by {err / EPS:.2f} eps32 of its max (bound 16)")
        assert err <= 16 * EPS, (name, err)


# ---- nm_total_correlation ------------------------------------------------------------------------------------------------
def _tc(q):
    M, B, Z = q.shape
    d_q = _padded(q)
    out = torch.full((2,), CANARY, dtype=torch.float32, device=DEV)
    _lib.check(_lib.load().nm_total_correlation(d_q.data_ptr(), M, B, Z, out.data_ptr(), torch.cuda.current_stream().cuda_stream),
               "nm_total_correlation")
    o = out.cpu().numpy()
    assert o[1] == np.float32(CANARY)
    return o[0]


def test_total_correlation_every_case():
    worst, failed = {}, []
    for case in F.TC_CASES:
        q = F.tc_inputs(case)
        ref, A = F.tc_ref(q)
        got = _tc(q)
        again = _tc(q)
        assert got.view(np.uint32) == again.view(np.uint32), case           # the same bits run to run
        r = abs(float(got) - ref) / (EPS * A)
        worst[case[3]] = max(worst.get(case[3], 0.0), r)
        if not r <= F.K_TC:
            failed.append((case, r, float(got), ref))
    print("nm_total_correlation: device worst ratio per input kind", {k: round(v, 2) for k, v in worst.items()},
          f"(twin {F.TWIN_TC_RATIO}), k = {F.K_TC:.1f}")
    assert not failed, failed[:5]


@pytest.mark.parametrize("c,M,B,Z", [(0.75, 3, 200, 6), (-90.0, 8, 65, 128), (30.0, 1, 1, 1), (2.5, 2, 1000, 127)])
def test_total_correlation_of_equal_entries(c, M, B, Z):
    """Every entry c: exactly -Z (c + log B)."""
    q = np.full((M, B, Z), c, np.float32)
    want = -Z * (c + np.log(B))
    _, A = F.tc_ref(q)
    assert abs(float(_tc(q)) - want) <= F.K_TC * EPS * A


def test_total_correlation_through_the_class():
    M, B, Z = 3, 200, 6
    q = F.tc_inputs((M, B, Z, "minus90", 1))
    model = _model("mvtCAE", M, Z)
    for arg in (torch.from_numpy(q), [torch.from_numpy(q[m]).double() for m in range(M)], torch.from_numpy(q).to(DEV)):
        tc = model.total_correlation(arg, None)
        assert tc.dim() == 0 and np.float32(tc.item()).view(np.uint32) == _tc(q).view(np.uint32)
