"""The isolated-step Adam checker (tests/adam_check.py) on the CPU: the reference alone passes it, it is anchored to
torch.optim.Adam, and it flags every seeded fault.

  * emulate_f32 -- the kernel's fp32 arithmetic in numpy, sqrt and rcp pushed one ulp in a random direction -- stays inside
    the bounds for t in {1, 2, 10, 1000, 100000}, lr in {5e-6, 1e-4, 1e-3}, gradient scales 1e-3 .. 1e3 with exact zeros
    and 1e-6-scaled entries mixed in.  Peak error / bound over that grid: 0.51 (m'), 0.63 (v'), 0.51 (p'), printed by
    the test.
  * adam_ref equals torch.optim.Adam on fp64 tensors over 5 steps to 1e-14 relative.
  * Seven faults seeded into the emulation fail the checker at t in {1, 3, 50, 1000}.
  * At t = 20000 both bias corrections round to 1 in fp32 (0.9^t = 0, 0.999^t = 2e-9): "no bias correction" and "step off by
    one" give bit-identical results to the right kernel there and no one-step check can see them
    (test_late_step_bias_faults_are_invisible pins that fact) -- which is why the late-step GPU case uses t ~ 1000.
"""
import numpy as np
import pytest
import torch

from tests import adam_check as A

N = 4096           # 16 tiles of 256 elements
BETAS, EPS = (0.9, 0.999), 1e-8


def draw(seed, t, scale, n=N):
    """p, m, v, g (fp32): gradients of the given scale, 10 % exact zeros, 10 % scaled by 1e-6; moments of a plausible size
    (zero at t = 1; zero too under half of the zero gradients: untouched elements)."""
    rng = np.random.default_rng(seed)
    F = np.float32
    g = (rng.standard_normal(n) * scale).astype(F)
    zero = rng.random(n) < 0.1
    g[zero] = 0
    g[rng.random(n) < 0.1] *= F(1e-6)
    p = (rng.standard_normal(n) * 0.1).astype(F)
    if t == 1:
        m, v = np.zeros(n, F), np.zeros(n, F)
    else:
        m = (0.3 * scale * rng.standard_normal(n)).astype(F)
        v = ((scale * rng.standard_normal(n)) ** 2 * rng.uniform(0.05, 1.0, n)).astype(F)
        idle = zero & (rng.random(n) < 0.5)
        m[idle] = 0
        v[idle] = 0
    return p, m, v, g


def T(*arrs):
    return tuple(torch.from_numpy(np.ascontiguousarray(a)) for a in arrs)


def check(before, g, after, t, lr):
    return A.assert_adam_step(T(*before), T(g)[0], T(*after), t, lr, BETAS, EPS, what="emulation")


def test_emulation_stays_inside_the_bounds():
    worst = {"m": 0.0, "v": 0.0, "p": 0.0}
    seed = 0
    for t in (1, 2, 10, 1000, 100000):
        for lr in (5e-6, 1e-4, 1e-3):
            for scale in (1e-3, 1e-2, 1e-1, 1.0, 1e1, 1e2, 1e3):
                seed += 1
                p, m, v, g = draw(seed, t, scale)
                after = A.emulate_f32(p, m, v, g, t, lr, BETAS, EPS, rng=np.random.default_rng(10_000 + seed))
                r = check((p, m, v), g, after, t, lr)
                assert r["idle"] > 0 and r["moved"] > 0
                for k in worst:
                    worst[k] = max(worst[k], r[k])
    print(f"[adam check] emulation: worst error / bound  m' {worst['m']:.3f}  v' {worst['v']:.3f}  p' {worst['p']:.3f}")
    assert all(w <= 1.0 for w in worst.values())


def test_extreme_gradients_pass():
    """Exact zeros, 1e-30 (g * g flushes to zero) and 1e15 entries, as the flat-kernel GPU case uses them."""
    for t in (1, 2, 1000):
        p, m, v, g = draw(77 + t, t, 1.0)
        g[::7] = 0
        g[1::7] = 1e-30
        g[2::7] = 1e15
        after = A.emulate_f32(p, m, v, g, t, 1e-4, BETAS, EPS, rng=np.random.default_rng(t))
        check((p, m, v), g, after, t, 1e-4)


def test_restatement_equals_torch_adam_fp64():
    """adam_ref against torch.optim.Adam on fp64 tensors, 5 steps (hyper-parameters fp32-representable, as the descriptor
    carries them; lr any double)."""
    rng = np.random.default_rng(3)
    lr, betas, eps = 1e-4, (A.f32(0.9), A.f32(0.999)), A.f32(1e-8)
    w = torch.nn.Parameter(torch.from_numpy(rng.standard_normal(1000) * 0.1))
    opt = torch.optim.Adam([w], lr=lr, betas=betas, eps=eps)
    p, m, v = w.detach().numpy().copy(), np.zeros(1000), np.zeros(1000)
    for t in range(1, 6):
        g = rng.standard_normal(1000) * 10.0 ** rng.integers(-3, 3, 1000)
        w.grad = torch.from_numpy(g.copy())
        opt.step()
        p, m, v, _ = A.adam_ref(p, m, v, g, t, lr, betas, eps)
        st = opt.state[w]
        for name, a, r in (("p", p, w.detach().numpy()), ("m", m, st["exp_avg"].numpy()), ("v", v, st["exp_avg_sq"].numpy())):
            rel = np.abs(a - r).max() / np.abs(r).max()
            assert rel <= 1e-14, (name, t, rel)
            assert np.abs(a - r).max() <= 1e-14 * np.abs(r).max() and np.all(np.abs(a - r) <= 1e-13 * np.abs(r) + 1e-300), (name, t)


def _pick(g, lo=256, hi=N - 512):
    """An index in the interior whose gradient -- and the lane group one tile further -- is of ordinary size."""
    for i in range(lo, hi, 4):
        if np.all(np.abs(g[i:i + 4]) > 1e-4 * np.abs(g).max()) and np.all(np.abs(g[i + 256:i + 260]) > 1e-4 * np.abs(g).max()):
            return i
    raise AssertionError("no ordinary lane group")


def faulty(fault, p, m, v, g, t, lr):
    rng = np.random.default_rng(99)
    good = A.emulate_f32(p, m, v, g, t, lr, BETAS, EPS, rng=rng)
    if fault == "beta2 = 0.99":
        return A.emulate_f32(p, m, v, g, t, lr, (0.9, 0.99), EPS, rng=rng)
    if fault == "no bias correction":
        return A.emulate_f32(p, m, v, g, t, lr, BETAS, EPS, rng=rng, bias_correction=False)
    if fault == "eps inside the square root":
        return A.emulate_f32(p, m, v, g, t, lr, BETAS, EPS, rng=rng, eps_inside_sqrt=True)
    if fault == "optimizer step off by one":
        return A.emulate_f32(p, m, v, g, t + 1, lr, BETAS, EPS, rng=rng)
    i = _pick(g)
    out = [a.copy() for a in good]
    if fault == "one element skipped":
        for a, b in zip(out, (p, m, v)):
            a[i] = b[i]
    elif fault == "one element applied twice":
        twice = A.emulate_f32(*(a[i:i + 1] for a in good), g[i:i + 1], t, lr, BETAS, EPS)
        for a, b in zip(out, twice):
            a[i] = b[0]
    elif fault == "lane group from the neighbouring tile":
        other = A.emulate_f32(p[i:i + 4], m[i:i + 4], v[i:i + 4], g[i + 256:i + 260], t, lr, BETAS, EPS)
        for a, b in zip(out, other):
            a[i:i + 4] = b
    else:
        raise ValueError(fault)
    return tuple(out)


FAULTS = ["beta2 = 0.99", "no bias correction", "eps inside the square root", "optimizer step off by one",
          "one element skipped", "one element applied twice", "lane group from the neighbouring tile"]


@pytest.mark.parametrize("t", [1, 3, 50, 1000])
@pytest.mark.parametrize("fault", FAULTS)
def test_seeded_fault_is_flagged(fault, t):
    for lr, scale in ((1e-4, 1e-2), (1e-3, 1.0)):
        p, m, v, g = draw(500 + t, t, scale)
        check((p, m, v), g, A.emulate_f32(p, m, v, g, t, lr, BETAS, EPS, rng=np.random.default_rng(99)), t, lr)   # the right one passes
        with pytest.raises(AssertionError, match="flat index"):
            check((p, m, v), g, faulty(fault, p, m, v, g, t, lr), t, lr)


def test_late_step_bias_faults_are_invisible():
    """t = 20000: the kernel without bias correction, or one step off, computes the same bits as the right one."""
    t, lr = 20000, 1e-4
    p, m, v, g = draw(9, t, 1.0)
    good = A.emulate_f32(p, m, v, g, t, lr, BETAS, EPS)
    for bad in (A.emulate_f32(p, m, v, g, t, lr, BETAS, EPS, bias_correction=False), A.emulate_f32(p, m, v, g, t + 1, lr, BETAS, EPS)):
        assert all(np.array_equal(a, b) for a, b in zip(good, bad))


def test_failure_names_the_tensor_and_the_pad():
    """With a layout the report names tensor, tile, lane group and (row, column) -- or says "pad"."""
    import multi_modal_normative_modeling_amd as nm
    lay = nm.ParamLayout(nm.ModelSpec([37, 21], [24, 16], 6, 5))
    mask = A.tensor_mask(lay).numpy()
    n = lay.total
    rng = np.random.default_rng(1)
    F = np.float32
    p = (rng.standard_normal(n) * 0.1).astype(F) * mask
    g = rng.standard_normal(n).astype(F) * mask
    m, v = np.zeros(n, F), np.zeros(n, F)
    good = A.emulate_f32(p, m, v, g, 1, 1e-4, BETAS, EPS)
    r = A.assert_adam_step(T(p, m, v), T(g)[0], T(*good), 1, 1e-4, BETAS, EPS, layout=lay)
    assert r["idle"] == int((~mask).sum()) > 0
    name = "encoder_list.1.encoder_layers.0.weight"                  # [24][27]: rows 24..31 and columns 27..31 are padding
    o = lay.offsets[name]
    hit = o + 1 * 256 + 3 * 16 + 5                                     # tile (0, 1), row 3, column 21
    pad = o + 1 * 256 + 3 * 16 + 12                                    # tile (0, 1), row 3, column 28: beyond K = 27
    assert mask[hit] and not mask[pad]
    for idx, expect in ((hit, r"encoder_layers\.0\.weight tile \(0, 1\) lane group 13: \(row 3, column 21\)"), (pad, "pad")):
        bad = [a.copy() for a in good]
        bad[0][idx] += F(1e-3)
        with pytest.raises(AssertionError, match=f"flat index {idx} = .*{expect}"):
            A.assert_adam_step(T(p, m, v), T(g)[0], T(*bad), 1, 1e-4, BETAS, EPS, layout=lay)
    assert A.locate(lay, lay.offsets["alpha_m_list.0"]) == "alpha_m_list.0: element 0 of 1"
    assert "pad" in A.locate(lay, lay.offsets["alpha_m_list.0"] + 1)
