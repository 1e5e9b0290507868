"""One fused Adam step against the gradient it consumed, element by element (a helper, not a conftest).

The step kernels store the gradient they feed to Adam (NM_F_GRADS) at the same flat index as the parameter and its two
moments, and every launch is deterministic.  So for ONE optimizer step the test holds p, m, v before, g from a gradient
launch at that state, and p', m', v' after the training launch: the relation between them is fp32 Adam on known inputs,
with none of the bf16-operand noise that sizes the bounds of the trajectory tests.  `assert_adam_step` checks that
relation on EVERY element of the flat buffers, tile padding and alignment gaps included.

The arithmetic checked (adam1 / adam_bias_consts in csrc/nm_core.inc; torch.optim.Adam as configured at cVAE.py:1111-1116):

    m' = m + (g - m) (1 - b1)
    v' = v b2 + (1 - b2) g g
    p' = p - step_size * m' / (sqrt(v') * inv_bc2_sqrt + eps)
    step_size = lr / (1 - b1^t),   inv_bc2_sqrt = 1 / sqrt(1 - b2^t)        (double, from a double lr)

`adam_ref` restates it in fp64.  The descriptor carries beta1, beta2 and eps as fp32 (nm_job_t, nm_adam_step), so the
restatement rounds those three to fp32 first -- (1 - b) is then exact in fp32 as well as in fp64 -- and does everything
else in double; with fp32-representable hyper-parameters it equals torch.optim.Adam on fp64 tensors to 1e-14
(tests/test_adam_check_cpu.py).  lr is taken as the double the caller configured: the descriptor's fp32 copy of a
constant rate is off by at most 1 eps relative, which the p' bound below has room for.

Bounds, with eps = 2^-24 (the unit roundoff of fp32: half an ulp, relative):

  m'  |m'_k - m'_ref| <= 2 eps (|m| + |g|).  Kernel roundings: the subtraction, the product with (1 - b1), the final
      sum, each <= 1 eps of a quantity <= |m| + |g|; an fma contraction removes one of them.  Emulation peak: 1.0 eps (0.51 of the bound).
  v'  |v'_k - v'_ref| <= 4 eps v'_ref + 2^-126.  Four roundings (v b2, (1 - b2) g, that times g, the sum) of non-negative
      terms that add up to v'; the absolute term allows one flush of a denormal product to zero.  Emulation peak: 2.5 eps (0.63 of the bound).
  p'  |p'_k - p'_ref| <= 2 eps |p'_ref| + 12 eps |u|, with u = step_size * m'_k / (sqrt(v'_k) * inv_bc2_sqrt + eps)
      computed in fp64 FROM THE KERNEL'S OWN m'_k, v'_k -- so an error in a moment is reported once, by its own check, and
      the three checks stay independent.  Roundings of u: the v_sqrt_f32 and v_rcp_f32 builtins 1 ulp = 2 eps each, three
      products and one sum 1/2 ulp = 1 eps each at most, the fp32 copies of step_size and inv_bc2_sqrt (and of a constant
      lr) up to 1 eps each; they do not all peak together -- the emulation (sqrt and rcp pushed one ulp in a random
      direction) peaks at 0.51 of the whole bound.  The final subtraction rounds to 1/2 ulp of p': 1 eps |p'_ref|, bounded with 2.

  Where g == 0 and m == v == 0 (tile padding, alignment gaps, alpha under a combiner that ignores it), p', m', v' must
  equal p, 0, 0 BIT FOR BIT: nothing may leak into an element whose gradient is exactly zero.

No percentile, no skip list, no "tensor too small" exemption.  `frozen` is not such an exemption: it marks elements of
the flat buffer that are not optimizer parameters at all (BatchNorm running statistics of the end-to-end classifier live
in `params`; BatchNorm's momentum update moves them, Adam must not): there g, m, v, m', v' must all be zero bit for bit.

Late steps.  At t ~ 20000 both bias corrections are 1 to fp32 accuracy (0.999^20000 = 2e-9), so a kernel without bias
correction, or with t off by one, computes the same fp32 numbers as the right one: those two faults are invisible to ANY
one-step check there (seen on the CPU: the seeded faults pass the checker at t = 20000).  The late-step GPU case therefore
runs at t ~ 1000, where 1 - 0.999^t = 0.632 and moves by 3e-4 relative per step.

`emulate_f32` is the kernel's fp32 arithmetic in numpy (sqrt and rcp optionally pushed one ulp in a random direction,
as the hardware builtins may); tests/test_adam_check_cpu.py keeps it inside the bounds and seeds faults into it.
"""
from __future__ import annotations

import math
from typing import Dict, Optional, Sequence, Tuple

import numpy as np
import torch

EPS32 = 2.0 ** -24
TINY = 2.0 ** -126
TILE = 16


def f32(x: float) -> float:
    """x rounded to fp32, as a Python float (how the descriptor carries beta1, beta2, adam_eps)."""
    return float(np.float32(x))


def adam_bias_consts(t: int, lr: float, betas: Sequence[float]) -> Tuple[float, float]:
    """(step_size, inv_bc2_sqrt) of optimizer step t (1-based) in double, as torch.optim.Adam computes them."""
    b1, b2 = f32(betas[0]), f32(betas[1])
    return float(lr) / (1.0 - b1 ** float(t)), 1.0 / math.sqrt(1.0 - b2 ** float(t))


def adam_ref(p, m, v, g, t: int, lr: float, betas=(0.9, 0.999), eps: float = 1e-8):
    """One Adam step in fp64 numpy: (p', m', v', u)."""
    p, m, v, g = (np.asarray(a, dtype=np.float64) for a in (p, m, v, g))
    b1, b2, e = f32(betas[0]), f32(betas[1]), f32(eps)
    step_size, inv_bc2_sqrt = adam_bias_consts(t, lr, betas)
    m1 = m + (g - m) * (1.0 - b1)
    v1 = v * b2 + (1.0 - b2) * g * g
    u = step_size * m1 / (np.sqrt(v1) * inv_bc2_sqrt + e)
    return p - u, m1, v1, u


def _ulp_push(x: np.ndarray, rng) -> np.ndarray:
    """Every element one fp32 ulp up or down, at random."""
    up = rng.integers(0, 2, size=x.shape).astype(bool)
    return np.where(up, np.nextafter(x, np.float32(np.inf)), np.nextafter(x, np.float32(-np.inf))).astype(np.float32)


def emulate_f32(p, m, v, g, t: int, lr: float, betas=(0.9, 0.999), eps: float = 1e-8, rng=None, bias_correction=True,
                eps_inside_sqrt=False):
    """adam1 of csrc/nm_core.inc in fp32 numpy: (p', m', v').  rng: push sqrt and rcp one ulp in a random direction (the
    builtins are 1-ulp instructions).  bias_correction / eps_inside_sqrt: seeded faults."""
    F = np.float32
    p, m, v, g = (np.asarray(a, dtype=F) for a in (p, m, v, g))
    b1, b2, e = F(betas[0]), F(betas[1]), F(eps)
    step_size, inv_bc2_sqrt = adam_bias_consts(t, lr, (float(b1), float(b2))) if bias_correction else (float(lr), 1.0)
    step_size, inv_bc2_sqrt = F(step_size), F(inv_bc2_sqrt)
    with np.errstate(all="ignore"):
        m1 = (m + (g - m) * (F(1) - b1)).astype(F)
        v1 = (v * b2 + (F(1) - b2) * g * g).astype(F)
        if eps_inside_sqrt:
            s = np.sqrt((v1 + e).astype(F)).astype(F)
            if rng is not None:
                s = _ulp_push(s, rng)
            denom = (s * inv_bc2_sqrt).astype(F)
        else:
            s = np.sqrt(v1).astype(F)
            if rng is not None:
                s = np.maximum(_ulp_push(s, rng), F(0)) * (v1 > 0)
            denom = (s.astype(F) * inv_bc2_sqrt + e).astype(F)
        r = (F(1) / denom).astype(F)
        if rng is not None:
            r = _ulp_push(r, rng)
        p1 = (p - step_size * (m1 * r)).astype(F)
    return p1, m1, v1


def locate(layout, idx: int) -> str:
    """Where flat index idx of the kernel buffer lies: tensor name and (row, column) / element, or "pad"."""
    for name in layout.names:
        o = layout.offsets[name]
        if name in layout.tiles:
            nt, kt = layout.tiles[name]
            if not (o <= idx < o + nt * kt * TILE * TILE):
                continue
            local = idx - o
            tile, r, c = local // (TILE * TILE), (local % (TILE * TILE)) // TILE, local % TILE
            row, col = (tile // kt) * TILE + r, (tile % kt) * TILE + c
            where = f"{name} tile ({tile // kt}, {tile % kt}) lane group {(local % (TILE * TILE)) // 4}"
            n, k = layout.shapes[name]
            if name in layout.colmap:
                hit = (layout.colmap[name] == col).nonzero().flatten()
                if row >= n or hit.numel() == 0:
                    return f"{where}: pad (kernel row {row}, column {col})"
                return f"{where}: (row {row}, column {int(hit[0])})"
            if row >= n or col >= k:
                return f"{where}: pad (row {row}, column {col} of {n} x {k})"
            return f"{where}: (row {row}, column {col})"
        n = math.prod(layout.shapes[name])
        if o <= idx < o + n:
            return f"{name}: element {idx - o} of {n}"
        if o + n <= idx < o + (n + 3) // 4 * 4:
            return f"{name}: pad (alignment gap behind element {n - 1})"
    return "pad (belongs to no tensor)"


def tensor_mask(layout) -> torch.Tensor:
    """True where an element of the kernel buffer belongs to a tensor (ParamLayout.flatten of all-ones tensors)."""
    ones = {n: torch.ones(layout.shapes[n]) for n in layout.names}
    return layout.flatten(ones) != 0


def _np(t) -> np.ndarray:
    a = t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)
    assert a.dtype == np.float32 and a.ndim == 1, (a.dtype, a.shape)
    return a


def _bits(a: np.ndarray) -> np.ndarray:
    return a.view(np.int32)


def assert_adam_step(before, g, after, t: int, lr: float, betas=(0.9, 0.999), eps: float = 1e-8, layout=None,
                     frozen=None, what: str = "") -> Dict[str, float]:
    """before = (p, m, v), after = (p', m', v'), g: flat fp32 CPU tensors of one length.  Asserts the bounds of the module
    docstring on every element; returns the worst error / bound ratio of each of the three checks."""
    p, m, v = (_np(a) for a in before)
    p1, m1, v1 = (_np(a) for a in after)
    g = _np(g)
    n = p.size
    assert all(a.size == n for a in (m, v, g, p1, m1, v1)), "buffers differ in length"

    def fail(kind, bad, detail):
        i = int(np.flatnonzero(bad)[0])
        where = f" = {locate(layout, i)}" if layout is not None else ""
        raise AssertionError(
            f"{what}: {kind} at flat index {i}{where} ({int(bad.sum())} of {n} elements fail; t = {t}, lr = {lr!r})\n"
            f"  p {p[i]!r} m {m[i]!r} v {v[i]!r} g {g[i]!r}\n  p' {p1[i]!r} m' {m1[i]!r} v' {v1[i]!r}\n  {detail(i)}")

    for name, a in (("p", p), ("m", m), ("v", v), ("g", g), ("p'", p1), ("m'", m1), ("v'", v1)):
        bad = ~np.isfinite(a)
        if bad.any():
            fail(f"non-finite {name}", bad, lambda i: "")
    fr = np.zeros(n, dtype=bool) if frozen is None else np.asarray(frozen, dtype=bool)
    if fr.any():            # not optimizer parameters: no gradient, no moments, before or after
        bad = fr & ((g != 0) |(_bits(m) != 0) | (_bits(v) != 0) | (_bits(m1) != 0) | (_bits(v1) != 0))
        if bad.any():
            fail("a non-parameter element (BatchNorm running statistic) has a gradient or a moment", bad, lambda i: "")
    live = ~fr
    p_ref, m_ref, v_ref, _ = adam_ref(p, m, v, g, t, lr, betas, eps)
    pd, md, vd, gd = (a.astype(np.float64) for a in (p, m, v, g))
    # m'
    err_m, bnd_m = np.abs(m1 - m_ref), 2 * EPS32 * (np.abs(md) + np.abs(gd))
    bad = live & (err_m > bnd_m)
    if bad.any():
        fail("exp_avg", bad, lambda i: f"m'_ref {m_ref[i]!r}: error {err_m[i]:.3e} > bound {bnd_m[i]:.3e}")
    # v'
    err_v, bnd_v = np.abs(v1 - v_ref), 4 * EPS32 * v_ref + TINY
    bad = live & (err_v > bnd_v)
    if bad.any():
        fail("exp_avg_sq", bad, lambda i: f"v'_ref {v_ref[i]!r}: error {err_v[i]:.3e} > bound {bnd_v[i]:.3e}")
    bad = live & (v1 < 0)
    if bad.any():
        fail("negative exp_avg_sq", bad, lambda i: "")
    # p' from the kernel's own moments
    step_size, inv_bc2_sqrt = adam_bias_consts(t, lr, betas)
    u = step_size * m1.astype(np.float64) / (np.sqrt(v1.astype(np.float64)) * inv_bc2_sqrt + f32(eps))
    pr = pd - u
    err_p, bnd_p = np.abs(p1 - pr), 2 * EPS32 * np.abs(pr) + 12 * EPS32 * np.abs(u)
    bad = live & (err_p > bnd_p)
    if bad.any():
        fail("parameter", bad, lambda i: f"u {u[i]!r} p'_ref {pr[i]!r} (from fp64 moments {p_ref[i]!r}): "
                                         f"error {err_p[i]:.3e} > bound {bnd_p[i]:.3e}")
    # untouched elements: bit for bit
    idle = live & (g == 0) & (m == 0) & (v == 0)
    bad = idle & ((_bits(p1) != _bits(p)) | (_bits(m1) != 0) | (_bits(v1) != 0))
    if bad.any():
        fail("an element with g == m == v == 0 changed", bad, lambda i: "must be p, 0, 0 bit for bit")

    def worst(err, bnd):
        ok = live & (bnd > 0)
        return float((err[ok] / bnd[ok]).max()) if ok.any() else 0.0

    return {"m": worst(err_m, bnd_m), "v": worst(err_v, bnd_v), "p": worst(err_p, bnd_p),
            "moved": int((live & (_bits(p1) != _bits(p))).sum()), "idle": int(idle.sum()), "n": n}
