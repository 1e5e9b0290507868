"""The gradient of one launch against the oracle, element by element (a helper, not a conftest).

Every training launch of the project is tied, bit for bit or to a few ulp, to one of two root kernels: the fused step
kernel (nm_launch, csrc/nm_core.inc) and the general-shape path (nm_launch_wide, csrc/nm_wide.inc); tests/adam_check.py
ties every fused Adam update to the gradient it consumed.  The gradients of the two roots themselves were compared with
the oracle per tensor only (relative L2 4e-2, a cosine): a dropped row or column of a large weight gradient, a stale
activation block, a mishandled last partial tile all stay below that.  This module holds what closes the gap.

The noise floor.  The oracle (oracle/cvae_ref.py with bf16 GEMM operands) and a kernel compute the same arithmetic in
different fp32 summation orders.  How far two correct implementations may lie apart is measured with a TWIN of the oracle:
the same network with the hidden units of every layer permuted (rows of that layer's weight and bias, columns of the next
layer or of the mean / logvar / output heads), gradients permuted back.  With LeakyReLU on, a pre-activation that changes
sign moves single elements by several percent of a tensor's maximum; with non_linear=False the twin stays within about
1e-3 of the maximum, while the median element of a dropped row or column is about a tenth of it.  Linear stacks run through
the same GEMM loops, block tables, epilogues and gradient stores as non-linear ones, so:

  Statistic A (assert_every_element), linear stacks: per tensor max |got - want| <= bound_A * max |want|; every element
      finite; a tensor whose oracle gradient is identically zero is exactly zero if the kernel writes it and still
      NaN-poisoned if it does not.  No percentile, no skip list, no exemption for small tensors.
  Statistic B (assert_every_slice), LeakyReLU on: for every row and every column of a matrix, and every 16-element piece of
      a vector, ||got - want|| <= bound_B * max(||want||, SLICE_FLOOR * the tensor's largest slice norm of that kind), SLICE_FLOOR = 0.3.
      Single elements flip there, and a flip moves the unit's whole ROW of the weight gradient too, by the one term of
      the batch sum that flipped (about 1 / sqrt(B) of the row), which a bound from a twin that flips no unit has no room
      for.  So a row of a hidden layer's weight gradient that is beyond the bound, and within it once ONE term of its
      batch sum is taken out, names a flipped unit -- one whose pre-activation lies inside its margin of zero (flip_model:
      0.3 % of the pre-activations), for at most 1 % of a tensor's rows; the oracle is run again with exactly those units
      on LeakyReLU's other branch and every row, column and piece is held to that run at the same bound
      (assert_every_slice_of_case).  (The one-element tensors alpha_m_list.m count as one vector.)  The
      floor keeps a slice whose own gradient is tiny (the column of
      a covariate that is hot in two rows of the batch) from setting the bound of all the others; a slice above the floor
      is held relative to itself.

What statistic A does not pin: the derivative of LeakyReLU per element.  Statistic B, run_case's bounds and the golden
comparisons cover that.

Bounds.  Each case carries bound_A and bound_B as constants, a multiple of the worst oracle-to-twin distance in that
statistic over the case's tensors.  The factor covers what the twin cannot imitate: the MFMA accumulation order, the
128-column block order, a last-ulp difference in expf.  tests/test_grad_check_cpu.py recomputes the twin distance and
holds every constant between 4 x and 8 x of it, so a bound cannot be loosened unnoticed; the constants are written at
5.7 x (the geometric middle of that window, two digits), so that a BLAS that blocks its sums differently does not push a
recomputed distance out of the window.  A GPU result beyond a bound is a finding to explain from the failing tensor and
slice index, not a reason to widen the factor.

Floors.  A model with one hidden layer gives the twin almost nothing to reorder (its first-layer sums do not change at
all): the distance comes out near 1e-7, where a kernel, whose MFMA sums do differ, sees bf16 roundings of activations
fall the other way.  bound_A is therefore never below FLOOR_A = 2e-3, the element-wise bound tests/test_gpu_parity.py
uses for short contractions (about one bf16 rounding unit, 2^-9).  bound_B is never below FLOOR_B = 4 x FLOOR_A: the
largest of 1e3 .. 1e7 Gaussian-like entries is 3.3 .. 5.3 times their RMS, so an error of FLOOR_A x max |want| in every
element of a slice of ordinary norm is a relative L2 error of about 4 x FLOOR_A of that slice -- below that, statistic B
would ask more of a kernel than statistic A's floor does.  A bound sits at its floor only where 4 x the twin distance is
below it.

`seeded_faults` yields the structural faults a kernel could have (a dropped row / column, swapped 16 x 16 tiles, a stale
128 x 128 block, a repeated bias element, a 2 % scale error, a pad row that leaks); test_grad_check_cpu.py seeds each into
the oracle's own gradients and requires the checker to flag it.
"""
from __future__ import annotations

import functools
from dataclasses import dataclass
from typing import Dict, Iterator, List, Optional, Tuple

import torch

import multi_modal_normative_modeling_amd as nm
from oracle import cvae_ref as R

FLOOR_A = 2e-3          # tests/test_gpu_parity.py: element-wise bound of short contractions
FLOOR_B = 8e-3          # statistic B's floor: 4 x FLOOR_A (see "Bounds" above)
SLICE_FLOOR = 0.3       # statistic B: a slice is held relative to at least this fraction of the tensor's largest slice norm
PIECE = 16              # statistic B on vectors: 16-element pieces
FACTOR_LO, FACTOR_HI = 4.0, 8.0


@dataclass(frozen=True)
class GradCase:
    id: str
    dims: Tuple[int, ...]
    hidden: Tuple[int, ...]
    Z: int
    c_dim: int
    B: int
    combine: str
    kind: str            # "multimodal" | "mvtcae"
    wide: bool           # which root kernel must serve it
    seed: int
    bound_A: float       # linear stack, statistic A
    bound_B: float       # LeakyReLU, statistic B


def _c(id, dims, hidden, Z, c_dim, B, combine, wide, seed, bound_A, bound_B, kind="multimodal"):
    return GradCase(id, tuple(dims), tuple(hidden), Z, c_dim, B, combine, kind, wide, seed, bound_A, bound_B)


# bound_A / bound_B: 5.7 x the oracle-to-twin distance or the floor (see the module docstring); the distances are
# recomputed by tests/test_grad_check_cpu.py::test_bounds_are_tied_to_the_twin
CASES: Dict[str, GradCase] = {c.id: c for c in [
    # -- general-shape path --------------------------------------------------------------------------------------------
    _c("W1", [37], (4096,), 128, 29, 256, "poe", True, 101, 2e-3, 8e-3),
    _c("W2", [37], (4096, 4096), 16, 5, 256, "poe", True, 102, 7.0e-3, 0.29),
    _c("W3", [70, 55, 33], (129, 128, 257), 65, 6, 255, "mopoe", True, 103, 1.1e-2, 1.3e-2),
    _c("W4", [50, 41], (136, 40, 129, 16, 128, 8, 200, 24), 100, 29, 19, "gpoe", True, 104, 1.2e-2, 1.6e-2),
    _c("W5", [379, 379, 379, 1137], (300, 300), 30, 29, 256, "gpoe", True, 105, 5.9e-3, 1.2e-2),
    _c("W6", [60], (100,), 64, 64, 83, "poe", True, 106, 2e-3, 8e-3),
    _c("W7", [45, 61], (200,), 72, 5, 1, "moe", True, 107, 2e-3, 8e-3),
    _c("W8", [40, 40, 40, 40], (130,), 64, 5, 200, "poe", True, 108, 2e-3, 8e-3, kind="mvtcae"),
    _c("W9", [40, 33], (130,), 128, 5, 200, "gpoe", True, 109, 2e-3, 8e-3, kind="mvtcae"),
    # -- fused step kernel ---------------------------------------------------------------------------------------------
    _c("F1", [77], (127,), 64, 29, 130, "poe", False, 201, 2e-3, 8e-3),
    _c("F2", [1137], (110, 110), 10, 29, 256, "poe", False, 202, 5.5e-3, 8e-3),
    _c("F3", [379, 379, 379, 1137], (110, 110), 10, 29, 256, "gpoe", False, 203, 3.9e-3, 9.9e-3),
    _c("F4", [129], (16, 127, 8), 5, 3, 255, "gpoe", False, 204, 2e-3, 8e-3),
    _c("F5", [60], (100,), 64, 63, 83, "poe", False, 205, 4.1e-3, 8e-3),
    _c("F6", [50, 41], (90, 40, 127, 16, 64, 8, 100, 24), 20, 29, 19, "mopoe", False, 206, 2e-3, 8e-3),
]}
WIDE_IDS = [k for k, c in CASES.items() if c.wide]
FUSED_IDS = [k for k, c in CASES.items() if not c.wide]


def onehot(gen, B, c_dim):
    """Two hot columns per row: one of the first c_dim - 2, one of the last two (the site / sex pattern of the data)."""
    c = torch.zeros(B, c_dim)
    c[torch.arange(B), torch.randint(0, c_dim - 2, (B,), generator=gen)] = 1
    c[torch.arange(B), c_dim - 2 + torch.randint(0, 2, (B,), generator=gen)] = 1
    return c


class CaseData:
    """Seeded data of one case: B + 1 table rows (the last one is the pad row of the leak fault; every run but that one
    uses the first B), covariates, draws, reference-rule weights."""

    def __init__(self, case: GradCase):
        gen = torch.Generator().manual_seed(case.seed)
        self.case = case
        n = case.B + 1
        self.xs = [torch.randn(n, d, generator=gen) * 1.2 for d in case.dims]
        self.c = onehot(gen, n, case.c_dim)
        self.eps = torch.randn(n, case.Z, generator=gen)
        self.P = nm.ParamLayout(self.spec(True)).init_reference_rule(case.seed)

    def spec(self, non_linear: bool) -> "nm.ModelSpec":
        c = self.case
        return nm.ModelSpec(list(c.dims), list(c.hidden), c.Z, c.c_dim, non_linear, c.kind)

    def job(self, non_linear: bool, device):
        """The case as a Job on `device`, gradient buffer NaN-poisoned."""
        c = self.case
        tables = [nm.Table(x[:c.B], self.c[:c.B], device) for x in self.xs]
        job = nm.Job(self.spec(non_linear), tables, combine=c.combine, state=self.P)
        job.set_eps(self.eps[:c.B])
        job.grads.fill_(float("nan"))
        return job


@functools.lru_cache(maxsize=None)
def data(case_id: str) -> CaseData:
    return CaseData(CASES[case_id])


def _run(cd: CaseData, P, non_linear: bool, rows: int, mode: str, trace: Optional[dict] = None, force: Optional[dict] = None):
    """Loss dict and gradients of the oracle on the first `rows` rows, with `mode` operand rounding.  `trace`, if given,
    receives name -> (input, pre-activation with its gradient retained) of every hidden layer's linear map (each layer
    runs once per forward pass).  `force`: name -> [(batch row, unit), ...] whose pre-activation is mirrored at zero (a
    constant is added, the gradient passes unchanged), so that LeakyReLU takes its other branch there."""
    c = cd.case
    rs = R.Spec(list(c.dims), list(c.hidden), c.Z, c.c_dim, non_linear)
    xs, cov, eps = [x[:rows] for x in cd.xs], cd.c[:rows].long(), cd.eps[:rows]
    fwd_fn, loss_fn = (R.mvt_forward, R.mvt_loss) if c.kind == "mvtcae" else (R.forward_multimodal, R.loss_multimodal)
    R.set_operand_rounding(mode)
    try:
        leaves = {k: v.clone().requires_grad_(True) for k, v in P.items()}
        if trace is not None or force:
            trace, force = ({} if trace is None else trace), (force or {})
            hidden_of = {id(leaves[w]): w for ws, _, _ in _chains(c) for w in ws}

            def hook(a, W, y):
                name = hidden_of.get(id(W))
                if name is None:
                    return y
                assert name not in trace, (name, "runs twice in one forward pass")
                if name in force:
                    shift = torch.zeros_like(y)
                    for b_, j_ in force[name]:
                        shift[b_, j_] = -2.0 * float(y.detach()[b_, j_])
                    y = y + shift
                y.retain_grad()
                trace[name] = (a.detach(), y)
                return y
            R.set_linear_hook(hook)
        fwd = fwd_fn(leaves, rs, xs, [cov] * len(xs), c.combine, eps)
        loss = loss_fn(rs, xs, fwd)
        loss["total"].sum().backward()
        grads = {k: (v.grad if v.grad is not None else torch.zeros_like(v)) for k, v in leaves.items()}
        return {k: float(torch.as_tensor(v).detach().sum()) for k, v in loss.items() if k != "ll_m"}, grads
    finally:
        R.set_linear_hook(None)
        R.set_operand_rounding("fp32")


@functools.lru_cache(maxsize=None)
def oracle_run(case_id: str, non_linear: bool, extra_row: bool = False):
    cd = data(case_id)
    return _run(cd, cd.P, non_linear, cd.case.B + (1 if extra_row else 0), "bf16")


def oracle_grads(case_id: str, non_linear: bool) -> Dict[str, torch.Tensor]:
    """Gradients of the bf16-operand oracle.  Cached: callers must not write into them."""
    return oracle_run(case_id, non_linear)[1]


@functools.lru_cache(maxsize=None)
def oracle_ll32(case_id: str, non_linear: bool) -> float:
    """Reconstruction log-likelihood (summed over the modalities) of the fp32 oracle: the reference of run_case's bound."""
    cd = data(case_id)
    c = cd.case
    rs = R.Spec(list(c.dims), list(c.hidden), c.Z, c.c_dim, non_linear)
    xs, cov = [x[:c.B] for x in cd.xs], cd.c[:c.B].long()
    with torch.no_grad():
        if c.kind == "mvtcae":
            fwd = R.mvt_forward(cd.P, rs, xs, [cov] * len(xs), c.combine, cd.eps[:c.B])
        else:
            fwd = R.forward_multimodal(cd.P, rs, xs, [cov] * len(xs), c.combine, cd.eps[:c.B])
        return float(sum(R.compute_ll(xs[m], fwd["locs"][m], fwd["scales"][m]) for m in range(len(xs))))


def clear_cache():
    """Drop the cached data and oracle runs (W2 holds two 4096 x 4096 gradients per run)."""
    for f in (data, oracle_run, oracle_ll32, twin_grads, flip_model):
        f.cache_clear()


# ---- the twin ---------------------------------------------------------------------------------------------------------------
def _chains(case: GradCase) -> List[Tuple[List[str], List[str], List[str]]]:
    """Per encoder and decoder: (hidden layers' weight names, their bias names, the weights whose COLUMNS follow the last
    hidden layer)."""
    L, out = len(case.hidden), []
    for m in range(len(case.dims)):
        e, d = f"encoder_list.{m}.", f"decoder_list.{m}."
        out.append(([f"{e}encoder_layers.{i}.weight" for i in range(L)], [f"{e}encoder_layers.{i}.bias" for i in range(L)],
                    [f"{e}enc_mean_layer.weight", f"{e}enc_logvar_layer.weight"]))
        out.append(([f"{d}decoder_layers.{i}.weight" for i in range(L)], [f"{d}decoder_layers.{i}.bias" for i in range(L)],
                    [f"{d}decoder_mean_layer.weight"]))
    return out


def twin_perms(case: GradCase, P) -> Dict[str, Tuple[Optional[torch.Tensor], Optional[torch.Tensor]]]:
    """name -> (row permutation, column permutation) of every tensor the twin permutes: every hidden layer of every encoder
    and decoder gets its own seeded permutation."""
    gen = torch.Generator().manual_seed(7919 * case.seed + 1)
    perms: Dict[str, Tuple[Optional[torch.Tensor], Optional[torch.Tensor]]] = {}
    for weights, biases, heads in _chains(case):
        prev = None
        for w, b in zip(weights, biases):
            p = torch.randperm(P[w].shape[0], generator=gen)
            perms[w], perms[b] = (p, prev), (p, None)
            prev = p
        for h in heads:
            perms[h] = (None, prev)
    return perms


def _permute(t, rows, cols):
    if rows is not None:
        t = t[rows]
    if cols is not None:
        t = t[:, cols]
    return t.contiguous()


def _inverse(p):
    if p is None:
        return None
    inv = torch.empty_like(p)
    inv[p] = torch.arange(p.numel())
    return inv


@functools.lru_cache(maxsize=None)
def twin_grads(case_id: str, non_linear: bool) -> Dict[str, torch.Tensor]:
    """The oracle's gradients computed by the permuted restatement of the same network, un-permuted: the same arithmetic in
    another fp32 summation order."""
    cd = data(case_id)
    perms = twin_perms(cd.case, cd.P)
    Pt = {k: (_permute(v, *perms[k]) if k in perms else v) for k, v in cd.P.items()}
    _, g = _run(cd, Pt, non_linear, cd.case.B, "bf16")
    return {k: (_permute(v, _inverse(perms[k][0]), _inverse(perms[k][1])) if k in perms else v) for k, v in g.items()}


# ---- the two statistics -----------------------------------------------------------------------------------------------------
def _where(name, t, flat_idx):
    if t.dim() == 2 and t.shape[0] > 1:
        r, c = divmod(int(flat_idx), t.shape[1])
        return (f"{name}[{r}, {c}] of {tuple(t.shape)} (row {r} = 128 * {r // 128} + 16 * {r % 128 // 16} + {r % 16}, "
                f"column {c} = 128 * {c // 128} + 16 * {c % 128 // 16} + {c % 16})")
    return f"{name}[{int(flat_idx)}] of {tuple(t.shape)}"


def _zero_rule(name, a, what):
    """The oracle's gradient is identically zero: untouched (all NaN) or written as exact zeros."""
    if bool(torch.isnan(a).all()):
        return
    bad = (a != 0) | torch.isnan(a)
    assert not bool(bad.any()), (f"{what}: {name}: the oracle's gradient is identically zero; the kernel must leave it "
                                 f"untouched or write exact zeros, got {int(bad.sum())} other elements, first "
                                 f"{_where(name, a, int(bad.flatten().nonzero()[0]))}")


def element_distance(got: Dict[str, torch.Tensor], want: Dict[str, torch.Tensor]) -> Dict[str, float]:
    """Statistic A per tensor: max |got - want| / max |want| (tensors with want == 0 left out)."""
    return {k: float((got[k] - w).abs().max()) / float(w.abs().max()) for k, w in want.items() if float(w.abs().max()) > 0}


def assert_every_element(got, want, bound: float, what: str = "") -> Dict[str, float]:
    """Statistic A on every tensor of `want`; returns error / bound per tensor."""
    out = {}
    for name, w in want.items():
        a = got[name]
        assert tuple(a.shape) == tuple(w.shape), (what, name, tuple(a.shape), tuple(w.shape))
        wmax = float(w.abs().max())
        if wmax == 0.0:
            _zero_rule(name, a, what)
            continue
        fin = torch.isfinite(a)
        assert bool(fin.all()), (f"{what}: {name}: {int((~fin).sum())} elements not finite (not written?), first "
                                 f"{_where(name, a, int((~fin).flatten().nonzero()[0]))}")
        err = (a - w).abs()
        worst = float(err.max())
        if worst > bound * wmax:
            i = int(err.argmax())
            raise AssertionError(
                f"{what}: {_where(name, a, i)}: got {float(a.flatten()[i])!r}, oracle {float(w.flatten()[i])!r}, |diff| "
                f"{worst:.3e} = {worst / wmax:.3e} of max |oracle| {wmax:.3e} > bound {bound:.1e}; "
                f"{int((err > bound * wmax).sum())} of {err.numel()} elements beyond it")
        out[name] = worst / wmax / bound
    return out


def _slices(name, t) -> Iterator[Tuple[str, torch.Tensor]]:
    """(kind, [n_slices, slice_len] view-like tensor) of a gradient tensor: rows and columns, or 16-element pieces."""
    if t.dim() == 2 and t.shape[0] > 1:
        yield "row", t
        yield "column", t.T
    else:
        v = t.flatten()
        pad = (-v.numel()) % PIECE
        if pad:
            v = torch.cat([v, v.new_zeros(pad)])
        yield "piece", v.view(-1, PIECE)


ALPHA = "alpha_m_list"


def _alpha_as_one_vector(d):
    """The M one-element tensors alpha_m_list.m as ONE vector (statistic B only).  They are the components of a single
    softmax argument, so their gradients sum to zero and any one of them may be the small remainder of a cancellation
    (W5: 3.6e-4 next to 0.86, and 9.9e-3 in the fp32 oracle): a relative error of such a scalar on its own measures nothing,
    as a piece of its vector it is held like every other element."""
    keys = sorted((k for k in d if k.startswith(ALPHA + ".")), key=lambda k: int(k.rsplit(".", 1)[1]))
    if not keys:
        return d
    out = {k: v for k, v in d.items() if k not in keys}
    out[ALPHA] = torch.cat([d[k].flatten() for k in keys])
    return out


def slice_distance(got, want) -> Dict[Tuple[str, str], Tuple[float, int]]:
    """Statistic B per (tensor, slice kind): the worst ||got - want|| / max(||want||, SLICE_FLOOR * largest ||want||) and
    the index of the slice that has it (tensors with want == 0 left out; the alphas as one vector)."""
    out = {}
    got, want = _alpha_as_one_vector(got), _alpha_as_one_vector(want)
    for name, w in want.items():
        if float(w.abs().max()) == 0.0:
            continue
        for (kind, ws), (_, gs) in zip(_slices(name, w), _slices(name, got[name])):
            wn = ws.double().norm(dim=1)
            den = torch.clamp(wn, min=SLICE_FLOOR * float(wn.max()))
            rel = (gs.double() - ws.double()).norm(dim=1) / den
            i = int(rel.argmax())
            out[(name, kind)] = (float(rel[i]), i)
    return out


def _take_out_flips(got, want, bound: float, flips: Dict[str, FlipModel], flipped: Optional[list]):
    """`got` with the admissible sign flips taken out: for every row of a hidden layer's weight gradient that is beyond
    the bound, the ONE candidate of that row's unit (FlipModel.row_candidates) that explains it best, if the row is within
    the bound once that flip's term is removed; the same flip is removed from the bias gradient's element."""
    out = dict(got)
    for name, fm in flips.items():
        w, bias = want[name].double(), name[:-6] + "bias"
        g, gb = got[name].double().clone(), got[bias].double().clone()
        wn = w.norm(dim=1)
        den = torch.clamp(wn, min=SLICE_FLOOR * float(wn.max()))
        rel = (g - w).norm(dim=1) / den
        allowed = max(1, int(MAX_FLIPPED_ROWS * len(rel)))
        for j in (rel > bound).nonzero().flatten().tolist():
            best = min(((float((g[j] - w[j] - dw).norm() / den[j]), b, dw, db) for b, dw, db in fm.row_candidates(j)),
                       key=lambda t: t[0], default=None)
            if best is None or best[0] > bound or allowed == 0:
                continue                                    # (stays as it is and fails statistic B below)
            allowed -= 1
            g[j] -= best[2]
            gb[j] -= best[3]
            if flipped is not None:
                flipped.append((name, j, best[1], float(fm.pre[best[1], j]), float(fm.margin[best[1], j]), float(rel[j]), best[0]))
        out[name], out[bias] = g.to(got[name].dtype), gb.to(got[bias].dtype)
    return out


def assert_every_slice(got, want, bound: float, what: str = "", flips: Optional[Dict[str, FlipModel]] = None,
                       flipped: Optional[list] = None) -> Dict[Tuple[str, str], float]:
    """Statistic B on every tensor of `want`; returns error / bound per (tensor, slice kind).

    `flips` (flip_model of the case): a ROW of a hidden layer's weight gradient that is beyond the bound is held instead
    against the oracle with ONE LeakyReLU unit of that row on the other side of zero -- a unit whose pre-activation lies
    inside its margin -- at the same bound; that flip's term is then taken out of the row and of the bias element, and every
    row, column and piece is checked as usual.  At most MAX_FLIPPED_ROWS of a tensor's rows (at least one) may pass that
    way; each is appended to `flipped` as (tensor, unit, batch row, pre-activation, margin, relative L2 before, after)."""
    for name, w in want.items():
        a = got[name]
        assert tuple(a.shape) == tuple(w.shape), (what, name, tuple(a.shape), tuple(w.shape))
        if float(w.abs().max()) == 0.0:
            _zero_rule(name, a, what)
            continue
        fin = torch.isfinite(a)
        assert bool(fin.all()), (f"{what}: {name}: {int((~fin).sum())} elements not finite (not written?), first "
                                 f"{_where(name, a, int((~fin).flatten().nonzero()[0]))}")
    if flips:
        got = _take_out_flips(got, want, bound, flips, flipped)
    out = {}
    for (name, kind), (rel, i) in slice_distance(got, want).items():
        if rel > bound:
            unit = PIECE if kind == "piece" else 1
            raise AssertionError(f"{what}: {name}: {kind} {i} (elements from {i * unit}; "
                                 f"= 128 * {i * unit // 128} + 16 * {i * unit % 128 // 16} + {i * unit % 16}): relative L2 "
                                 f"{rel:.3e} > bound {bound:.1e}")
        out[(name, kind)] = rel / bound
    return out


def assert_every_slice_of_case(case_id: str, got, what: str = "", flipped: Optional[list] = None):
    """Statistic B of a LeakyReLU run of the case at its bound_B, sign flips included: the rows that are beyond the bound
    and that one admissible flip explains (_take_out_flips) name the flipped units; the oracle is then run again with
    exactly those units on LeakyReLU's other branch -- which also moves, for that batch row, everything the unit's gradient
    flows back into -- and EVERY row, column and piece is held to that run at the same bound, with no further allowance."""
    bound, want = CASES[case_id].bound_B, oracle_grads(case_id, True)
    flipped = [] if flipped is None else flipped
    clean = {k: torch.nan_to_num(v) for k, v in got.items()}
    _take_out_flips(clean, want, bound, flip_model(case_id), flipped)
    if not flipped:
        return assert_every_slice(got, want, bound, what)
    force: dict = {}
    for name, j, b, *_ in flipped:
        force.setdefault(name, []).append((b, j))
    cd = data(case_id)
    _, want2 = _run(cd, cd.P, True, cd.case.B, "bf16", force=force)
    return assert_every_slice(got, want2, bound, what + f" ({len(flipped)} sign flips)")


def twin_distance(case_id: str) -> Tuple[float, float]:
    """(statistic A on the linear stack, statistic B with LeakyReLU) between the oracle and its twin: the worst over the
    case's tensors."""
    a = max(element_distance(twin_grads(case_id, False), oracle_grads(case_id, False)).values())
    b = max(v[0] for v in slice_distance(twin_grads(case_id, True), oracle_grads(case_id, True)).values())
    return a, b


# ---- LeakyReLU sign flips a correct implementation may make ------------------------------------------------------------------
MAX_FLIPPED_ROWS = 0.01    # of a tensor's rows (at least one) may be held against the oracle with one flip


@dataclass
class FlipModel:
    """Per hidden layer (keyed by its weight's name), over the batch rows b and the layer's units j: the pre-activation,
    the margin within which it may land on the other side of zero, dL/dh of the unit's output, the layer's bf16 input."""
    pre: torch.Tensor
    margin: torch.Tensor
    dh: torch.Tensor
    a: torch.Tensor

    def row_candidates(self, j: int) -> Iterator[Tuple[int, torch.Tensor, float]]:
        """(batch row b, change of row j of the weight gradient, change of element j of the bias gradient) for every
        pre-activation of unit j inside its margin: the derivative 0.01 becomes 1, or the reverse."""
        for b in (self.pre[:, j].abs() < self.margin[:, j]).nonzero().flatten().tolist():
            d = (1.0 - R.LEAKY_SLOPE) * float(self.dh[b, j]) * (1.0 if float(self.pre[b, j]) < 0 else -1.0)
            yield b, d * self.a[b], d


@functools.lru_cache(maxsize=None)
def flip_model(case_id: str) -> Dict[str, FlipModel]:
    """Which LeakyReLU units may change sides in a correct implementation, from the oracle alone.

    What the twin cannot imitate (see "Floors" in the module docstring): an activation whose bf16 rounding falls the
    other way.  The margin is a MODEL of that, not a measurement of the kernel: one such rounding in the latent z of a
    batch row changes every hidden activation after it by a fraction of
    a bf16 unit, so each input a[b, k] of a later sum may be off by about half a bf16 unit, at most 2^-8 |a[b, k]|, with
    independent signs: the pre-activation of unit j in row b then moves by about
        margin[b, j] = 2^-8 ||bf16(W[j, :]) * bf16(a[b, :])||_2 ,
    and a unit inside that margin of zero may take LeakyReLU's other branch.  Row j of the layer's weight gradient then
    moves by 0.99 dL/dh[b, j] a[b, :], one of the B terms of its batch sum -- about 1 / sqrt(B) of the row, which no bound
    derived from a twin that flips no unit has room for (W5: unit 279 of decoder 1's second layer, -9.2e-5 in row 87,
    margin 5.8e-4: the row moves by 8.6e-2, bound_B 1.2e-2)."""
    cd = data(case_id)
    trace: dict = {}
    _run(cd, cd.P, True, cd.case.B, "bf16", trace)
    out = {}
    for name, (a, y) in trace.items():
        W, a, pre = R._bf(cd.P[name]).double(), R._bf(a).double(), y.detach().double()
        dh = y.grad.double() / torch.where(pre >= 0, 1.0, R.LEAKY_SLOPE)
        out[name] = FlipModel(pre, 2.0 ** -8 * (a.square() @ W.square().T).sqrt(), dh, a)
    return out


# ---- seeded faults ----------------------------------------------------------------------------------------------------------
def _edge_indices(n: int) -> List[int]:
    return sorted({i for i in (0, 127, 128, n - 1) if 0 <= i < n})


def seeded_faults(case_id: str, non_linear: bool, structural_only: bool = False):
    """Yields (label, tensor name, faulty tensor, region) for every weight matrix of the case in turn; `region` is the
    part of the ORACLE's tensor the fault removes or moves (what a checker can see of it at best).

    One row / one column zeroed at 0, 127, 128 and last; a 16 x 16 tile swapped with its right neighbour; a 128 x 128
    block replaced by its neighbour block; bias element 128 replaced by element 127; the tensor scaled by 1.02; one extra
    table row leaking in (the oracle at B + 1 rows, rescaled to the mean over B, minus the oracle at B).
    structural_only: the zeroed rows and columns alone (what statistic B is for)."""
    cd = data(case_id)
    B = cd.case.B
    g = oracle_grads(case_id, non_linear)
    g1 = None if structural_only else oracle_run(case_id, non_linear, True)[1]
    for name, w in g.items():
        if not (name.endswith(".weight") and w.dim() == 2):
            continue
        n, k = w.shape
        for r in _edge_indices(n):
            f = w.clone()
            f[r] = 0
            yield f"row {r} zeroed", name, f, w[r]
        for c in _edge_indices(k):
            f = w.clone()
            f[:, c] = 0
            yield f"column {c} zeroed", name, f, w[:, c]
        if structural_only:
            continue
        if k >= 32:
            r0, c0 = (n // 2) // 16 * 16, ((k - 32) // 2) // 16 * 16
            r1 = min(n, r0 + 16)
            f = w.clone()
            f[r0:r1, c0:c0 + 16], f[r0:r1, c0 + 16:c0 + 32] = w[r0:r1, c0 + 16:c0 + 32], w[r0:r1, c0:c0 + 16]
            yield f"tile ({r0 // 16}, {c0 // 16}) swapped with its right neighbour", name, f, w[r0:r1, c0:c0 + 32]
        if k > 128:
            wd, h = min(128, k - 128), min(128, n)
            f = w.clone()
            f[:h, 128:128 + wd] = w[:h, :wd]
            yield "block (0, 1) stale: holds block (0, 0)", name, f, w[:h, :128 + wd]
        elif n > 128:
            h = min(128, n - 128)
            f = w.clone()
            f[128:128 + h] = w[:h]
            yield "block (1, 0) stale: holds block (0, 0)", name, f, w[:128 + h]
        bias = name[:-6] + "bias"
        if bias in g and g[bias].numel() > 128:
            f = g[bias].clone()
            f[128] = f[127]
            yield "bias element 128 holds element 127", bias, f, g[bias][127:129]
        yield "scaled by 1.02", name, w * 1.02, w
        leak = g1[name] * ((B + 1) / B) - w
        yield "one pad row leaks in", name, w + leak, leak
