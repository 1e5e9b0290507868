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

The baseline zoo (cases D*, M*, DW*).  Job.struct() turns on switches for the DMVAE family and mvtCAE that no
cVAE_multimodal case reaches -- ReLU (act_slope 0), the sigmoid output with -0.5 sum (x - x_hat)^2, private latent columns
that go from fc_mu straight into the modality's own decoder, tables without the covariate block, learnable loss weights
with their own gradient, and on the fused kernel mvtCAE's ProductOfExperts2 on variances, the variance floor and the
total-correlation term -- so those kinds get cases of their own, with the same two statistics, twin and bounds:
  * the oracle is R.dm_forward / R.dm_loss; the twin permutes the hidden units of fc1 and fc2; inputs are uniform in
    [0, 1); a WeightedDMVAE carries the unequal weights DM_WEIGHTS;
  * the linear run (statistic A) needs non_linear = 0, which Job.struct() never sends for these kinds: LinearDmJob clears
    the flag in the descriptor, and R.DmSpec(non_linear=False) is the oracle of that run.  The sigmoid output stays;
  * the ReLU run (statistic B) uses the flip handling as it is: slope 0 in place of 0.01, the same margin and the same
    cap.  tests/test_grad_check_cpu.py shows what a perturbation of the margin's size flips under ReLU;
  * rows [:n_private] of every fc_logvar weight and bias have no gradient at all (private_rows): they are held to the
    rule for a tensor that is zero -- untouched poison or exact zeros -- not to the slice floor;
  * zoo_faults seeds what these branches could get wrong: the private / shared boundary off by one, a private fc_logvar
    row that is not zero, the sigmoid's derivative missing on the last partial output chunk, weights[i] applied to another
    modality, the weights' gradients swapped, the total-correlation gradient stopping short of a ragged batch's end.
Every shape is the one the issue names: nm_validate_job accepts each as it stands, none had to move.  M1T is an addition:
M1 with the total-correlation weight at 0.1 per modality instead of the class's 1e-4.  At 1e-4 the term moves
enc_mean_layer's gradient by about 1e-3 of its largest element, and a fault in its last 8 batch rows by less than the
bf16 rounding of the delta it rides on (3.8e-4, FLOOR_A is 2e-3): M1, M2 and M3 run that code but cannot pin it.  At 0.1
the same fault is 4e-2 of the largest element, and M1T pins the term's backward pass on a ragged batch.
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
    kind: str            # "multimodal" | "mvtcae" | "dmvae" | "weighted_dmvae" | "mmvaeplus"
    wide: bool           # which root kernel must serve it
    seed: int
    bound_A: float       # linear stack, statistic A
    bound_B: float       # LeakyReLU (the DMVAE family: ReLU), statistic B
    tc_beta: float = R.MVT_BETA      # mvtCAE: weight of the total-correlation term per modality (the class has 1e-4)

    @property
    def is_dm(self) -> bool:
        return self.kind in DM_CLS

    @property
    def slope(self) -> float:
        """Negative slope of the activation: the DMVAE family's ReLU has none."""
        return 0.0 if self.is_dm else R.LEAKY_SLOPE

    @property
    def n_private(self) -> int:
        """DMVAE family: the first min(c_dim, Z) latent columns are private to their modality."""
        return min(self.c_dim, self.Z) if self.is_dm else 0


DM_CLS = {"dmvae": "DMVAE", "weighted_dmvae": "WeightedDMVAE", "mmvaeplus": "mmVAEPlus"}
DM_WEIGHTS = (0.8, 1.1, 1.3, 0.9)       # unequal, so that each weight's own gradient and scaling is seen


def _c(id, dims, hidden, Z, c_dim, B, combine, wide, seed, bound_A, bound_B, kind="multimodal", **kw):
    return GradCase(id, tuple(dims), tuple(hidden), Z, c_dim, B, combine, kind, wide, seed, bound_A, bound_B, **kw)


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
    # -- the baseline zoo on the fused step kernel (c_dim of a DMVAE-family case = its number of private latent columns) ---
    # twin distances measured on the CPU (A linear / B ReLU or LeakyReLU): D1 3.2e-5 / 5.8e-7, D2 5.4e-6 / 2.2e-8,
    # D3 2.9e-7 / 1.5e-4, D4 2.9e-4 / 1.2e-3, D5 0 / 0, D6 0 / 0, M1 3.4e-4 / 5.7e-4, M2 4.0e-8 / 6.1e-6, M3 1.1e-7 / 5.4e-8:
    # 4 x each is below its floor.  DW1 3.8e-4 / 2.9e-4, DW2 7.0e-4 / 3.2e-5, DW3 7.5e-4 / 8.9e-4: bound_A at 5.7 x.
    _c("D1", [77, 60], (127, 64), 20, 7, 130, "poe", False, 301, 2e-3, 8e-3, kind="dmvae"),
    _c("D2", [129, 61, 47], (64, 48), 12, 29, 255, "poe", False, 302, 2e-3, 8e-3, kind="dmvae"),
    _c("D3", [61, 90, 47], (64, 48), 12, 4, 256, "poe", False, 303, 2e-3, 8e-3, kind="weighted_dmvae"),
    _c("D4", [379, 379, 379, 1137], (110, 110), 10, 3, 256, "poe", False, 304, 2e-3, 8e-3, kind="mmvaeplus"),
    _c("D5", [60], (16, 127), 64, 63, 19, "poe", False, 305, 2e-3, 8e-3, kind="dmvae"),
    _c("D6", [45, 61], (100, 8), 17, 1, 1, "poe", False, 306, 2e-3, 8e-3, kind="dmvae"),
    _c("M1", [40, 40, 40, 40], (127,), 64, 5, 200, "poe", False, 311, 2e-3, 8e-3, kind="mvtcae"),
    _c("M1T", [40, 40, 40, 40], (127,), 64, 5, 200, "poe", False, 311, 2e-3, 8e-3, kind="mvtcae", tc_beta=0.1),
    _c("M2", [129, 33], (16, 127, 8), 5, 3, 255, "gpoe", False, 312, 2e-3, 8e-3, kind="mvtcae"),
    _c("M3", [50, 41], (90, 40), 20, 29, 19, "mopoe", False, 313, 2e-3, 8e-3, kind="mvtcae"),
    # -- the baseline zoo on the general-shape path ---------------------------------------------------------------------------
    _c("DW1", [70, 55, 33], (129, 257), 65, 6, 255, "poe", True, 321, 2.1e-3, 8e-3, kind="dmvae"),
    _c("DW2", [60, 45, 70], (300, 160), 128, 64, 200, "poe", True, 322, 4.0e-3, 8e-3, kind="weighted_dmvae"),
    _c("DW3", [37], (1024, 129), 100, 100, 83, "poe", True, 323, 4.3e-3, 8e-3, kind="mmvaeplus"),
]}
ZOO_IDS = [k for k, c in CASES.items() if k[0] in "DM"]
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
    uses the first B), covariates, draws, reference-rule weights.  The DMVAE family: inputs in [0, 1) (its outputs are
    sigmoids), tables without the covariate block (its networks take none), unequal loss weights for WeightedDMVAE."""

    def __init__(self, case: GradCase):
        gen = torch.Generator().manual_seed(case.seed)
        self.case = case
        n = case.B + 1
        if case.is_dm:
            self.xs = [torch.rand(n, d, generator=gen) for d in case.dims]
            self.c = torch.zeros(n, 0)
        else:
            self.xs = [torch.randn(n, d, generator=gen) * 1.2 for d in case.dims]
            self.c = onehot(gen, n, case.c_dim)
        self.eps = torch.randn(n, case.Z, generator=gen)
        self.P = nm.ParamLayout(self.spec(True)).init_reference_rule(case.seed)
        if "weights" in self.P:
            self.P["weights"] = torch.tensor(DM_WEIGHTS[:len(case.dims)])

    def spec(self, non_linear: bool) -> "nm.ModelSpec":
        c = self.case
        return nm.ModelSpec(list(c.dims), list(c.hidden), c.Z, c.c_dim, non_linear, c.kind)

    def ref_spec(self, non_linear: bool):
        """The oracle's description of the case."""
        c = self.case
        if c.is_dm:
            return R.DmSpec(list(c.dims), list(c.hidden), c.Z, c.c_dim, DM_CLS[c.kind], non_linear)
        return R.Spec(list(c.dims), list(c.hidden), c.Z, c.c_dim, non_linear)

    def job(self, non_linear: bool, device):
        """The case as a Job on `device`, gradient buffer NaN-poisoned."""
        c = self.case
        tables = [nm.Table(x[:c.B], self.c[:c.B], device) for x in self.xs]
        cls = LinearDmJob if c.is_dm and not non_linear else nm.Job
        job = cls(self.spec(non_linear), tables, combine=c.combine, state=self.P)
        if c.kind == "mvtcae":
            job.tc_weight = len(c.dims) * c.tc_beta
        job.set_eps(self.eps[:c.B])
        job.grads.fill_(float("nan"))
        return job


class LinearDmJob(nm.Job):
    """A DMVAE-family job as a LINEAR stack (statistic A).  The classes apply ReLU unconditionally, so Job.struct() forces
    non_linear = 1 for them; the kernels read that flag on its own, apart from act_slope, and this descriptor clears it."""

    def struct(self):
        j = super().struct()
        j.non_linear = 0
        return j


@functools.lru_cache(maxsize=None)
def data(case_id: str) -> CaseData:
    return CaseData(CASES[case_id])


def _run(cd: CaseData, P, non_linear: bool, rows: int, mode: str, trace: Optional[dict] = None, force: Optional[dict] = None,
         tweak: Optional[dict] = None, tc_mask: Optional[Tuple[int, int]] = None):
    """Loss dict and gradients of the oracle on the first `rows` rows, with `mode` operand rounding.  `trace`, if given,
    receives name -> [input, pre-activation, the layer's output as the layer after it receives it], the last two with
    their gradients retained, of every hidden layer's linear map (each layer runs once per forward pass).  `force`:
    name -> [(batch row, unit), ...] whose pre-activation is mirrored at zero (a constant is added, the gradient passes
    unchanged), so that the activation takes its other branch there.  `tweak`: name -> function applied to the result of
    that weight's linear map (seeded faults).  `tc_mask` (mvtCAE): (expert, first row) -- that expert's means of the rows
    from `first row` on enter the total-correlation term as constants (the value stays, their gradient is gone)."""
    c = cd.case
    rs = cd.ref_spec(non_linear)
    xs, cov, eps = [x[:rows] for x in cd.xs], cd.c[:rows].long(), cd.eps[:rows]
    fwd_fn, loss_fn = (R.mvt_forward, R.mvt_loss) if c.kind == "mvtcae" else (R.forward_multimodal, R.loss_multimodal)
    R.set_operand_rounding(mode)
    beta, R.MVT_BETA = R.MVT_BETA, c.tc_beta
    try:
        leaves = {k: v.clone().requires_grad_(True) for k, v in P.items()}
        if trace is not None or force or tweak:
            trace, force, tweak = ({} if trace is None else trace), (force or {}), (tweak or {})
            hidden_of = {id(leaves[w]): w for ws, _, _ in _chains(c) for w in ws}
            fed_by = {id(leaves[b]): a for ws, _, heads in _chains(c) for a, b in zip(ws, ws[1:] + heads[:1])}
            tweaked = {id(leaves[w]): f for w, f in tweak.items()}

            def hook(a, W, y):
                if id(W) in tweaked:
                    y = tweaked[id(W)](y)
                if id(W) in fed_by and fed_by[id(W)] in trace:          # (this map's input is the output of the layer before)
                    a.retain_grad()
                    trace[fed_by[id(W)]][2] = a
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
                trace[name] = [a.detach(), y, None]
                return y
            R.set_linear_hook(hook)
        if c.is_dm:
            fwd = R.dm_forward(leaves, rs, xs, eps)
            loss = R.dm_loss(leaves, rs, xs, fwd)
        else:
            fwd = fwd_fn(leaves, rs, xs, [cov] * len(xs), c.combine, eps)
            if tc_mask is not None:
                e, r0 = tc_mask
                fwd = {**fwd, "mus": [torch.cat((mu[:r0], mu[r0:].detach())) if m == e else mu for m, mu in enumerate(fwd["mus"])]}
            loss = loss_fn(rs, xs, fwd)
        loss["total"].sum().backward()
        grads = {k: (v.grad if v.grad is not None else torch.zeros_like(v)) for k, v in leaves.items()}
        return {k: float(torch.as_tensor(v).detach().sum()) for k, v in loss.items() if k != "ll_m"}, grads
    finally:
        R.MVT_BETA = beta
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
    """Reconstruction log-likelihood (summed over the modalities) of the fp32 oracle: the reference of run_case's bound.
    The DMVAE family: the oracle's `ll`, -0.5 sum (x - x_hat)^2 (times weights[i] for WeightedDMVAE)."""
    cd = data(case_id)
    c = cd.case
    rs = cd.ref_spec(non_linear)
    xs, cov = [x[:c.B] for x in cd.xs], cd.c[:c.B].long()
    with torch.no_grad():
        if c.is_dm:
            return float(R.dm_loss(cd.P, rs, xs, R.dm_forward(cd.P, rs, xs, cd.eps[:c.B]))["ll"])
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
        if case.is_dm:
            for p, heads in ((e, ["fc_mu", "fc_logvar"]), (d, ["fc_out"])):
                out.append(([f"{p}fc1.weight", f"{p}fc2.weight"], [f"{p}fc1.bias", f"{p}fc2.bias"], [f"{p}{h}.weight" for h in heads]))
            continue
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


def private_rows(case_id: str) -> Dict[str, int]:
    """name -> n: rows [:n] of the tensor have an identically zero oracle gradient inside a tensor that is not zero.  The
    DMVAE family's private latent columns go from fc_mu straight into the modality's own decoder: no draw, no KL, so
    rows [:n_private] of every fc_logvar weight and bias get no gradient (with n_private == latent that is the whole
    tensor).  Statistic B would hold such a row to SLICE_FLOOR of the largest row only; _zero_rule holds it exactly."""
    c = CASES[case_id]
    return {f"encoder_list.{m}.fc_logvar.{t}": c.n_private for m in range(len(c.dims)) for t in ("weight", "bias")} if c.n_private else {}


def _hold_zero_rows(got, want, zero_rows: Optional[Dict[str, int]], what: str):
    """Rows [:n] of the tensors named in `zero_rows` held to _zero_rule; returns `got` with those rows set to zero, so
    that what follows sees neither the poison an untouched row still holds nor those rows again."""
    out = dict(got)
    for name, n in (zero_rows or {}).items():
        if name in want:
            assert float(want[name][:n].abs().max()) == 0.0, (name, n, "the oracle's gradient is not zero there")
            _zero_rule(f"{name}[:{n}]", got[name][:n], what)
            out[name] = got[name].clone()
            out[name][:n] = 0
    return out


def element_distance(got: Dict[str, torch.Tensor], want: Dict[str, torch.Tensor]) -> Dict[str, float]:
    """Statistic A per tensor: max |got - want| / max |want| (tensors with want == 0 left out)."""
    return {k: float((got[k] - w).abs().max()) / float(w.abs().max()) for k, w in want.items() if float(w.abs().max()) > 0}


def assert_every_element(got, want, bound: float, what: str = "", zero_rows: Optional[Dict[str, int]] = None) -> Dict[str, float]:
    """Statistic A on every tensor of `want`; returns error / bound per tensor.  `zero_rows` (private_rows of the case):
    rows of a non-zero tensor the oracle leaves at zero, held to the rule for a tensor that is zero."""
    got = _hold_zero_rows(got, want, zero_rows, what)
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
                       flipped: Optional[list] = None, zero_rows: Optional[Dict[str, int]] = None) -> Dict[Tuple[str, str], float]:
    """Statistic B on every tensor of `want`; returns error / bound per (tensor, slice kind).

    `flips` (flip_model of the case): a ROW of a hidden layer's weight gradient that is beyond the bound is held instead
    against the oracle with ONE LeakyReLU unit of that row on the other side of zero -- a unit whose pre-activation lies
    inside its margin -- at the same bound; that flip's term is then taken out of the row and of the bias element, and every
    row, column and piece is checked as usual.  At most MAX_FLIPPED_ROWS of a tensor's rows (at least one) may pass that
    way; each is appended to `flipped` as (tensor, unit, batch row, pre-activation, margin, relative L2 before, after).
    `zero_rows`: as in assert_every_element."""
    got = _hold_zero_rows(got, want, zero_rows, what)
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
    bound, want, zero = CASES[case_id].bound_B, oracle_grads(case_id, True), private_rows(case_id)
    flipped = [] if flipped is None else flipped
    clean = {k: torch.nan_to_num(v) for k, v in got.items()}
    _take_out_flips(clean, want, bound, flip_model(case_id), flipped)
    if not flipped:
        return assert_every_slice(got, want, bound, what, zero_rows=zero)
    force: dict = {}
    for name, j, b, *_ in flipped:
        force.setdefault(name, []).append((b, j))
    cd = data(case_id)
    _, want2 = _run(cd, cd.P, True, cd.case.B, "bf16", force=force)
    return assert_every_slice(got, want2, bound, what + f" ({len(flipped)} sign flips)", zero_rows=zero)


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
    slope: float = R.LEAKY_SLOPE

    def row_candidates(self, j: int) -> Iterator[Tuple[int, torch.Tensor, float]]:
        """(batch row b, change of row j of the weight gradient, change of element j of the bias gradient) for every
        pre-activation of unit j inside its margin: the derivative `slope` (0.01; ReLU: 0) becomes 1, or the reverse."""
        for b in (self.pre[:, j].abs() < self.margin[:, j]).nonzero().flatten().tolist():
            d = (1.0 - self.slope) * float(self.dh[b, j]) * (1.0 if float(self.pre[b, j]) < 0 else -1.0)
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
    for name, (a, y, h) in trace.items():
        W, a, pre = R._bf(cd.P[name]).double(), R._bf(a).double(), y.detach().double()
        # dL/dh of the unit's output, read where the layer after it receives it (ReLU's inactive side passes nothing back
        # to the pre-activation to divide out)
        out[name] = FlipModel(pre, 2.0 ** -8 * (a.square() @ W.square().T).sqrt(), h.grad.double(), a, cd.case.slope)
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
    structural_only: the zeroed rows and columns alone (what statistic B is for); otherwise a zoo case's own faults
    (zoo_faults) follow."""
    cd = data(case_id)
    B = cd.case.B
    g = oracle_grads(case_id, non_linear)
    g1 = None if structural_only else oracle_run(case_id, non_linear, True)[1]
    for name, w in g.items():
        if not (name.endswith(".weight") and w.dim() == 2 and bool(w.any())):      # (all private: fc_logvar has no gradient)
            continue
        n, k = w.shape
        for r in _edge_indices(n):
            if not bool(w[r].any()):          # (a private fc_logvar row, a ReLU unit no row of the batch switches on:
                continue                      # zeroing zeros seeds nothing)
            f = w.clone()
            f[r] = 0
            yield f"row {r} zeroed", name, f, w[r]
        for c in _edge_indices(k):
            if not bool(w[:, c].any()):
                continue
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
    if not structural_only and case_id in ZOO_IDS:
        yield from zoo_faults(case_id, non_linear)


# ---- the baseline zoo's own faults ------------------------------------------------------------------------------------------
class _NoSigmoidFactor(torch.autograd.Function):
    """The identity, whose backward pass divides the incoming gradient by sigmoid'(y): behind it the output layer's delta
    is x_hat - x without the factor x_hat (1 - x_hat)."""

    @staticmethod
    def forward(ctx, y):
        s = torch.sigmoid(y)
        ctx.save_for_backward(s)
        return y.clone()

    @staticmethod
    def backward(ctx, g):
        s, = ctx.saved_tensors
        return g / (s * (1.0 - s))


def zoo_faults(case_id: str, non_linear: bool):
    """Yields (label, tensor name, faulty tensor, region), as seeded_faults does, for the faults the zoo's own branches of
    the kernels could have; `region` is what the fault removes from, moves in or adds to the ORACLE's gradient.

    DMVAE family: rows n_private - 1 and n_private of fc_mu (weight and bias) swapped; row n_private - 1 of fc_logvar.weight
    set to 1e-6 of the encoder's largest gradient element instead of zero; the sigmoid's derivative dropped on the last
    d % 16 output rows of fc_out (the oracle run again with _NoSigmoidFactor on those columns); with learnable weights,
    the gradients of weights[0] and weights[1] swapped, and decoder 0's gradients scaled as if by weights[1].
    mvtCAE: the total-correlation term's contribution of the last B % 64 batch rows missing in the last expert's
    enc_mean_layer gradient (the oracle run again with those rows masked out of the term, _run's tc_mask)."""
    cd = data(case_id)
    c, g = cd.case, oracle_grads(case_id, non_linear)
    M, S = len(c.dims), c.n_private
    if c.kind == "mvtcae":
        r0, e = c.B - c.B % 64, M - 1
        assert r0 < c.B
        name = f"encoder_list.{e}.enc_mean_layer.weight"
        _, g2 = _run(cd, cd.P, non_linear, c.B, "bf16", tc_mask=(e, r0))
        yield f"TC gradient stops at batch row {r0}", name, g2[name], g[name] - g2[name]
        return
    for m in range(M):
        p = f"encoder_list.{m}."
        if 0 < S < c.Z:
            for t in ("weight", "bias"):
                f = g[f"{p}fc_mu.{t}"].clone()
                f[[S - 1, S]] = f[[S, S - 1]]
                yield "boundary: fc_mu rows n_private - 1 and n_private swapped", f"{p}fc_mu.{t}", f, g[f"{p}fc_mu.{t}"][S - 1:S + 1]
        if S > 0:
            f = g[f"{p}fc_logvar.weight"].clone()
            f[S - 1] = 1e-6 * max(float(f.abs().max()), float(g[f"{p}fc_mu.weight"].abs().max()))
            yield "private: fc_logvar row n_private - 1 not zero", f"{p}fc_logvar.weight", f, f[S - 1]
    tail = {m: (d % 16 or 16) for m, d in enumerate(c.dims)}
    cut = lambda t: (lambda y: torch.cat((y[:, :-t], _NoSigmoidFactor.apply(y[:, -t:])), dim=1))
    _, g2 = _run(cd, cd.P, non_linear, c.B, "bf16", tweak={f"decoder_list.{m}.fc_out.weight": cut(t) for m, t in tail.items()})
    for m, t in tail.items():
        for name in (f"decoder_list.{m}.fc_out.weight", f"decoder_list.{m}.fc_out.bias"):
            yield f"sigmoid: no derivative on the last {t} output rows", name, g2[name], g2[name][-t:] - g[name][-t:]
    if "weights" in g:
        f = g["weights"].clone()
        f[[0, 1]] = f[[1, 0]]
        yield "weights: gradients of weights[0] and weights[1] swapped", "weights", f, g["weights"][:2]
        scale = float(cd.P["weights"][1] / cd.P["weights"][0])
        for k, v in g.items():
            if k.startswith("decoder_list.0."):
                yield "scaling: decoder 0 by weights[1]", k, v * scale, v
