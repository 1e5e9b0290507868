"""The seeded draw behind the twin fuzz (tests/test_gpu_twins.py, tests/fuzz_many.py --twin): model shapes, options and
training knobs over the whole domain each bit-identical kernel twin admits.  Pure Python: no device, no library call.

A twin is a compact form of a kernel that is correct only because it equals the generic kernel bit for bit:
  "plain"          nm_step_kernel<false, 0, true> (NM_F_PLAIN)            against the generic step kernel
  "devpass"        nm_devpass (one expert)                                against nm_forward
  "devpass_multi"  nm_devpass_multi (2..4 experts)                        against nm_forward
  "latent"         nm_latent_pass                                         against nm_forward with the latent exports
  "split"          nm_launch_split (one workgroup per modality)           against one workgroup per model

draw(twin, seed) is a pure function of its arguments.  Every dimension comes from its edge list -- the tile sizes the kernels
are built on: 16-wide MFMA tiles, 64-column output chunks, 128- and 256-row tiles, the four-column latent path -- or
uniformly from its admitted range.  Seed s < len(edges) WALKS the edge list (one slot of the case takes edge (s * stride +
offset) mod len, strides coprime to the lengths, so a twin's first len(edges) seeds reach every edge whatever the generator
gives); every other slot, and every later seed, tosses a coin between a random edge and the uniform range.  M and the combiner
walk too (a Latin square where both have four values); the switches and training knobs are drawn.
tests/test_twin_cases_cpu.py holds the draw to its contract: every case admitted by the predicate it targets, every edge and
every option reached over a twin's seed list plus FIXED."""
from __future__ import annotations

from dataclasses import dataclass, replace
from typing import Optional, Tuple

import numpy as np
import torch

TWINS = ("plain", "devpass", "devpass_multi", "latent", "split")
TRAINING = ("plain", "split")
COMPACT_FORWARD = ("devpass", "devpass_multi", "latent")   # first hidden width <= 112, latent rounded to 16 <= 32
SEEDS = {"plain": tuple(range(32)), "devpass": tuple(range(16)), "devpass_multi": tuple(range(24)),
         "latent": tuple(range(24)), "split": tuple(range(16))}

D_EDGES = (3, 63, 64, 65, 127, 128, 129, 379, 420)
H_EDGES = (8, 15, 16, 17, 31, 32, 33, 63, 64, 65, 111, 112, 113, 126, 127)
Z_EDGES = (1, 2, 3, 4, 5, 8, 15, 16, 17, 31, 32, 33, 63, 64)
N_EDGES = (1, 15, 16, 17, 127, 128, 129, 255, 256, 257, 300, 383, 384, 385, 512, 513)
ZC1_TARGETS = (16, 17, 32, 33, 64, 65, 128)            # Z + c_dim + 1: whole and whole-plus-one k tiles of the decoder's input
D_RANGE, H_RANGE, C_RANGE, N_RANGE = (3, 420), (8, 127), (3, 29), (1, 513)
COMPACT_H0_MAX, COMPACT_Z_MAX, Z_MAX = 112, 32, 64
M_RANGE = {"plain": (1, 2, 3, 4), "devpass": (1,), "devpass_multi": (2, 3, 4), "latent": (1, 2, 3, 4), "split": (2, 3, 4)}
COMBINERS = ("poe", "gpoe", "moe", "mopoe")

LRS = (1e-4, 3e-3)
BETAS = ((0.9, 0.999), (0.5, 0.9))
ADAM_EPS = (1e-8, 1e-5)
KL_WEIGHTS = (None, 0.25, 4.0)
LL_WEIGHTS = (1.0, 0.5)
LR_TABLE_LENS = (0, 3, 7)                               # 0: no table
STEP_TOTALS = (3, 4, 5, 6)

# (stride, offset) of each dimension's walk over its edge list: coprime to every length the list can have, and different per
# dimension, so that seed s does not pair the s-th edge of one list with the s-th of another
_WALK = {"D": (2, 0), "H": (4, 3), "Z": (3, 5), "N": (5, 2)}


@dataclass(frozen=True)
class Case:
    twin: str
    name: str                              # "s<seed>" or the FIXED case's name
    dims: Tuple[int, ...]
    hidden: Tuple[int, ...]
    Z: int
    c_dim: int
    N: int
    combine: str
    non_linear: bool
    kind: str
    single_bypass: bool
    inject: bool                           # injected reparameterisation draws (else the in-kernel generator)
    shared_cov: bool                       # one covariate matrix for every modality (else one per modality)
    # training twins ("plain", "split"); the forward twins carry the defaults
    steps: Tuple[int, int] = (2, 1)        # two launches of a and b steps
    lr: float = 1e-4
    betas: Tuple[float, float] = (0.9, 0.999)
    adam_eps: float = 1e-8
    kl_weight: Optional[float] = None
    ll_weight: float = 1.0
    lr_table: Optional[Tuple[float, ...]] = None
    job_seed: int = 11                     # Job(seed=...): keys the in-kernel draws
    init_seed: int = 0                     # ParamLayout.init_reference_rule(init_seed)
    data_seed: int = 0                     # the tables and the injected draws

    @property
    def M(self) -> int:
        return len(self.dims)

    @property
    def id(self) -> str:
        return f"{self.twin}-{self.name}"


def z_edges(twin: str):
    return tuple(z for z in Z_EDGES if z <= (COMPACT_Z_MAX if twin in COMPACT_FORWARD else Z_MAX))


def kinds(twin: str, M: int):
    """The model kinds a Job can have and still pass the twin's predicate.  Job.plain_ok names "single" / "multimodal".
    Job.devpass_ok / devpass_multi_ok / latent_ok do not look at the kind: of the others, the DMVAE family fails n_private /
    is_dm, mvtCAE's Job always has tc_weight = M * 1e-4, the end-to-end trunk has 2 M kernel modalities for M encoders --
    "regression" is left: M modalities with an encoder each, Gaussian output, the regressor no part of a forward pass.
    "single" is the one-modality class.  The split launch is fuzzed on the kind the sweeps train with it."""
    if twin == "plain":
        return ("single", "multimodal") if M == 1 else ("multimodal",)
    if twin == "split":
        return ("multimodal",)
    return ("single", "multimodal", "regression") if M == 1 else ("multimodal", "regression")


def _walk(dim: str, edges, seed: int):
    stride, off = _WALK[dim]
    return edges[(seed * stride + off) % len(edges)] if seed < len(edges) else None


def _coin(rng, edges, lo: int, hi: int) -> int:
    """Half the time an edge, half the time uniform over [lo, hi]."""
    e, u = int(edges[int(rng.integers(0, len(edges)))]), int(rng.integers(lo, hi + 1))
    return e if rng.integers(0, 2) else u


def draw(twin: str, seed: int) -> Case:
    if twin not in TWINS:
        raise ValueError(f"unknown twin {twin!r}")
    rng = np.random.default_rng([TWINS.index(twin), int(seed)])
    compact = twin in COMPACT_FORWARD
    Ms = M_RANGE[twin]
    M = Ms[seed % len(Ms)]
    combine = COMBINERS[(seed + (seed // 4 if len(Ms) == 4 else 0)) % 4]
    # D per modality
    dims = [_coin(rng, D_EDGES, *D_RANGE) for _ in range(M)]
    slot = int(rng.integers(0, M))
    w = _walk("D", D_EDGES, seed)
    if w is not None:
        dims[slot] = w
    # hidden stack: the first width of the compact forward kernels stays within their first-layer stage
    L = int(rng.integers(1, 4))
    w = _walk("H", H_EDGES, seed)
    if w is not None and compact and w > COMPACT_H0_MAX:
        L = max(L, 2)
    h0_edges = tuple(h for h in H_EDGES if h <= COMPACT_H0_MAX) if compact else H_EDGES
    h0_hi = COMPACT_H0_MAX if compact else H_RANGE[1]
    hidden = [_coin(rng, h0_edges, H_RANGE[0], h0_hi)] + [_coin(rng, H_EDGES, *H_RANGE) for _ in range(L - 1)]
    slot = int(rng.integers(1 if (w is not None and compact and w > COMPACT_H0_MAX) else 0, L))
    if w is not None:
        hidden[slot] = w
    # latent width, covariate width (Z + c_dim <= 127 holds over the whole of both ranges)
    ze = z_edges(twin)
    Z = _coin(rng, ze, 1, ze[-1])
    w = _walk("Z", ze, seed)
    if w is not None:
        Z = w
    c_hit = [t - 1 - Z for t in ZC1_TARGETS if C_RANGE[0] <= t - 1 - Z <= C_RANGE[1]]
    c_any = int(rng.integers(C_RANGE[0], C_RANGE[1] + 1))
    c_pick, c_coin = int(rng.integers(0, 8)), int(rng.integers(0, 2))
    c_dim = c_hit[c_pick % len(c_hit)] if (c_hit and c_coin) else c_any
    # table rows
    N = _coin(rng, N_EDGES, *N_RANGE)
    w = _walk("N", N_EDGES, seed)
    if w is not None:
        N = w
    non_linear, shared_cov, inject = bool(rng.integers(0, 2)), bool(rng.integers(0, 2)), bool(rng.integers(0, 2))
    ks = kinds(twin, M)
    kind = ks[int(rng.integers(0, len(ks)))]
    bypass_coin = bool(rng.integers(0, 2))
    single_bypass = bypass_coin if (M == 1 and twin in ("plain", "latent")) else True    # (nm_devpass needs it on)
    # training knobs (drawn for every twin, so that the stream does not depend on the twin; used by the training twins)
    total = int(STEP_TOTALS[int(rng.integers(0, len(STEP_TOTALS)))])
    if N > 512:
        total = max(total, 4)                           # three batches per epoch: the wrap is step 3
    a = int(rng.integers(1, total))
    lens = [n for n in LR_TABLE_LENS if n == 0 or total % n]
    n_lr = int(lens[int(rng.integers(0, len(lens)))])
    lr = float(LRS[int(rng.integers(0, 2))])
    scale = rng.uniform(0.25, 1.75, size=7)
    case = Case(
        twin=twin, name=f"s{seed}", dims=tuple(dims), hidden=tuple(hidden), Z=Z, c_dim=c_dim, N=N, combine=combine,
        non_linear=non_linear, kind=kind, single_bypass=single_bypass, inject=inject, shared_cov=shared_cov,
        steps=(a, total - a), lr=lr, betas=BETAS[int(rng.integers(0, 2))], adam_eps=float(ADAM_EPS[int(rng.integers(0, 2))]),
        kl_weight=KL_WEIGHTS[int(rng.integers(0, 3))], ll_weight=float(LL_WEIGHTS[int(rng.integers(0, 2))]),
        lr_table=tuple(float(lr * s) for s in scale[:n_lr]) if n_lr else None,
        job_seed=int(rng.integers(1, 1 << 30)), init_seed=int(rng.integers(0, 1 << 30)), data_seed=int(rng.integers(0, 1 << 30)))
    if twin not in TRAINING:
        d = Case.__dataclass_fields__
        case = replace(case, **{f: d[f].default for f in ("steps", "lr", "betas", "adam_eps", "kl_weight", "ll_weight", "lr_table")})
    return case


def _fixed(twin, name, dims, hidden, Z, c_dim, N, **kw):
    kw = {"combine": "gpoe", "non_linear": True, "kind": "multimodal", "single_bypass": True, "inject": False,
          "shared_cov": True, **kw}
    return Case(twin=twin, name=name, dims=tuple(dims), hidden=tuple(hidden), Z=Z, c_dim=c_dim, N=N, **kw)


def _smallest(twin):
    """Every dimension at the lower end of its admitted range, M at the twin's minimum."""
    return _fixed(twin, "smallest", (D_RANGE[0],) * M_RANGE[twin][0], (H_RANGE[0],), 1, C_RANGE[0], N_RANGE[0], steps=(2, 1))


UCA = (379, 379, 379, 1137)
# hand-written cases the random ranges leave out.  The smallest case of "devpass" / "devpass_multi" is also the reduced case
# of what the fuzz found there ("Twin fuzz: findings"): one table row, so 112 export rows of the live 128-row tile
# and every out_rowdev row behind the table that the compact kernels used to leave as they were
FIXED = {
    "plain": [
        _fixed("plain", "early_fusion_1137", (1137,), (110, 110), 10, 29, 300, steps=(2, 1)),      # 18 output chunks
        _fixed("plain", "uca", UCA, (110, 110), 10, 29, 300, steps=(2, 1)),                        # the M = 4 sweep model
        _smallest("plain"),
    ],
    "devpass": [
        _fixed("devpass", "early_fusion_1137", (1137,), (110, 110), 10, 29, 300),
        _smallest("devpass"),
    ],
    "devpass_multi": [
        _fixed("devpass_multi", "uca", UCA, (110, 110), 10, 29, 300),
        _smallest("devpass_multi"),
    ],
    "latent": [_smallest("latent")],
    "split": [_smallest("split")],
}


def cases(twin: str):
    """Every case of a twin: its seed list, then its FIXED cases."""
    return [draw(twin, s) for s in SEEDS[twin]] + list(FIXED[twin])


_BITS = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}


def _pattern(t: torch.Tensor, i: int) -> str:
    e = t.reshape(-1)[i:i + 1].contiguous()
    size = e.element_size()
    bits = int(e.view(_BITS[size]).item()) & ((1 << (8 * size)) - 1)
    return f"{e.item()!r} (0x{bits:0{2 * size}x})"


def assert_same(a, b, what):
    """torch.equal per named tensor of the two dicts; the failure names the tensor, the number of differing elements, the
    first differing flat index and both bit patterns there."""
    assert list(a) == list(b), (what, list(a), list(b))
    for k in a:
        x, y = a[k], b[k]
        assert x.shape == y.shape and x.dtype == y.dtype, (what, k, tuple(x.shape), tuple(y.shape), x.dtype, y.dtype)
        if torch.equal(x, y):
            continue
        ne = (x.reshape(-1) != y.reshape(-1)).nonzero().flatten()
        i = int(ne[0])
        raise AssertionError(f"{what}: {k} differs in {ne.numel()} of {x.numel()} elements; first at flat index {i}: "
                             f"{_pattern(x, i)} against {_pattern(y, i)}")
