"""The gradients of both root kernels against the oracle, element by element (tests/grad_check.py holds the statistics, the
bounds and where they come from).

Every other training launch is tied bit for bit or to a few ulp to the fused step kernel (nm_launch) or the general-shape
path (nm_launch_wide), and tests/adam_check.py ties every Adam update to the gradient it consumed; this module ties the
two roots' gradients to the bf16-operand oracle.  Each case runs ONE gradient launch (JobSet.grads(0)) into a NaN-poisoned
gradient buffer:

  * non_linear=False: statistic A -- per tensor max |got - oracle| <= bound_A * max |oracle|, every element finite, a
    tensor the oracle leaves at zero untouched or exactly zero;
  * non_linear=True: statistic B -- the relative L2 error of every row, every column and every 16-element vector piece
    <= bound_B.  Rows of hidden layers' weight gradients beyond it that ONE LeakyReLU unit of the row on the other branch
    explains -- a unit whose pre-activation lies inside its margin of zero (grad_check.flip_model), at most 1 % of a
    tensor's rows -- name the flipped units; the oracle is run again with exactly those units on the other branch and
    every row, column and piece is held to that run at the same bound.  The run prints every such unit;
  * both: the reconstruction loss within 1e-4 of the fp32 oracle (run_case's bound, scaled by sqrt(256 / B) below a full
    batch as in tests/test_gpu_fuzz.py).

The baseline zoo's cases (D*, M*, DW*: the DMVAE family and mvtCAE, whose descriptor switches no cVAE_multimodal case
reaches) run through the same _check; tests/grad_check.py says what differs for them.  The cases sit on the declared limits of the general-shape path (width 4096, latent 128, eight layers, four experts, mvtCAE's
experts x latent = 256) and on its block boundaries (127 / 128 / 129 columns, latent 65, z | c of exactly 128 and of 129
columns, an odd chunk count of the output layer, one row, ragged batches), and on the fused kernel's own limits.  All
limits at once (4 experts x 8 layers x 4096 columns) is too large for the CPU oracle and stays untested.

Result on the MI355X, worst error as a fraction of the bound (statistic A linear / statistic B LeakyReLU; 1.0 = at the
bound); no kernel was changed:
    W1 0.56 / 0.23    W2 0.16 / 0.32*   W3 0.11 / 0.16    W4 0.001 / 0.000    W5 0.19 / 0.19 (3 sign flips, see below)
    W6 0.000 / 0.003  W7 0.000 / 0.000  W8 0.11 / 0.06    W9 0.09 / 0.09
    F1 0.29 / 0.02    F2 0.10 / 0.16    F3 0.36 / 0.18    F4 0.000 / 0.000    F5 0.19 / 0.11    F6 0.50 / 0.003
The baseline zoo (DMVAE family: statistic B with ReLU; private fc_logvar rows held to exact zero; no kernel was changed, no
case needed a sign flip):
    D1 0.03 / 0.000   D2 0.12 / 0.11    D3 0.000 / 0.000  D4 0.24 / 0.13    D5 0.000 / 0.000  D6 0.000 / 0.000
    M1 0.18 / 0.07    M1T 0.18 / 0.07   M2 0.07 / 0.006   M3 0.21 / 0.000   DW1 0.14 / 0.11   DW2 0.17 / 0.05   DW3 0.17 / 0.004
All 26 runs together take under 4 s.  Four value faults planted in a scratch copy of csrc/nm_core.inc, one at a time, and
what failed (both runs of each case named): the private columns' d mu read one column early -> D1, D3, D4, D5, D6; no sigmoid
derivative on the last output chunk -> D1 .. D6; weights[m] taken from m - 1 -> D3; the total-correlation gradient stopping
at B & ~63 -> M1T (both runs) and M3 (linear run), while M1 and M2 pass: at the class's weight of 1e-4 that term is below any
bound a correct kernel meets (tests/grad_check.py, "The baseline zoo").
(* W2's bound_B is 0.29, its twin being that far away in single rows: with the slice floor a dropped row or column below
about 9 % of the tensor's largest passes statistic B there; statistic A on W2's linear run, bound 7e-3, sees it.)
The reconstruction loss of every run lies within its bound (W1: 7.7e-6).  Every case takes under 1.5 s.  The module prints
the table of the run at hand when it finishes (pytest -s).

W5 with LeakyReLU is the case that showed what a sign flip does to statistic B.  In batch row 87 three decoder units have
pre-activations next to zero -- decoder 0, layer 0, unit 218 (1.2e-4, margin 1.3e-3); decoder 1, layer 1, units 99 (1.2e-6)
and 279 (-9.2e-5, margin 5.8e-4) -- and on the MI355X all three land on the other side.  (Why is a hypothesis, not a
measurement: one latent of that row moved by one bf16 unit flips exactly these three of the row's 2400 decoder units on the
CPU, tests/test_grad_check_cpu.py; which rounding the kernel takes differently was not established.)  LeakyReLU's
derivative there is 1 instead of 0.01 or the reverse, and
that one term of the 256 moves each unit's whole row of the weight gradient: rows 218, 99 and 279 are 6.857e-2, 1.471e-2 and
8.660e-2 away from the plain oracle, and row 35 of decoder 1's layer 0, into which the two flipped gradients flow back,
2.352e-2 (bound_B 1.2e-2, twin distance 2.2e-3: W5's twin flips no unit).  The oracle run with exactly these three units
mirrored at zero gives the same four figures against the plain oracle on the CPU (6.858e-2, 1.47e-2, 8.659e-2, 2.362e-2;
tests/test_grad_check_cpu.py), and against that run every row, column and piece of W5 is within 0.19 of the bound.  No other
case needs a flip.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

import multi_modal_normative_modeling_amd as nm
from tests import grad_check as G
from tests.hip_harness import DEV

_WORST = {}
_FLIPPED = {}


@pytest.fixture(autouse=True)
def _bounded_memory():
    yield
    G.clear_cache()


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    print("\n[grad exact] worst error / bound per case (statistic A linear, statistic B LeakyReLU):")
    for cid in G.CASES:
        w = _WORST.get(cid, {})
        print(f"[grad exact]   {cid}  " + "  ".join(f"{k} {w[k][0]:.3f} ({w[k][1]})" for k in sorted(w))
              + (f"  [{_FLIPPED[cid]} row(s) with one sign flip]" if _FLIPPED.get(cid) else ""))


def _check(cid, non_linear):
    case = G.CASES[cid]
    cd = G.data(cid)
    job = cd.job(non_linear, DEV)
    assert job.spec.wide == case.wide, (cid, "served by the wrong root kernel")
    assert bool(torch.isnan(job.grads).all())
    nm.JobSet([job]).grads(0)
    torch.cuda.synchronize()
    got = job.grads_dict()
    want = G.oracle_grads(cid, non_linear)
    assert set(got) == set(want)
    ll32 = G.oracle_ll32(cid, non_linear)
    ll = float(job.loss_log[0, 2])
    tol = 1e-4 * max(1.0, (256.0 / case.B) ** 0.5)
    print(f"[grad exact] {cid} non_linear={non_linear}: reconstruction loss {ll!r} vs fp32 oracle {ll32!r}: "
          f"{abs(ll - ll32) / abs(ll32):.3e} (bound {tol:.1e})")
    if non_linear:
        d = G.slice_distance({k: torch.nan_to_num(v) for k, v in got.items()}, want)
        k = max(d, key=lambda q: d[q][0])
        print(f"[grad exact] {cid} statistic B: worst {d[k][0]:.3e} = {d[k][0] / case.bound_B:.3f} of the bound at {k} slice {d[k][1]}")
        flipped = []
        try:
            r = G.assert_every_slice_of_case(cid, got, f"{cid} {'ReLU' if case.is_dm else 'LeakyReLU'}", flipped)
        finally:
            for t in flipped:
                print(f"[grad exact] {cid} statistic B: {t[0]} row {t[1]} held against the oracle with unit {t[1]} flipped in batch "
                      f"row {t[2]} (pre-activation {t[3]:.3e}, margin {t[4]:.3e}): {t[5]:.3e} -> {t[6]:.3e}")
            _FLIPPED[cid] = len(flipped)
        key = "B"
    else:
        d = {k: v for k, v in G.element_distance({k: torch.nan_to_num(v) for k, v in got.items()}, want).items()}
        k = max(d, key=d.get)
        print(f"[grad exact] {cid} statistic A: worst {d[k]:.3e} = {d[k] / case.bound_A:.3f} of the bound in {k}")
        r = G.assert_every_element(got, want, case.bound_A, f"{cid} linear", zero_rows=G.private_rows(cid))
        key = "A"
    worst = max(r, key=r.get)
    _WORST.setdefault(cid, {})[key] = (r[worst], worst if isinstance(worst, str) else " ".join(worst))
    assert abs(ll - ll32) <= tol * abs(ll32), (cid, non_linear, ll, ll32)
    # the launch wrote every element of every tensor the oracle has a gradient for, and nothing is left of the poison there
    # (rows the oracle leaves at zero inside such a tensor -- grad_check.private_rows -- were held to the zero rule above)
    for k, w in want.items():
        if float(w.abs().max()) > 0:
            assert bool(torch.isfinite(got[k][G.private_rows(cid).get(k, 0):]).all()), k


@pytest.mark.parametrize("non_linear", [False, True], ids=["linear_A", "leaky_B"])
@pytest.mark.parametrize("cid", G.WIDE_IDS)
def test_general_shape_path(cid, non_linear):
    _check(cid, non_linear)


@pytest.mark.parametrize("non_linear", [False, True], ids=["linear_A", "leaky_B"])
@pytest.mark.parametrize("cid", G.FUSED_IDS)
def test_fused_kernel(cid, non_linear):
    _check(cid, non_linear)
