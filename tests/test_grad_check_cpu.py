"""The gradient checker (tests/grad_check.py) on the CPU: its bounds are tied to the oracle's twin, it flags every seeded
fault, and the limits of the general-shape path refuse what lies just past them.

  * Every committed bound_A / bound_B lies between 4 x and 8 x the oracle-to-twin distance recomputed here, or at its
    floor where 4 x the distance is below the floor.  The twin itself passes both statistics at those bounds.
  * Seeded faults (grad_check.seeded_faults), applied to the oracle's own gradients of the LINEAR stack, for every weight
    matrix of every case in turn: statistic A must flag each.  A fault may go unflagged only where the oracle's own values
    in the slice it touches are below twice the bound (nothing is there to lose); those are counted and must stay under
    5 % of the case's faults.
  * With LeakyReLU on, statistic B -- with its allowance for one sign flip per row switched on, as the GPU tests run it --
    must flag every zeroed row and column the same way, in statistic B's own measure: unflagged only where the slice's norm is below twice
    the bound times the slice floor.  The cap is wider there, 25 %: an inactive LeakyReLU unit carries 1 / 100 of an active
    one's gradient, so in a batch of 1 row (W7) or 19 rows (W4) a sixth of the tested rows and columns lie under the slice
    floor (measured: W4 32 of 194, W7 11 of 60, W2 3 of 46, every other case under 5 %).  Statistic A flags those very
    slices on the linear stack, where no unit is inactive.
  * The sign flips the MI355X showed on W5, forced into the oracle: the checker names exactly those units, meets that run,
    and still fails a structural fault on top of them.
  * The rule for a tensor whose oracle gradient is identically zero, and for elements that were never written.
  * The baseline zoo's cases (D*, M*, DW*): the same bounds test and seeded faults, the zoo's own faults
    (grad_check.zoo_faults) flagged by both statistics, the private fc_logvar rows held to exact zero inside a non-zero
    tensor, and what a perturbation of the flip margin's size does under ReLU.
  * Width 4097, latent 129, 9 layers, mvtCAE 3 x 86: ValueError from ModelSpec.validate; width and latent also the named
    status from nm_validate_job (tests/test_cabi_cpu.py has the other two); the limits themselves are accepted.
"""
import ctypes as C

import pytest
import torch

import multi_modal_normative_modeling_amd as nm
from multi_modal_normative_modeling_amd import _lib
from tests import grad_check as G
from tests.test_cabi_cpu import _probe, lib          # noqa: F401  (the host descriptor and the library fixture)

SKIP_CAP = 0.05
SKIP_CAP_B = 0.25


@pytest.fixture(autouse=True)
def _bounded_memory():
    """The cached oracle runs of one case (W2: two 4096 x 4096 gradients each) do not outlive the test that used them."""
    yield
    G.clear_cache()


@pytest.mark.parametrize("cid", list(G.CASES))
def test_bounds_are_tied_to_the_twin(cid):
    case = G.CASES[cid]
    dist = G.twin_distance(cid)
    print(f"[grad check] {cid}: twin distance A {dist[0]:.3e} (bound {case.bound_A:.1e}), B {dist[1]:.3e} (bound {case.bound_B:.1e})")
    for stat, d, bound, floor in (("A", dist[0], case.bound_A, G.FLOOR_A), ("B", dist[1], case.bound_B, G.FLOOR_B)):
        assert bound >= floor, (cid, stat, bound, floor)
        if bound == floor:
            assert G.FACTOR_LO * d <= floor, (cid, stat, "at the floor, but 4 x the twin distance is above it", d)
        else:
            assert G.FACTOR_LO * d <= bound <= G.FACTOR_HI * d, (cid, stat, bound, d, bound / d)
    assert case.bound_A < 0.02 and case.bound_B < 1.0          # (a 2 % scale error / a dropped slice must stay visible)
    ra = G.assert_every_element(G.twin_grads(cid, False), G.oracle_grads(cid, False), case.bound_A, f"{cid} twin")
    rb = G.assert_every_slice(G.twin_grads(cid, True), G.oracle_grads(cid, True), case.bound_B, f"{cid} twin")
    assert max(ra.values()) <= 1.0 / G.FACTOR_LO + 1e-9 and max(rb.values()) <= 1.0 / G.FACTOR_LO + 1e-9
    assert G.data(cid).spec(True).wide == case.wide


def _flagged(check, name, faulty, want, bound, **kw):
    try:
        check({name: faulty}, {name: want}, bound, "seeded", **kw)
    except AssertionError:
        return True
    return False


@pytest.mark.parametrize("cid", list(G.CASES))
def test_every_seeded_fault_is_flagged_by_statistic_A(cid):
    case = G.CASES[cid]
    g = G.oracle_grads(cid, False)
    G.assert_every_element(g, g, case.bound_A, cid)
    n = skipped = 0
    kinds = set()
    for label, name, faulty, region in G.seeded_faults(cid, False):
        n += 1
        kinds.add(label.split(" ")[0])
        if _flagged(G.assert_every_element, name, faulty, g[name], case.bound_A, zero_rows=G.private_rows(cid)):
            continue
        # unflagged: allowed only where the oracle itself has (next to) nothing in the slice the fault touches
        assert float(region.abs().max()) < 2 * case.bound_A * float(g[name].abs().max()), (cid, name, label, "not flagged")
        skipped += 1
    print(f"[grad check] {cid}: {n} seeded faults, {skipped} on slices the oracle leaves (nearly) empty")
    assert {"row", "column", "scaled", "one"} <= kinds and n >= 10 * len(case.dims)
    assert skipped < SKIP_CAP * n, (cid, skipped, n)


@pytest.mark.parametrize("cid", list(G.CASES))
def test_every_dropped_row_and_column_is_flagged_by_statistic_B(cid):
    case = G.CASES[cid]
    g = G.oracle_grads(cid, True)
    fm = G.flip_model(cid)
    G.assert_every_slice(g, g, case.bound_B, cid, fm)
    n = skipped = 0
    for label, name, faulty, region in G.seeded_faults(cid, True, structural_only=True):
        n += 1
        bias = name[:-6] + "bias"
        flips = {name: fm[name]} if name in fm else None           # (with the flip allowance on, as on the GPU)
        try:
            G.assert_every_slice({name: faulty, bias: g[bias]}, {name: g[name], bias: g[bias]}, case.bound_B, "seeded", flips)
        except AssertionError:
            continue
        w = g[name]
        norms = (w if label.startswith("row") else w.T).double().norm(dim=1)
        assert float(region.double().norm()) < 2 * case.bound_B * G.SLICE_FLOOR * float(norms.max()), (cid, name, label, "not flagged")
        skipped += 1
    print(f"[grad check] {cid}: {n} dropped rows / columns, {skipped} on slices the oracle leaves (nearly) empty")
    assert skipped < SKIP_CAP_B * n, (cid, skipped, n)


ZOO_FAULTS = {"dmvae": {"boundary", "private", "sigmoid"}, "mmvaeplus": {"boundary", "private", "sigmoid"},
              "weighted_dmvae": {"boundary", "private", "sigmoid", "weights", "scaling"}, "mvtcae": {"TC"}}


@pytest.mark.parametrize("cid", G.ZOO_IDS)
def test_every_zoo_fault_is_flagged_by_both_statistics(cid):
    """grad_check.zoo_faults -- the private / shared boundary off by one row, a private fc_logvar row at 1e-6 of the
    largest element, no sigmoid derivative on the last partial output chunk, the weights' gradients swapped, a decoder
    scaled by another modality's weight -- seeded into the oracle's gradients: statistic A on the linear stack and
    statistic B with the activation on each flag every one of them (the private row through the zero rule).

    mvtCAE's total-correlation term is the exception, and a finding of this module: at the class's weight of 1e-4 per
    modality the whole term moves enc_mean_layer's gradient by about 1e-3 of its largest element, and the rows 192 .. 199
    of M1 by less than the bf16 rounding of the delta they ride on (the seeded fault measures 3.8e-4 in M1, 4.3e-4 in M2,
    2.5e-3 in M3, where all 19 rows go; FLOOR_A is 2e-3).  No element-wise bound that a correct kernel meets sees that, so
    for M1, M2 and M3 this test only holds the fault to be that small; M1T -- M1 with the term's weight at 0.1 -- is the
    case that pins the term's backward pass on a ragged batch, and there both statistics must flag it."""
    case, zero = G.CASES[cid], G.private_rows(cid)
    expected = set(ZOO_FAULTS[case.kind])
    if case.n_private == case.Z:
        expected.discard("boundary")                           # (every column private: no boundary inside the latent)
    for non_linear, check, bound in ((False, G.assert_every_element, case.bound_A), (True, G.assert_every_slice, case.bound_B)):
        g = G.oracle_grads(cid, non_linear)
        seen = set()
        for label, name, faulty, region in G.zoo_faults(cid, non_linear):
            seen.add(label.split(":")[0].split(" ")[0])
            if _flagged(check, name, faulty, g[name], bound, zero_rows=zero):
                continue
            assert case.kind == "mvtcae" and case.tc_beta == G.R.MVT_BETA, (cid, non_linear, name, label, "not flagged")
            assert float(region.abs().max()) < 2 * G.FLOOR_A * float(g[name].abs().max()), (cid, name, label)
        assert seen == expected, (cid, seen, expected)


def test_private_rows_are_held_to_the_zero_rule():
    """Rows [:n_private] of fc_logvar inside a tensor that is not zero: exact zeros or untouched poison pass, 1e-6 of the
    largest element does not -- in either statistic, and statistic B's slice floor alone would let it through."""
    cid = "D1"
    g, zero = G.oracle_grads(cid, True), G.private_rows(cid)
    name = "encoder_list.1.fc_logvar.weight"
    assert zero[name] == 7 and float(g[name][:7].abs().max()) == 0.0 and float(g[name][7:].abs().max()) > 0.0
    want = {name: g[name]}
    bad = g[name].clone()
    bad[6, 60] = 1e-6 * float(g[name].abs().max())
    poison = g[name].clone()
    poison[:7] = float("nan")
    for check, bound in ((G.assert_every_element, G.CASES[cid].bound_A), (G.assert_every_slice, G.CASES[cid].bound_B)):
        check({name: g[name].clone()}, want, bound, cid, zero_rows=zero)
        check({name: poison}, want, bound, cid, zero_rows=zero)
        with pytest.raises(AssertionError, match=r"identically zero.*fc_logvar.weight\[:7\]\[6, 60\]"):
            check({name: bad}, want, bound, cid, zero_rows=zero)
        with pytest.raises(AssertionError, match="not finite"):
            check({name: poison}, want, bound, cid)                    # (without the rule the poison is an unwritten element)
    G.assert_every_slice({name: bad}, want, G.CASES[cid].bound_B, cid)          # the slice floor alone does not see it
    # every column private (D2): the whole tensor is zero and the rule for such a tensor holds it
    g2 = G.oracle_grads("D2", True)
    assert all(float(g2[k].abs().max()) == 0.0 for k in G.private_rows("D2"))


def test_zero_and_unwritten_rules():
    """want == 0: untouched (all NaN) or exact zeros, nothing else; want != 0: every element finite.  Both statistics."""
    nan = float("nan")
    want = {"alpha": torch.zeros(1), "w": torch.tensor([[1.0, -2.0], [0.5, 0.25]])}
    for check in (G.assert_every_element, G.assert_every_slice):
        check({"alpha": torch.tensor([nan]), "w": want["w"].clone()}, want, 1e-2)
        check({"alpha": torch.zeros(1), "w": want["w"] * 1.001}, want, 1e-2)
        for alpha in (torch.tensor([1e-30]), torch.tensor([float("inf")])):
            with pytest.raises(AssertionError, match="identically zero"):
                check({"alpha": alpha, "w": want["w"].clone()}, want, 1e-2)
        for bad in (nan, float("inf")):
            w = want["w"].clone()
            w[1, 0] = bad
            with pytest.raises(AssertionError, match="not finite"):
                check({"alpha": torch.zeros(1), "w": w}, want, 1e-2)
    z2 = {"v": torch.zeros(3)}
    with pytest.raises(AssertionError, match="identically zero"):       # partly written
        G.assert_every_element({"v": torch.tensor([nan, 0.0, nan])}, z2, 1e-2)
    # the failure names the tile: row 130 = 128 * 1 + 16 * 0 + 2
    w = torch.ones(200, 40)
    f = w.clone()
    f[130, 17] = 0.0
    with pytest.raises(AssertionError, match=r"w\[130, 17\].*128 \* 1 \+ 16 \* 0 \+ 2"):
        G.assert_every_element({"w": f}, {"w": w}, 5e-3)
    with pytest.raises(AssertionError, match="row 130"):
        G.assert_every_slice({"w": f}, {"w": w}, 5e-3)


def test_twin_is_the_same_network():
    """In fp32 the twin's loss equals the oracle's to summation order, and un-permuting restores every gradient's place."""
    cd = G.data("W3")
    perms = G.twin_perms(cd.case, cd.P)
    assert len(perms) == 3 * (2 * 2 * 3 + 3)               # 3 modalities x (3 weights + 3 biases, encoder and decoder; 3 heads)
    Pt = {k: (G._permute(v, *perms[k]) if k in perms else v) for k, v in cd.P.items()}
    l0, g0 = G._run(cd, cd.P, True, cd.case.B, "fp32")
    l1, g1 = G._run(cd, Pt, True, cd.case.B, "fp32")
    assert abs(l0["total"] - l1["total"]) <= 1e-5 * abs(l0["total"])
    for k, v in g1.items():
        back = G._permute(v, G._inverse(perms[k][0]), G._inverse(perms[k][1])) if k in perms else v
        assert float((back - g0[k]).abs().max()) <= 1e-4 * float(g0[k].abs().max()) + 1e-12, k
    moved = [k for k in perms if perms[k][0] is not None and not torch.equal(Pt[k], cd.P[k])]
    assert len(moved) == 3 * 2 * 2 * 3


def test_one_sign_flip_moves_a_whole_row_and_is_the_only_thing_allowed():
    """The finding behind statistic B's flip allowance, from the oracle alone.  Unit 279 of decoder 1's second hidden layer
    in W5 has the pre-activation -9.2e-5 in batch row 87 (the unit's median: 8.4e-2; its margin: 5.8e-4).  On the other
    side of zero LeakyReLU's derivative is 1 instead of 0.01 and ROW 279 of that layer's weight gradient moves by
    0.99 |dL/dh| ||a[87, :]|| = 8.6e-2 of statistic B's denominator, 7 x bound_B (the MI355X showed 8.66e-2 there), while
    W5's twin flips no unit (distance 2.2e-3).  The checker holds such a row against the oracle with that one flip -- and
    nothing else: not a unit outside its margin, not two flips in a row, not a dropped row, not more rows than
    MAX_FLIPPED_ROWS of a tensor."""
    cid, name, j, row = "W5", "decoder_list.1.decoder_layers.1.weight", 279, 87
    bias, bound = name[:-6] + "bias", G.CASES[cid].bound_B
    want, fm = G.oracle_grads(cid, True), G.flip_model(cid)
    f = fm[name]
    assert -2e-4 < float(f.pre[row, j]) < 0 and float(f.pre[:, j].abs().median()) > 0.05
    assert 4e-4 < float(f.margin[row, j]) < 8e-4
    near = sum(int((m.pre.abs() < m.margin).sum()) for m in fm.values()) / sum(m.pre.numel() for m in fm.values())
    assert near < 0.005                                        # (the margin admits 0.3 % of the pre-activations)
    cand = {b: (dw, db) for b, dw, db in f.row_candidates(j)}
    assert row in cand

    def moved(pairs):
        g = {k: v.clone() for k, v in want.items()}
        for jj, dw, db in pairs:
            g[name][jj] += dw.float()
            g[bias][jj] += db
        return g

    got = moved([(j, *cand[row])])
    d = G.slice_distance(got, want)[(name, "row")]
    print(f"[grad check] W5: one sign flip at (row {row}, unit {j}) moves the weight-gradient row by {d[0]:.3e} of its denominator")
    assert d[1] == j and 0.08 < d[0] < 0.095 and d[0] > 5 * bound
    with pytest.raises(AssertionError, match="row 279"):
        G.assert_every_slice(got, want, bound, cid)
    flipped = []
    r = G.assert_every_slice(got, want, bound, cid, fm, flipped)
    assert max(r.values()) < 1e-3 and [t[:3] for t in flipped] == [(name, j, row)]
    # a unit far outside its margin: the same move is not admissible
    far = int(((f.pre[:, j].abs() > 10 * f.margin[:, j]) * f.dh[:, j].abs() * f.a.norm(dim=1)).argmax())
    d_far = 0.99 * float(f.dh[far, j]) * f.a[far]
    with pytest.raises(AssertionError, match="row 279"):
        G.assert_every_slice(moved([(j, d_far, 0.0)]), want, bound, cid, fm)
    # the flip and a second term of the same row; the row dropped
    with pytest.raises(AssertionError, match="row 279"):
        G.assert_every_slice(moved([(j, *cand[row]), (j, d_far, 0.0)]), want, bound, cid, fm)
    g = moved([])
    g[name][j] = 0
    with pytest.raises(AssertionError, match="row 279"):
        G.assert_every_slice(g, want, bound, cid, fm)
    # more admissible flips in one tensor than MAX_FLIPPED_ROWS allows (300 rows: 3)
    many = []
    for jj in range(f.pre.shape[1]):
        c = max(f.row_candidates(jj), key=lambda t: float(t[1].norm()), default=None)
        wn = want[name].double().norm(dim=1)
        if c is not None and float(c[1].norm()) > 2 * bound * max(float(wn[jj]), G.SLICE_FLOOR * float(wn.max())):
            many.append((jj, c[1], c[2]))
    assert len(many) > 3
    G.assert_every_slice(moved(many[:3]), want, bound, cid, fm)
    with pytest.raises(AssertionError, match=f"row {many[3][0]}"):
        G.assert_every_slice(moved(many[:4]), want, bound, cid, fm)


def test_oracle_with_named_units_flipped_is_recovered_and_nothing_else_passes():
    """What the MI355X showed on W5, from the oracle alone: three units of batch row 87 on LeakyReLU's other branch move
    their rows by 6.86e-2, 1.47e-2 and 8.66e-2 of statistic B's denominator and row 35 of the layer below by 2.36e-2.  The
    checker names exactly these units from the rows, and the oracle run with them flipped is met exactly; a structural
    fault on top of the flips still fails."""
    cid = "W5"
    cd, want, bound = G.data(cid), G.oracle_grads(cid, True), G.CASES[cid].bound_B
    d0, d1 = "decoder_list.0.decoder_layers.0.weight", "decoder_list.1.decoder_layers.1.weight"
    _, got = G._run(cd, cd.P, True, cd.case.B, "bf16", force={d0: [(87, 218)], d1: [(87, 99), (87, 279)]})
    d = G.slice_distance(got, want)
    assert d[(d1, "row")][1] == 279 and abs(d[(d1, "row")][0] - 8.66e-2) < 1e-3
    assert d[(d0, "row")][1] == 218 and abs(d[(d0, "row")][0] - 6.86e-2) < 1e-3
    assert d[("decoder_list.1.decoder_layers.0.weight", "row")][1] == 35
    assert abs(d[("decoder_list.1.decoder_layers.0.weight", "row")][0] - 2.36e-2) < 1e-3
    with pytest.raises(AssertionError):
        G.assert_every_slice(got, want, bound, cid)
    flipped = []
    r = G.assert_every_slice_of_case(cid, got, cid, flipped)
    assert sorted(t[:3] for t in flipped) == [(d0, 218, 87), (d1, 99, 87), (d1, 279, 87)] and max(r.values()) < 1e-6
    _, again = G._run(cd, cd.P, True, cd.case.B, "bf16")
    assert all(torch.equal(again[k], want[k]) for k in want)        # (forcing leaves nothing behind in the oracle)
    for name, fault in (("decoder_list.1.decoder_layers.0.weight", lambda t: t[35].zero_()),
                        ("decoder_list.2.decoder_mean_layer.weight", lambda t: t[:, 128].zero_()),
                        (d1, lambda t: t[:, 284].zero_())):
        bad = {k: v.clone() for k, v in got.items()}
        fault(bad[name])
        with pytest.raises(AssertionError, match="relative L2"):
            G.assert_every_slice_of_case(cid, bad, cid)


def test_one_bf16_unit_of_one_latent_flips_exactly_the_three_units_of_w5():
    """A HYPOTHESIS for where W5's three flips come from, checked as far as the CPU can: move ONE latent of batch row 87 by
    one bf16 unit (z[87, 20] or z[87, 25], upwards) and, of the 2400 decoder units of that row, exactly the three the
    MI355X flips change sign: decoder 0 layer 0 unit 218, decoder 1 layer 1 units 99 and 279.  Which rounding the kernel
    takes differently is NOT established (neither latent lies next to a bf16 tie in the oracle; a bf16 rounding of an
    encoder activation that falls the other way moves a latent by about as much).  It shows that a perturbation of the size
    the flip margin models produces this very pattern."""
    cd, fm = G.data("W5"), G.flip_model("W5")
    bf = lambda t: t.to(torch.bfloat16).float()

    def changed(a):
        out = set()
        for m in range(4):
            h = a
            for i in range(2):
                p = f"decoder_list.{m}.decoder_layers.{i}."
                pre = bf(h) @ bf(cd.P[p + "weight"]).T + cd.P[p + "bias"]
                ref = fm[p + "weight"].pre[87]
                out |= {(m, i, j) for j in ((pre >= 0) != (ref >= 0)).nonzero().flatten().tolist()}
                h = torch.nn.functional.leaky_relu(pre, 0.01)
        return out

    a0 = fm["decoder_list.0.decoder_layers.0.weight"].a[87].float()           # bf16(z | c) of row 87
    assert changed(a0) == set()
    for k in (20, 25):
        a = a0.clone()
        a[k] += 2.0 ** (int(torch.floor(torch.log2(a[k].abs()))) - 7)
        assert changed(a) == {(0, 0, 218), (1, 1, 99), (1, 1, 279)}, k


# ---- refusals just past the edge of the general-shape path ----------------------------------------------------------------
def _wide(**kw):
    """A host descriptor of the general-shape path."""
    j = _probe(**{"D": 37, "L": len(kw.get("H", (110, 110))), **kw})
    j.wide, j.w_off, j.wsh = 1, -1, None
    return j


EDGES = [
    # what, accepted, refused, status   (9 layers and mvtCAE 3 x 86 -> NM_E_LAYERS / NM_E_WIDE_TC: tests/test_cabi_cpu.py
    # asserts those two codes already; their Python side is below)
    ("width", dict(H=(4096,)), dict(H=(4097,)), "NM_E_WIDTH"),
    ("latent", dict(H=(300,), Z=128), dict(H=(300,), Z=129), "NM_E_LATENT"),
]


@pytest.mark.parametrize("what,ok,bad,status", EDGES, ids=[e[0] for e in EDGES])
def test_general_shape_limits_in_c(lib, what, ok, bad, status):
    assert (_lib.NM_WIDE_MAX_WIDTH, _lib.NM_WIDE_MAX_LATENT, _lib.NM_MAX_HID, _lib.NM_MAX_EXP) == (4096, 128, 8, 4)
    assert lib.nm_validate_job(C.byref(_wide(**ok))) == 0
    assert lib.nm_validate_job(C.byref(_wide(**bad))) == getattr(_lib, status)


def test_general_shape_limits_in_python():
    def spec(hidden, Z=10, dims=(37,), c_dim=29, kind="multimodal"):
        return nm.ModelSpec(list(dims), list(hidden), Z, c_dim, True, kind)

    for ok in (spec([4096]), spec([300], Z=128), spec([300] + [8] * 7), spec([130], Z=64, dims=[40] * 4, c_dim=5, kind="mvtcae"),
               spec([130], Z=128, dims=[40, 33], c_dim=5, kind="mvtcae")):
        ok.validate()
        assert ok.wide
        nm.ParamLayout(ok)
    for bad, msg in ((spec([4097]), "hidden widths"), (spec([300], Z=129), "latent_dim"), (spec([300] + [8] * 8), "hidden layers"),
                     (spec([130], Z=86, dims=[40] * 3, c_dim=5, kind="mvtcae"), "modalities x latent_dim <= 256")):
        with pytest.raises(ValueError, match=msg):
            bad.validate()
        with pytest.raises(ValueError, match=msg):
            nm.ParamLayout(bad)


@pytest.mark.parametrize("cid", [k for k in G.ZOO_IDS if G.CASES[k].is_dm])
def test_one_bf16_unit_of_one_latent_under_relu(cid):
    """flip_model's margin at slope 0, from the oracle alone: every decoder input column (shared latents and private
    means) of every batch row moved up by ONE bf16 unit in turn, the decoder's two hidden layers recomputed with bf16
    operands.  The margin models HALF a unit in every input, signs independent; a whole unit in one input k moves a
    first-layer pre-activation by at most 2^-7 |W[j, k] a[k]| <= 2 margin[b, j], so a first-layer unit that changes sides
    lies within twice its margin -- asserted.  The second layer sees the first layer's changes summed, for which no such
    line holds; measured, 90 % and more of all the units that change sides lie inside their margin (D4 767 of 822, DW2 7106
    of 7212) and none beyond 2.8 x; asserted: most inside, none beyond 4 x.  So with ReLU, as with LeakyReLU in W5, a
    perturbation of the size the margin models flips units next to zero only, and the margin is not a LeakyReLU figure."""
    cd, fm, c = G.data(cid), G.flip_model(cid), G.CASES[cid]
    bf = lambda t: t.to(torch.bfloat16).float()
    flips = inside = 0
    for m in range(len(c.dims)):
        p = f"decoder_list.{m}."
        a0 = fm[p + "fc1.weight"].a.float()
        for k in [None] + list(range(c.Z)):
            a = a0.clone()
            if k is not None:
                nz = a[:, k] != 0
                a[nz, k] += 2.0 ** (torch.floor(torch.log2(a[nz, k].abs())) - 7)
            h = a
            for layer in ("fc1", "fc2"):
                f = fm[p + layer + ".weight"]
                pre = bf(h) @ bf(cd.P[p + layer + ".weight"]).T + cd.P[p + layer + ".bias"]
                changed = (pre >= 0) != (f.pre >= 0)
                ratio = (f.pre.abs() / f.margin)[changed]
                if k is None:
                    assert not bool(changed.any())                                  # (the restatement is the oracle's)
                elif ratio.numel():
                    assert float(ratio.max()) < (2.0 if layer == "fc1" else 4.0), (cid, m, k, layer, float(ratio.max()))
                    flips += ratio.numel()
                    inside += int((ratio < 1.0).sum())
                h = torch.relu(pre)
    print(f"[grad check] {cid}: {flips} units change sides over all one-unit moves, {inside} inside their margin")
    assert inside >= 0.85 * flips
