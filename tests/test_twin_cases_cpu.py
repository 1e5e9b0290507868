"""The twin fuzz's draw (tests/twin_cases.py) is honest -- no GPU here.  Every seed of every twin and every FIXED case is
admitted by the predicate it targets, on the Python side (a bare Job, as tests/test_plain_cabi_cpu.py: _bare_job) and on the C
side (a host descriptor filled as Job.struct() fills it: nm_validate_job and the matching nm_*_ok), so the GPU test leaves out
no case; over a twin's seeds plus FIXED every edge value the twin admits occurs in each of D, a hidden width, Z and N, and
every M, combiner, switch and training knob value occurs; the draw is a pure function of (twin, seed); assert_same bites."""
import ctypes as C

import pytest
import torch

import multi_modal_normative_modeling_amd as nm
from multi_modal_normative_modeling_amd import _lib
from multi_modal_normative_modeling_amd.engine import Job
from tests import twin_cases as T


@pytest.fixture(scope="module")
def lib():
    if not _lib.LIB_PATH.exists():
        import __graft_entry__ as ge
        ge.build()
    return _lib.load()


def _spec(cs):
    return nm.ModelSpec(list(cs.dims), list(cs.hidden), cs.Z, cs.c_dim, cs.non_linear, cs.kind)


def _exports(cs):
    """Which export buffers the twin's jobs carry (tests/test_gpu_twins.py): (per-modality exports, latent exports)."""
    return cs.twin in ("devpass", "devpass_multi"), cs.twin == "latent"


def _bare_job(cs):
    """A Job with the fields the *_ok() checks read and no device behind it (Job() itself packs tables on the GPU)."""
    j = object.__new__(Job)
    j.spec = _spec(cs)
    j.kmods = j.spec.kernel_modalities()
    nk = len(j.kmods)
    j.combine, j.single_bypass, j.tc_weight = cs.combine, cs.single_bypass, 0.0
    per_mod, latent = _exports(cs)
    t = torch.zeros(1)
    j.out_mu = j.out_logvar = j.out_z = t if latent else None
    j.out_loc, j.out_sqerr, j.out_rowdev = ([t if per_mod else None] * nk for _ in range(3))
    j.dz_extra = None
    j.dloc_extra, j.dloc_rowcoef = [None] * nk, [None] * nk
    return j


def _descriptor(lib, cs):
    """The host descriptor of the case's job, filled as Job.struct() and Table fill it (any non-null address for a buffer)."""
    s, d, p = _spec(cs), _lib.NmJob(), 4096
    layout = nm.ParamLayout(s)
    kmods = s.kernel_modalities()
    d.M, d.M_enc, d.C, d.L, d.Z = len(kmods), s.M, s.net_c_dim, len(s.hidden), s.latent
    d.act_slope, d.out_kind, d.n_private, d.w_off = 0.01, 0, s.n_private, -1
    for i, h in enumerate(s.hidden):
        d.H[i] = h
    d.combine = _lib.NM_COMBINE[cs.combine]
    d.single_bypass, d.n_rows, d.non_linear = int(cs.single_bypass), cs.N, int(s.non_linear)
    d.shared_cov, d.wide = int(cs.shared_cov or cs.M == 1), int(s.wide)
    d.loss_cap, d.eps_cap = 8, (3 if cs.inject else 1)
    d.lr, d.beta1, d.beta2, d.adam_eps = cs.lr, cs.betas[0], cs.betas[1], cs.adam_eps
    d.lr_table, d.lr_cap = (p, len(cs.lr_table)) if cs.lr_table else (None, 0)
    d.kl_weight, d.ll_weight = float(s.M if cs.kl_weight is None else cs.kl_weight), cs.ll_weight
    d.params = d.adam_m = d.adam_v = d.grads = d.loss_log = d.workspace = d.wsh = p
    d.eps = p if cs.inject else None
    d.seed, d.n_params = cs.job_seed, layout.total
    d.gpart_stride = (layout.total + 255) // 256 * 256
    per_mod, latent = _exports(cs)
    d.out_mu = d.out_logvar = d.out_z = p if latent else None
    layout.fill_head(d)
    if d.reg_head:
        d.reg_resid = d.reg_dres = p
    for k, (m, _, _) in enumerate(kmods):
        md, D = d.mod[k], s.input_dims[m]
        md.D, md.Kx, md.x_pitch, md.Cz = D, (D + s.net_c_dim + 1 + 31) // 32 * 32, (D + 3) // 4 * 4, (s.net_c_dim + 1 + 7) // 8 * 8
        md.x_f32 = md.xb = md.cz = p
        layout.fill_modality(md, k)
        md.out_loc = md.out_sqerr = md.out_rowdev = p if per_mod else None
    assert lib.nm_fill_shadow(C.byref(d)) > 0
    return d


ALL = [cs for twin in T.TWINS for cs in T.cases(twin)]


def test_seed_lists_and_fixed_cases():
    assert {t: len(T.SEEDS[t]) for t in T.TWINS} == {"plain": 32, "devpass": 16, "devpass_multi": 24, "latent": 24, "split": 16}
    assert len({cs.id for cs in ALL}) == len(ALL)
    fixed = {t: {cs.name: cs for cs in T.FIXED[t]} for t in T.TWINS}
    for t in ("plain", "devpass"):
        assert fixed[t]["early_fusion_1137"].dims == (1137,)
    for t in ("plain", "devpass_multi"):
        assert fixed[t]["uca"].dims == (379, 379, 379, 1137)
    for t in T.TWINS:
        sm = fixed[t]["smallest"]
        assert sm.dims == (3,) * T.M_RANGE[t][0] and sm.hidden == (8,) and (sm.Z, sm.N, sm.c_dim) == (1, 1, 3)
        assert all(cs.twin == t for cs in T.cases(t))


@pytest.mark.parametrize("cs", ALL, ids=lambda cs: cs.id)
def test_no_draw_is_refused(lib, cs):
    """The share of cases the GPU test may leave out is zero: the Job's own check and the library's both admit the case."""
    s = _spec(cs)
    s.validate()
    assert not s.wide and cs.Z + cs.c_dim <= _lib.NM_MAX_WIDTH and cs.M in T.M_RANGE[cs.twin]
    assert cs.kind in T.kinds(cs.twin, cs.M)
    job, d = _bare_job(cs), _descriptor(lib, cs)
    assert lib.nm_validate_job(C.byref(d)) == 0
    if cs.twin == "plain":
        assert job.plain_ok() and lib.nm_plain_ok(C.byref(d)) == 0
    elif cs.twin == "devpass":
        assert job.devpass_ok() and lib.nm_devpass_ok(C.byref(d)) == 0
    elif cs.twin == "devpass_multi":
        assert job.devpass_multi_ok() and not job.devpass_ok() and lib.nm_devpass_multi_ok(C.byref(d)) == 0
    elif cs.twin == "latent":
        assert job.latent_ok() and lib.nm_latent_pass_ok(C.byref(d)) == 0
    else:
        # the split launch has no predicate of its own beyond JobSet.split_parts: several kernel modalities, every one a
        # workgroup, all resident at once (a set of one model is padded to 8: 8 M workgroups on 256 CUs); its reference
        # is the generic kernel, so the job must not need anything else either
        assert 2 <= len(job.kmods) == cs.M <= _lib.NM_MAX_MOD and 8 * cs.M <= 256
        assert job.plain_ok() and lib.nm_plain_ok(C.byref(d)) == 0


@pytest.mark.parametrize("cs", ALL, ids=lambda cs: cs.id)
def test_case_is_inside_the_admitted_domain(cs):
    big = cs.name in ("early_fusion_1137", "uca")
    assert all(T.D_RANGE[0] <= d <= (1137 if big else T.D_RANGE[1]) for d in cs.dims)
    assert 1 <= len(cs.hidden) <= 3 and all(T.H_RANGE[0] <= h <= T.H_RANGE[1] for h in cs.hidden)
    assert 1 <= cs.Z <= T.Z_MAX and T.C_RANGE[0] <= cs.c_dim <= T.C_RANGE[1] and cs.Z + cs.c_dim <= 127
    assert T.N_RANGE[0] <= cs.N <= T.N_RANGE[1]
    if cs.twin in T.COMPACT_FORWARD:
        assert cs.hidden[0] <= 112 and (cs.Z + 15) // 16 * 16 <= 32
    if cs.twin == "devpass" or cs.M > 1:
        assert cs.single_bypass
    a, b = cs.steps
    assert a >= 1 and b >= 1 and 3 <= a + b <= 6
    if cs.lr_table is not None:
        assert len(cs.lr_table) in (3, 7) and (a + b) % len(cs.lr_table) != 0 and all(v > 0 for v in cs.lr_table)
    if cs.twin in T.TRAINING and cs.N > 512:
        assert a + b >= 4                                           # three batches per epoch: the wrap is crossed


@pytest.mark.parametrize("twin", T.TWINS)
def test_coverage(twin):
    cs = T.cases(twin)
    assert {d for c in cs for d in c.dims} >= set(T.D_EDGES)
    assert {h for c in cs for h in c.hidden} >= set(T.H_EDGES)
    assert {c.Z for c in cs} >= set(T.z_edges(twin))
    assert {c.N for c in cs} >= set(T.N_EDGES)
    assert {c.M for c in cs} == set(T.M_RANGE[twin])
    assert {c.combine for c in cs} == set(T.COMBINERS)
    assert {len(c.hidden) for c in cs} == {1, 2, 3}
    for field in ("non_linear", "shared_cov", "inject"):
        assert {getattr(c, field) for c in cs} == {True, False}, field
    assert {c.kind for c in cs} == {k for m in T.M_RANGE[twin] for k in T.kinds(twin, m)}
    if twin in ("plain", "latent"):                                 # the bypass is drawn where a one-expert model admits it off
        assert {c.single_bypass for c in cs if c.M == 1} == {True, False}
    if twin in T.COMPACT_FORWARD:                                   # ... the widths beyond the first-layer stage behind it
        assert {h for c in cs for h in c.hidden[1:]} >= {113, 126, 127}
    # Z + c_dim + 1 on a whole k tile and one past it (128 is out of reach: Z <= 64, c_dim <= 29)
    assert {c.Z + c.c_dim + 1 for c in cs} & {16, 17, 32, 33}
    if twin in T.TRAINING:
        assert {c.lr for c in cs} == set(T.LRS)
        assert {c.betas for c in cs} == set(T.BETAS)
        assert {c.adam_eps for c in cs} == set(T.ADAM_EPS)
        assert {c.kl_weight for c in cs} == set(T.KL_WEIGHTS)
        assert {c.ll_weight for c in cs} == set(T.LL_WEIGHTS)
        assert {len(c.lr_table) if c.lr_table else 0 for c in cs} == set(T.LR_TABLE_LENS)
        assert {sum(c.steps) for c in cs} == set(T.STEP_TOTALS)
        assert any(c.N > 256 and sum(c.steps) > (c.N + 255) // 256 for c in cs)      # a ragged batch and the epoch wrap


def test_draw_is_deterministic_and_seeds_differ():
    for twin in T.TWINS:
        drawn = [T.draw(twin, s) for s in T.SEEDS[twin]]
        assert drawn == [T.draw(twin, s) for s in T.SEEDS[twin]]
        assert len(set(drawn)) == len(drawn)
        assert len({(c.dims, c.hidden, c.Z, c.c_dim, c.N) for c in drawn}) == len(drawn)
    assert T.draw("plain", 5) != T.draw("split", 5)
    with pytest.raises(ValueError):
        T.draw("rowsplit", 0)


def test_assert_same_bites():
    g = torch.Generator().manual_seed(3)
    a = {"params": torch.randn(300, generator=g), "adam_v": torch.randn(7, 40, generator=g).abs(),
         "wsh": torch.randint(0, 256, (64,), generator=g, dtype=torch.uint8)}
    b = {k: v.clone() for k, v in a.items()}
    T.assert_same(a, b, "exact copy")
    b["adam_v"].view(-1).view(torch.int32)[133] ^= 1                # the last mantissa bit of one element of one tensor
    with pytest.raises(AssertionError) as e:
        T.assert_same(a, b, "one ulp")
    msg = str(e.value)
    want, got = a["adam_v"].view(-1)[133:134].view(torch.int32).item(), b["adam_v"].view(-1)[133:134].view(torch.int32).item()
    assert "one ulp" in msg and "adam_v" in msg and "1 of 280" in msg and "index 133" in msg
    assert f"0x{want:08x}" in msg and f"0x{got:08x}" in msg and "params" not in msg
    b = {k: v.clone() for k, v in a.items()}
    b["wsh"][9] ^= 0x10                                              # a byte of a bf16 shadow image
    with pytest.raises(AssertionError, match=r"wsh differs in 1 of 64 elements; first at flat index 9"):
        T.assert_same(a, b, "shadow")
