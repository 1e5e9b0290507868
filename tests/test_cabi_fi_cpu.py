"""CPU-side checks of the regression model's evaluation pass' entry points (nm_fi_pass, nm_fi_pass_ok): they are exported, the
library's truth table on host descriptors (one job per rule), the statuses the launch decides on the host, and Job.fi_ok() --
which asks the library about the job's shape descriptor -- agrees with the predicate over the same grid.  No compute calls:
there is no GPU here."""
import ctypes as C

import pytest

import multi_modal_normative_modeling_amd as nm
from multi_modal_normative_modeling_amd import _lib, metrics
from multi_modal_normative_modeling_amd.engine import Job, JobSet
from multi_modal_normative_modeling_amd.layout import ParamLayout


@pytest.fixture(scope="module")
def lib():
    if not _lib.LIB_PATH.exists():
        import __graft_entry__ as ge
        ge.build()
    return _lib.load()


def _probe(M=3, L=2, Z=10, C_=2, H=(110, 110), D=379):
    """A host descriptor of the regression script's default shape: 3 x 379 ROI, H [110, 110], Z 10, two raw covariates."""
    j = _lib.NmJob()
    j.M_enc, j.M = M, M
    j.L, j.Z, j.C = L, Z, C_
    for i, h in enumerate(H):
        j.H[i] = h
    for m in range(min(M, _lib.NM_MAX_MOD)):
        j.mod[m].D = D
        j.mod[m].Kx = (D + C_ + 1 + 31) // 32 * 32
        j.mod[m].x_pitch = (D + 3) // 4 * 4
        j.mod[m].Cz = (C_ + 1 + 7) // 8 * 8
    j.n_rows, j.loss_cap, j.eps_cap = 256, 1, 1
    j.wsh = 4096
    j.w_off, j.single_bypass = -1, 0
    j.reg_head, j.reg_s = 1, 1024
    for i in range(3):
        j.reg_w[i], j.reg_b[i] = 256 * (i + 1), 4096 + 4 * i
    return j


def test_symbols_are_exported(lib):
    for sym in ("nm_fi_pass", "nm_fi_pass_ok"):
        assert sym in _lib.EXPORTED_SYMBOLS
        assert hasattr(lib, sym), sym
    assert C.sizeof(_lib.NmFi) == 24 and _lib.NM_FI_ROW_COLUMNS == 8        # (the .inc asserts sizeof(nm_fi_t) == 24)
    assert len(metrics.FI_ROW_COLUMNS) == 8 and metrics.FI_ROW_COLUMNS[0] == "fi_pred"


def test_predicate_admits(lib):
    assert lib.nm_fi_pass_ok(C.byref(_probe())) == 0                           # the default shape
    for M in (1, 2, 3, 4):
        assert lib.nm_fi_pass_ok(C.byref(_probe(M=M))) == 0, M
    for Z in (1, 16, 17, 32):
        assert lib.nm_fi_pass_ok(C.byref(_probe(Z=Z))) == 0, Z
    assert lib.nm_fi_pass_ok(C.byref(_probe(H=(112, 110)))) == 0                # the first-layer stage's limit
    byp = _probe(M=1)
    byp.single_bypass = 1
    assert lib.nm_fi_pass_ok(C.byref(byp)) == 0
    bare = _probe()                                 # the pass writes no residual image: the buffers are not asked for
    bare.reg_resid = bare.reg_dres = None
    assert lib.nm_fi_pass_ok(C.byref(bare)) == 0
    gp = _probe()
    gp.combine = _lib.NM_COMBINE["gpoe"]            # (_probe's alpha offsets are 0: present)
    assert lib.nm_fi_pass_ok(C.byref(gp)) == 0


def _with(**fields):
    j = _probe()
    for k, v in fields.items():
        setattr(j, k, v)
    return j


def test_predicate_refuses_one_job_per_rule(lib):
    bad = {
        "wide": _with(wide=1),
        "no head": _with(reg_head=0),
        "reg_s": _with(reg_s=-1),
        "five modalities": _probe(M=5),
        "no modality": _probe(M=0),
        "a decoder without an encoder": _with(M_enc=2),
        "private latent": _with(n_private=1),
        "total correlation": _with(tc_weight=1e-4),
        "learnable weights": _with(w_off=0),
        "sigmoid output": _with(out_kind=1),
        "H[0] beyond the stage": _probe(H=(113, 110)),
        "H beyond the tile": _probe(H=(110, 129)),
        "H zero": _probe(H=(110, 0)),
        "Z 33": _probe(Z=33),
        "Z 0": _probe(Z=0),
        "a classifier": _with(cls_layers=1, cls_classes=2),
        "logits layer alone": _with(cls_classes=2),
    }
    w = _probe()
    w.reg_w[1] = -1
    bad["reg_w offset missing"] = w
    w = _probe()
    w.reg_w[0] = 128
    bad["reg_w offset unaligned"] = w
    b = _probe()
    b.reg_b[2] = -1
    bad["reg_b offset missing"] = b
    gp = _probe()
    gp.combine = _lib.NM_COMBINE["gpoe"]
    gp.mod[1].alpha = -1
    bad["gPoE without an alpha offset"] = gp
    for why, j in bad.items():
        assert lib.nm_fi_pass_ok(C.byref(j)) == _lib.NM_E_DEVPASS, why
    gp.combine = _lib.NM_COMBINE["poe"]
    assert lib.nm_fi_pass_ok(C.byref(gp)) == 0
    assert lib.nm_fi_pass_ok(None) == _lib.NM_E_NULL


def test_launch_status_is_decided_on_the_host(lib):
    """NM_E_NULL / NM_E_GEOMETRY come back before the device is asked anything (there is none here)."""
    assert lib.nm_fi_pass(None, 1, 4096, 1, 4096, 0, 1, 0, None) == _lib.NM_E_NULL
    assert lib.nm_fi_pass(4096, 1, 4096, 1, None, 0, 1, 0, None) == _lib.NM_E_NULL
    assert lib.nm_fi_pass(4096, 1, None, 2, 4096, 0, 1, 0, None) == _lib.NM_E_NULL      # a draw table is needed beyond one draw
    for n_draws in (0, -1, _lib.NM_MAX_DRAWS + 1):
        assert lib.nm_fi_pass(4096, 1, 4096, n_draws, 4096, 0, 1, 0, None) == _lib.NM_E_GEOMETRY, n_draws
        assert lib.nm_fi_pass(4096, 1, None, n_draws, 4096, 0, 1, 0, None) == _lib.NM_E_GEOMETRY, n_draws
    for n_jobs, tile0, n_tiles in ((0, 0, 1), (1, 0, 0), (1, -1, 1), (-3, 0, 2)):
        assert lib.nm_fi_pass(4096, n_jobs, 4096, 3, 4096, tile0, n_tiles, 0, None) == _lib.NM_E_GEOMETRY, (n_jobs, tile0, n_tiles)
        assert lib.nm_fi_pass(4096, n_jobs, None, 1, 4096, tile0, n_tiles, 0, None) == _lib.NM_E_GEOMETRY, (n_jobs, tile0, n_tiles)


def _bare_job(spec, tc_weight=0.0, combine="gpoe", bypass=False):
    """A Job with the fields its shape descriptor is filled from and no device behind it (Job() itself packs tables on the GPU)."""
    j = object.__new__(Job)
    j.spec, j.layout = spec, ParamLayout(spec)
    j.kmods = spec.kernel_modalities()
    j.var_floor, j.tc_weight = 0.0, tc_weight
    j.combine, j.single_bypass = combine, bypass
    return j


GRID = [
    ([379, 379, 379], [110, 110], 10, 2, "regression", True),          # the regression script's default
    ([17, 23, 29], [40, 32], 1, 2, "regression", True),
    ([65, 130], [24], 16, 3, "regression", True),
    ([17], [112], 1, 2, "regression", True),
    ([17, 23, 29, 65], [40, 32], 17, 4, "regression", True),
    ([64, 128], [32], 32, 5, "regression", True),
    ([17, 23, 29], [40, 32], 33, 5, "regression", False),              # latent above 32
    ([17, 23, 29], [113, 32], 16, 3, "regression", False),             # first hidden layer beyond the stage
    ([17, 23, 29], [256], 16, 3, "regression", False),                 # general-shape trunk
    ([17, 23, 29], [40, 32], 16, 3, "multimodal", False),              # no head
    ([17, 23, 29], [40, 32], 16, 3, "endtoend", False),
]


@pytest.mark.parametrize("dims,hidden,Z,cdim,kind,want", GRID)
def test_job_fi_ok_is_the_library_predicate(lib, dims, hidden, Z, cdim, kind, want):
    spec = nm.ModelSpec(list(dims), list(hidden), Z, cdim, True, kind, (32, 16) if kind == "endtoend" else (), 2)
    for combine in ("gpoe", "poe"):
        job = _bare_job(spec, combine=combine)
        assert (lib.nm_fi_pass_ok(C.byref(job._shape_struct())) == 0) == want
        assert job.fi_ok() == want
        js = object.__new__(JobSet)
        js.jobs, js.wide = [job, job], bool(spec.wide)
        assert js.fi_ok() == want
    job = _bare_job(spec)                           # the answer follows the attributes the descriptor carries, not a first call
    job.tc_weight = 3e-4
    assert not job.fi_ok()
    job.tc_weight = 0.0
    assert job.fi_ok() == want


def test_jobset_switch_and_auto_table(lib, monkeypatch):
    spec = nm.ModelSpec([17, 23, 29], [40, 32], 10, 2, True, "regression")
    js = object.__new__(JobSet)
    js.jobs, js.wide = [_bare_job(spec)], False
    monkeypatch.delenv("NMHIP_FI", raising=False)
    assert js.fi_ok()
    assert js.fi_pick() == nm.engine.FI_AUTO[3]
    monkeypatch.setenv("NMHIP_FI", "1")
    assert js.fi_pick()
    monkeypatch.setenv("NMHIP_FI", "0")
    assert not js.fi_ok() and not js.fi_pick()
    assert set(nm.engine.FI_AUTO) == {1, 2, 3, 4}
