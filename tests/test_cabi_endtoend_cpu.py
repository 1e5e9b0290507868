"""CPU-side checks of the end-to-end evaluation pass' entry points (nm_e2e_pass, nm_e2e_pass_ok): they are exported, the
library's truth table on host descriptors, the statuses the launch decides on the host, and Job.e2e_ok() -- which asks the
library about the job's shape descriptor -- agrees with the predicate over the same grid.  No compute calls: there is no
GPU here."""
import ctypes as C

import pytest

import multi_modal_normative_modeling_amd as nm
from multi_modal_normative_modeling_amd import _lib
from multi_modal_normative_modeling_amd.engine import Job, JobSet
from multi_modal_normative_modeling_amd.layout import ParamLayout


@pytest.fixture(scope="module")
def lib():
    if not _lib.LIB_PATH.exists():
        import __graft_entry__ as ge
        ge.build()
    return _lib.load()


def _probe(Me=3, M=None, L=2, Z=64, C_=29, H=(110, 110), D=379, cls=(128, 64, 32), classes=2):
    """A host descriptor of the config-5 shape: 3 x 379 ROI, H [110, 110], Z 64, C 29, classifier [128, 64, 32]."""
    j = _lib.NmJob()
    j.M_enc, j.M = Me, (2 * Me if M is None else M)
    j.L, j.Z, j.C = L, Z, C_
    for i, h in enumerate(H):
        j.H[i] = h
    for m in range(min(j.M, _lib.NM_MAX_MOD)):
        j.mod[m].D = D
        j.mod[m].Kx = (D + C_ + 1 + 31) // 32 * 32
        j.mod[m].x_pitch = (D + 3) // 4 * 4
        j.mod[m].Cz = (C_ + 1 + 7) // 8 * 8
    j.n_rows, j.loss_cap, j.eps_cap = 256, 1, 1
    j.wsh = 4096
    j.w_off, j.single_bypass = -1, 0
    j.cls_layers, j.cls_classes = len(cls), classes
    for i, w in enumerate(cls[: _lib.NM_MAX_CLS]):
        j.cls_width[i] = w
    return j


def test_symbols_are_exported(lib):
    for sym in ("nm_e2e_pass", "nm_e2e_pass_ok", "nm_e2e_alpha_ok"):
        assert sym in _lib.EXPORTED_SYMBOLS
        assert hasattr(lib, sym), sym
    assert C.sizeof(_lib.NmE2e) == 16 and _lib.NM_E2E_ROW_COLUMNS == 8


def test_predicate_admits(lib):
    assert lib.nm_e2e_pass_ok(C.byref(_probe())) == 0                          # config 5
    for Z in (1, 33, 64):
        assert lib.nm_e2e_pass_ok(C.byref(_probe(Z=Z, C_=63))) == 0, Z         # Z + C = 127 at Z = 64
    for Me in (1, 2, 4):
        assert lib.nm_e2e_pass_ok(C.byref(_probe(Me=Me))) == 0, Me
    for cls in ((), (1,), (128,), (128, 128, 128, 128, 128)):
        assert lib.nm_e2e_pass_ok(C.byref(_probe(cls=cls))) == 0, cls
    for classes in (2, 3, 4):
        assert lib.nm_e2e_pass_ok(C.byref(_probe(classes=classes))) == 0, classes
    assert lib.nm_e2e_pass_ok(C.byref(_probe(H=(112, 110)))) == 0               # the first-layer stage's limit


def test_predicate_refuses(lib):
    bad = _probe()
    bad.wide = 1
    assert lib.nm_e2e_pass_ok(C.byref(bad)) == _lib.NM_E_DEVPASS
    assert lib.nm_e2e_pass_ok(C.byref(_probe(Me=3, M=3))) == _lib.NM_E_DEVPASS   # M != 2 M_enc
    assert lib.nm_e2e_pass_ok(C.byref(_probe(Me=3, M=5))) == _lib.NM_E_DEVPASS
    assert lib.nm_e2e_pass_ok(C.byref(_probe(Me=0, M=3))) == _lib.NM_E_DEVPASS   # M_enc = 0: "every modality has an encoder"
    assert lib.nm_e2e_pass_ok(C.byref(_probe(Me=5, M=10))) == _lib.NM_E_DEVPASS
    assert lib.nm_e2e_pass_ok(C.byref(_probe(cls=(129, 64)))) == _lib.NM_E_DEVPASS        # a tiled block
    assert lib.nm_e2e_pass_ok(C.byref(_probe(cls=(256, 128)))) == _lib.NM_E_DEVPASS
    six = _probe(cls=(32, 32, 32, 32, 32))
    six.cls_layers = 6
    assert lib.nm_e2e_pass_ok(C.byref(six)) == _lib.NM_E_DEVPASS
    assert lib.nm_e2e_pass_ok(C.byref(_probe(Z=64, C_=64))) == _lib.NM_E_DEVPASS          # Z + C = 128
    assert lib.nm_e2e_pass_ok(C.byref(_probe(Z=65, C_=3))) == _lib.NM_E_DEVPASS
    assert lib.nm_e2e_pass_ok(C.byref(_probe(Z=0))) == _lib.NM_E_DEVPASS
    assert lib.nm_e2e_pass_ok(C.byref(_probe(H=(113, 110)))) == _lib.NM_E_DEVPASS
    for classes in (0, 1, 5):
        assert lib.nm_e2e_pass_ok(C.byref(_probe(classes=classes))) == _lib.NM_E_DEVPASS, classes
    for field, val in (("n_private", 1), ("out_kind", 1), ("tc_weight", 1e-4), ("w_off", 0)):
        bad = _probe()
        setattr(bad, field, val)
        assert lib.nm_e2e_pass_ok(C.byref(bad)) == _lib.NM_E_DEVPASS, field
    gp = _probe()                                   # gPoE without alpha offsets (the end-to-end class registers none)
    gp.combine = _lib.NM_COMBINE["gpoe"]
    assert lib.nm_e2e_pass_ok(C.byref(gp)) == 0     # (_probe's offsets are 0: present)
    assert lib.nm_e2e_alpha_ok(C.byref(gp)) == 0
    gp.mod[1].alpha = -1
    assert lib.nm_e2e_pass_ok(C.byref(gp)) == _lib.NM_E_DEVPASS
    assert lib.nm_e2e_alpha_ok(C.byref(gp)) == _lib.NM_E_OFFSETS
    gp.combine = _lib.NM_COMBINE["poe"]
    assert lib.nm_e2e_pass_ok(C.byref(gp)) == 0 and lib.nm_e2e_alpha_ok(C.byref(gp)) == 0
    assert lib.nm_e2e_alpha_ok(None) == _lib.NM_E_NULL
    assert lib.nm_e2e_pass_ok(None) == _lib.NM_E_NULL
    # the siblings keep their own answers: they refuse the end-to-end model
    assert lib.nm_devpass_multi_ok(C.byref(_probe())) == _lib.NM_E_DEVPASS
    assert lib.nm_latent_pass_ok(C.byref(_probe())) == _lib.NM_E_DEVPASS


def test_launch_status_is_decided_on_the_host(lib):
    """NM_E_NULL / NM_E_GEOMETRY come back before the device is asked anything (there is none here)."""
    assert lib.nm_e2e_pass(None, 1, 4096, 0, 1, 0, None) == _lib.NM_E_NULL
    assert lib.nm_e2e_pass(4096, 1, None, 0, 1, 0, None) == _lib.NM_E_NULL
    for n_jobs, tile0, n_tiles in ((0, 0, 1), (1, 0, 0), (1, -1, 1), (-3, 0, 2)):
        assert lib.nm_e2e_pass(4096, n_jobs, 4096, tile0, n_tiles, 0, None) == _lib.NM_E_GEOMETRY, (n_jobs, tile0, n_tiles)


def _bare_job(spec, tc_weight=0.0, combine="poe"):
    """A Job with the fields its shape descriptor is filled from and no device behind it (Job() itself packs tables on the GPU)."""
    j = object.__new__(Job)
    j.spec, j.layout = spec, ParamLayout(spec)
    j.kmods = spec.kernel_modalities()
    j.var_floor, j.tc_weight = 0.0, tc_weight
    j.combine, j.single_bypass = combine, False
    return j


GRID = [
    ([379, 379, 379], [110, 110], 64, 29, "endtoend", (128, 64, 32), 2, True),        # config 5
    ([379, 379, 379], [110, 110], 10, 29, "endtoend", (128, 64, 32), 2, True),
    ([17, 23, 29], [40, 32], 1, 63, "endtoend", (1,), 2, True),
    ([17, 23, 29], [40, 32], 33, 63, "endtoend", (32,), 4, True),
    ([17, 23, 29], [40, 32], 64, 63, "endtoend", (128, 128, 128, 128, 128), 3, True),   # Z + C = 127
    ([65], [112], 16, 3, "endtoend", (32, 16), 2, True),
    ([17, 23, 29, 130], [40, 32], 17, 3, "endtoend", (32, 16), 2, True),
    ([17, 23, 29], [40, 32], 16, 3, "endtoend", (256, 128), 2, False),                 # a tiled classifier
    ([17, 23, 29], [40, 32], 16, 3, "endtoend", (129,), 2, False),
    ([17, 23, 29], [113, 32], 16, 3, "endtoend", (32,), 2, False),                     # first hidden layer beyond the stage
    ([17, 23, 29], [300, 160], 16, 3, "endtoend", (32,), 2, False),                    # general-shape trunk
    ([17, 23, 29], [40, 32], 16, 3, "endtoend", (), 2, False),                         # no classifier at all
    ([17, 23, 29], [40, 32], 16, 3, "multimodal", (), 2, False),                       # not the end-to-end model
    ([17, 23, 29], [40, 32], 16, 3, "regression", (), 2, False),
]


@pytest.mark.parametrize("dims,hidden,Z,cdim,kind,layers,classes,want", GRID)
def test_job_e2e_ok_is_the_library_predicate(lib, dims, hidden, Z, cdim, kind, layers, classes, want):
    spec = nm.ModelSpec(list(dims), list(hidden), Z, cdim, True, kind, tuple(layers), classes)
    job = _bare_job(spec)
    assert (lib.nm_e2e_pass_ok(C.byref(job._shape_struct())) == 0) == want
    assert job.e2e_ok() == want
    js = object.__new__(JobSet)
    js.jobs, js.wide = [job, job], bool(spec.wide)
    assert js.e2e_ok() == want


def test_gpoe_without_alpha_is_refused_on_both_sides(lib):
    spec = nm.ModelSpec([17, 23, 29], [40, 32], 16, 3, True, "endtoend", (32, 16), 2)
    for combine, want in (("poe", True), ("moe", True), ("mopoe", True), ("gpoe", False)):
        job = _bare_job(spec, combine=combine)
        assert (lib.nm_e2e_pass_ok(C.byref(job._shape_struct())) == 0) == want, combine
        assert job.e2e_ok() == want, combine
    job = _bare_job(spec)                           # the answer follows the attributes the descriptor carries, not a first call
    assert job.e2e_ok()
    job.combine = "gpoe"
    assert not job.e2e_ok()
    job.combine, job.tc_weight = "poe", 3e-4
    assert not job.e2e_ok()
    job.tc_weight = 0.0
    assert job.e2e_ok()


def test_jobset_switch_and_auto_table(lib, monkeypatch):
    spec = nm.ModelSpec([17, 23, 29], [40, 32], 16, 3, True, "endtoend", (32, 16), 2)
    js = object.__new__(JobSet)
    js.jobs, js.wide = [_bare_job(spec)], False
    monkeypatch.delenv("NMHIP_E2E", raising=False)
    assert js.e2e_ok()
    assert js.e2e_pick() == nm.engine.E2E_AUTO[3]
    monkeypatch.setenv("NMHIP_E2E", "1")
    assert js.e2e_pick()
    monkeypatch.setenv("NMHIP_E2E", "0")
    assert not js.e2e_ok() and not js.e2e_pick()
    assert set(nm.engine.E2E_AUTO) == {1, 2, 3, 4}
