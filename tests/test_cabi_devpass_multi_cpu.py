"""CPU-side checks of the multi-expert deviation-pass entry points (nm_devpass_multi, nm_devpass_multi_ok): they are
exported, the library's truth table on host descriptors, and Job.devpass_multi_ok() -- the copy of those conditions the
launch path reads off the jobs -- agrees with the library.  No compute calls: there is no GPU here."""
import ctypes as C

import pytest
import torch

import multi_modal_normative_modeling_amd as nm
from multi_modal_normative_modeling_amd import _lib
from multi_modal_normative_modeling_amd.engine import Job, JobSet


@pytest.fixture(scope="module")
def lib():
    if not _lib.LIB_PATH.exists():
        import __graft_entry__ as ge
        ge.build()
    return _lib.load()


def _probe(M=3, L=2, Z=10, C_=29, H=(110, 110), D=379):
    """A host descriptor nm_devpass_multi_ok accepts (the pattern of tests/test_cabi_cpu.py: _probe)."""
    j = _lib.NmJob()
    j.M, j.L, j.Z, j.C = M, L, Z, C_
    for i, h in enumerate(H):
        j.H[i] = h
    for m in range(min(M, _lib.NM_MAX_MOD)):
        j.mod[m].D = D
        j.mod[m].Kx = (D + C_ + 1 + 31) // 32 * 32
        j.mod[m].x_pitch = (D + 3) // 4 * 4
        j.mod[m].Cz = (C_ + 1 + 7) // 8 * 8
    j.n_rows, j.loss_cap, j.eps_cap = 256, 1, 1
    j.n_params = 118479
    j.wsh = 4096
    j.w_off, j.single_bypass = -1, 1
    return j


def test_symbols_are_exported(lib):
    for sym in ("nm_devpass_multi", "nm_devpass_multi_ok"):
        assert sym in _lib.EXPORTED_SYMBOLS
        assert hasattr(lib, sym), sym


def test_devpass_multi_ok_truth_table(lib):
    for M in (2, 3, 4):
        for bypass in (0, 1):
            ok = _probe(M=M)
            ok.single_bypass = bypass
            assert lib.nm_devpass_multi_ok(C.byref(ok)) == 0, (M, bypass)
            ok.M_enc = M                                              # (M_enc = M says the same as M_enc = 0)
            assert lib.nm_devpass_multi_ok(C.byref(ok)) == 0, (M, bypass)
    # the limits themselves are accepted: first hidden width 112, latent 32
    assert lib.nm_devpass_multi_ok(C.byref(_probe(H=(112, 110), Z=32))) == 0
    assert lib.nm_devpass_multi_ok(C.byref(_probe(M=1))) == _lib.NM_E_DEVPASS
    assert lib.nm_devpass_multi_ok(C.byref(_probe(M=5))) == _lib.NM_E_DEVPASS
    for field, val in (("M_enc", 2), ("n_private", 1), ("tc_weight", 1e-4), ("w_off", 0), ("out_kind", 1), ("wide", 1), ("Z", 33)):
        bad = _probe(M=3)
        setattr(bad, field, val)
        assert lib.nm_devpass_multi_ok(C.byref(bad)) == _lib.NM_E_DEVPASS, field
    assert lib.nm_devpass_multi_ok(C.byref(_probe(H=(113, 110)))) == _lib.NM_E_DEVPASS
    assert lib.nm_devpass_multi_ok(None) == _lib.NM_E_NULL
    # the one-expert entry point keeps its own answers: it refuses what this one accepts
    assert lib.nm_devpass_ok(C.byref(_probe(M=3))) == _lib.NM_E_DEVPASS


def _bare_job(spec, combine="gpoe", latent_exports=False, tc_weight=0.0):
    """A Job with the fields devpass_multi_ok() reads and no device behind it (Job() itself packs tables on the GPU)."""
    j = object.__new__(Job)
    j.spec = spec
    j.kmods = spec.kernel_modalities()
    j.combine = combine
    j.single_bypass = True
    j.tc_weight = tc_weight
    j.out_mu = j.out_logvar = j.out_z = torch.zeros(1) if latent_exports else None
    return j


def _descriptor(job):
    """The fields of job.struct() that nm_devpass_multi_ok reads, filled as Job.struct() fills them."""
    s, d = job.spec, _lib.NmJob()
    d.M, d.M_enc, d.C, d.L, d.Z = len(job.kmods), s.M, s.net_c_dim, len(s.hidden), s.latent
    for i, h in enumerate(s.hidden):
        d.H[i] = h
    d.out_kind = 1 if s.is_dm else 0
    d.n_private = s.n_private
    d.w_off = 0 if s.kind == "weighted_dmvae" else -1
    d.tc_weight = job.tc_weight
    d.wide = int(s.wide)
    d.single_bypass = 1
    return d


@pytest.mark.parametrize("dims,hidden,Z,kind,want", [
    ([379, 379], [110, 110], 10, "multimodal", True),
    ([379, 379, 379], [110, 110], 10, "multimodal", True),
    ([379, 379, 379, 1137], [110, 110], 10, "multimodal", True),
    ([40, 40, 40, 120], [112], 32, "multimodal", True),
    ([379], [110, 110], 10, "multimodal", False),                 # one expert: nm_devpass serves it
    ([61, 90, 47], [120, 48], 12, "multimodal", False),           # first hidden layer too wide for the first-layer stage
    ([61, 90, 47], [113, 48], 12, "multimodal", False),
    ([61, 90, 47], [64, 48], 40, "multimodal", False),            # latent beyond two 16-column tiles
    ([61, 90, 47], [64, 48], 33, "multimodal", False),
    ([61, 90, 47], [64, 48], 12, "dmvae", False),                 # private latent, sigmoid output
    ([61, 90, 47], [64, 48], 12, "weighted_dmvae", False),        # learnable loss weights
    ([61, 90, 47], [64, 48], 12, "endtoend", False),              # decoder-only modalities (second decoder bank)
    ([61, 90, 47], [300, 300], 12, "multimodal", False),          # general-shape path
])
def test_job_check_agrees_with_library(lib, dims, hidden, Z, kind, want):
    spec = nm.ModelSpec(list(dims), list(hidden), Z, 3, True, kind)
    job = _bare_job(spec)
    assert job.devpass_multi_ok() == want
    assert (lib.nm_devpass_multi_ok(C.byref(_descriptor(job))) == 0) == want


def test_job_check_extra_conditions(lib, monkeypatch):
    """What the host check adds to the library's: latent exports asked for, total correlation (mvtCAE), NMHIP_DEVPASS=0."""
    spec = nm.ModelSpec([61, 90, 47], [64, 48], 12, 3, True, "multimodal")
    assert _bare_job(spec).devpass_multi_ok()
    assert not _bare_job(spec, latent_exports=True).devpass_multi_ok()
    tc = _bare_job(nm.ModelSpec([61, 90, 47], [64, 48], 12, 3, True, "mvtcae"), tc_weight=3e-4)
    assert not tc.devpass_multi_ok()
    assert lib.nm_devpass_multi_ok(C.byref(_descriptor(tc))) == _lib.NM_E_DEVPASS
    js = object.__new__(JobSet)
    js.jobs, js.wide = [_bare_job(spec), _bare_job(spec)], False
    monkeypatch.delenv("NMHIP_DEVPASS", raising=False)
    assert js.devpass_multi_ok()
    assert not js.devpass_ok()                                      # (several experts: not the one-expert kernel's)
    monkeypatch.setenv("NMHIP_DEVPASS", "0")
    assert not js.devpass_multi_ok()
    monkeypatch.delenv("NMHIP_DEVPASS")
    js.jobs.append(_bare_job(spec, latent_exports=True))
    assert not js.devpass_multi_ok()
