"""CPU-side checks of the latent-deviation entry points (nm_latent_pass, nm_latent_pass_ok, nm_latent_stats,
nm_latent_score): they are exported, the library's truth table on host descriptors, Job.latent_ok() -- the copy of those
conditions the launch path reads off the jobs -- agrees with the library, NMHIP_LATENT=0 switches the pick off, and the two
small kernels' entry points return their argument errors before they touch a device.  No compute calls: no GPU here."""
import ctypes as C

import pytest

import multi_modal_normative_modeling_amd as nm
from multi_modal_normative_modeling_amd import _lib
from multi_modal_normative_modeling_amd.engine import JobSet
from tests.test_cabi_devpass_multi_cpu import _bare_job, _descriptor, _probe


@pytest.fixture(scope="module")
def lib():
    if not _lib.LIB_PATH.exists():
        import __graft_entry__ as ge
        ge.build()
    return _lib.load()


def test_symbols_are_exported(lib):
    for sym in ("nm_latent_pass", "nm_latent_pass_ok", "nm_latent_stats", "nm_latent_score"):
        assert sym in _lib.EXPORTED_SYMBOLS
        assert hasattr(lib, sym), sym


def test_latent_pass_ok_truth_table(lib):
    for M in (1, 2, 3, 4):
        for bypass in (0, 1):
            ok = _probe(M=M)
            ok.single_bypass = bypass
            assert lib.nm_latent_pass_ok(C.byref(ok)) == 0, (M, bypass)
            ok.M_enc = M                                              # (M_enc = M says the same as M_enc = 0)
            assert lib.nm_latent_pass_ok(C.byref(ok)) == 0, (M, bypass)
    # the limits themselves are accepted: first hidden width 112, latent 32
    assert lib.nm_latent_pass_ok(C.byref(_probe(H=(112, 110), Z=32))) == 0
    assert lib.nm_latent_pass_ok(C.byref(_probe(M=1, H=(112, 110), Z=32))) == 0
    assert lib.nm_latent_pass_ok(C.byref(_probe(H=(113, 110)))) == _lib.NM_E_DEVPASS
    assert lib.nm_latent_pass_ok(C.byref(_probe(Z=33))) == _lib.NM_E_DEVPASS
    assert lib.nm_latent_pass_ok(C.byref(_probe(M=5))) == _lib.NM_E_DEVPASS
    assert lib.nm_latent_pass_ok(C.byref(_probe(M=0))) == _lib.NM_E_DEVPASS
    for M in (1, 3):
        for field, val in (("M_enc", M + 1), ("n_private", 1), ("tc_weight", 1e-4), ("w_off", 0), ("out_kind", 1), ("wide", 1)):
            bad = _probe(M=M)
            setattr(bad, field, val)
            assert lib.nm_latent_pass_ok(C.byref(bad)) == _lib.NM_E_DEVPASS, (M, field)
    assert lib.nm_latent_pass_ok(None) == _lib.NM_E_NULL
    # the launch itself checks its arguments before anything else
    assert lib.nm_latent_pass(None, 1, 0, 1, 0, None) == _lib.NM_E_NULL
    assert lib.nm_latent_pass(4096, 0, 0, 1, 0, None) == _lib.NM_E_GEOMETRY
    assert lib.nm_latent_pass(4096, 1, -1, 1, 0, None) == _lib.NM_E_GEOMETRY


@pytest.mark.parametrize("dims,hidden,Z,kind,want", [
    ([379, 379], [110, 110], 10, "multimodal", True),
    ([379, 379, 379], [110, 110], 10, "multimodal", True),
    ([379, 379, 379, 1137], [110, 110], 10, "multimodal", True),
    ([40, 40, 40, 120], [112], 32, "multimodal", True),
    ([379], [110, 110], 10, "multimodal", True),                  # one expert: accepted here (nm_devpass_multi refuses it)
    ([379], [110, 110], 10, "single", True),                      # ... and the cVAE class
    ([61], [64, 48], 12, "multimodal", True),
    ([61, 90, 47], [120, 48], 12, "multimodal", False),           # first hidden layer too wide for the first-layer stage
    ([61, 90, 47], [113, 48], 12, "multimodal", False),
    ([61, 90, 47], [64, 48], 40, "multimodal", False),            # latent beyond two 16-column tiles
    ([61, 90, 47], [64, 48], 33, "multimodal", False),
    ([61, 90, 47], [64, 48], 12, "dmvae", False),                 # private latent, sigmoid output
    ([61, 90, 47], [64, 48], 12, "weighted_dmvae", False),        # learnable loss weights
    ([61, 90, 47], [64, 48], 12, "endtoend", False),              # decoder-only modalities: not every modality has an encoder
    ([61, 90, 47], [300, 300], 12, "multimodal", False),          # general-shape path
    ([61, 90, 47], [64, 48], 12, "regression", True),             # (the regressor sits behind the decoders: no part of this pass)
])
def test_job_check_agrees_with_library(lib, dims, hidden, Z, kind, want):
    spec = nm.ModelSpec(list(dims), list(hidden), Z, 3, True, kind)
    job = _bare_job(spec)
    assert job.latent_ok() == want
    assert (lib.nm_latent_pass_ok(C.byref(_descriptor(job))) == 0) == want
    # the latent exports are what the pass writes: asking for them refuses nothing
    assert _bare_job(spec, latent_exports=True).latent_ok() == want


def test_total_correlation_and_the_environment_switch(lib, monkeypatch):
    tc = _bare_job(nm.ModelSpec([61, 90, 47], [64, 48], 12, 3, True, "mvtcae"), tc_weight=3e-4)
    assert not tc.latent_ok()
    assert lib.nm_latent_pass_ok(C.byref(_descriptor(tc))) == _lib.NM_E_DEVPASS
    spec = nm.ModelSpec([61, 90, 47], [64, 48], 12, 3, True, "multimodal")
    one = nm.ModelSpec([61], [64, 48], 12, 3, True, "multimodal")
    js = object.__new__(JobSet)
    js.jobs, js.wide = [_bare_job(spec), _bare_job(one)], False
    monkeypatch.delenv("NMHIP_LATENT", raising=False)
    assert js.latent_ok()
    assert js.latent_pick() == all(nm.engine.LATENT_AUTO.get(m, False) for m in (3, 1))
    monkeypatch.setenv("NMHIP_LATENT", "0")
    assert not js.latent_ok() and not js.latent_pick()
    assert "NMHIP_LATENT=0" in js._latent_refusal()
    monkeypatch.delenv("NMHIP_LATENT")
    monkeypatch.setenv("NMHIP_DEVPASS", "0")                       # (the deviation pass's switch is not this kernel's)
    assert js.latent_ok()
    monkeypatch.delenv("NMHIP_DEVPASS")
    js.jobs.append(tc)
    assert not js.latent_ok() and "job 2" in js._latent_refusal()
    js.jobs, js.wide = [_bare_job(nm.ModelSpec([61, 90, 47], [300, 300], 12, 3, True, "multimodal"))], True
    assert not js.latent_ok() and "general-shape" in js._latent_refusal()


def test_stats_and_score_argument_errors(lib):
    p = 4096                                                          # (any non-null address: the checks come first)
    for args in ((None, p, 1, 10, 10, p, p), (p, None, 1, 10, 10, p, p), (p, p, 1, 10, 10, None, p), (p, p, 1, 10, 10, p, None)):
        assert lib.nm_latent_stats(*args, None) == _lib.NM_E_NULL, args
    for Z in (0, -1, 65):
        assert lib.nm_latent_stats(p, p, 1, Z, 80, p, p, None) == _lib.NM_E_LATENT, Z
    assert lib.nm_latent_stats(p, p, 0, 10, 10, p, p, None) == _lib.NM_E_METRICS          # no set at all
    assert lib.nm_latent_stats(p, p, 1, 10, 9, p, p, None) == _lib.NM_E_METRICS           # pitch below Z
    ok = [p, p, p, 1, 10, 10, p, p, p, p]
    for i in (0, 1, 2, 6, 7):
        bad = list(ok)
        bad[i] = None
        assert lib.nm_latent_score(*bad, None) == _lib.NM_E_NULL, i
    both = list(ok)
    both[8] = both[9] = None
    assert lib.nm_latent_score(*both, None) == _lib.NM_E_NULL                             # (one output may be missing, not both)
    for Z in (0, 65):
        bad = list(ok)
        bad[4], bad[5] = Z, 80
        assert lib.nm_latent_score(*bad, None) == _lib.NM_E_LATENT, Z
    bad = list(ok)
    bad[3] = 0
    assert lib.nm_latent_score(*bad, None) == _lib.NM_E_METRICS
    bad = list(ok)
    bad[5] = 9
    assert lib.nm_latent_score(*bad, None) == _lib.NM_E_METRICS
    assert b"latent" in lib.nm_status_string(_lib.NM_E_LATENT)
