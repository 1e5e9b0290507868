"""CPU-side checks of the decoder pass's entry points (nm_decode_pass, nm_decode_pass_ok): they are exported, the library's
truth table on host descriptors -- exactly that of nm_latent_pass_ok: the two halves cover the same models -- Job.decode_ok()
agrees with the library, the launch returns its argument errors before it touches a device, NMHIP_DECODE=0 / 1 switch the
pass off / the classes' decode() route on, and the request rules the library cannot see (the request lives in device
memory) are raised by the Python side before the upload.  No compute calls: no GPU here."""
import ctypes as C

import pytest
import torch

import multi_modal_normative_modeling_amd as nm
from multi_modal_normative_modeling_amd import _lib, engine
from multi_modal_normative_modeling_amd.engine import JobSet
from tests.test_cabi_devpass_multi_cpu import _bare_job as _bare_job_fields, _descriptor, _probe
from tests.test_cabi_latent_cpu import test_job_check_agrees_with_library as _latent_spec_test


def _bare_job(spec, **kw):
    """The bare job of the sibling files with the decoder pass's fields as Job.__init__ leaves them."""
    j = _bare_job_fields(spec, **kw)
    j.dec_rows = j.dec_z = None
    j._dec_epoch = 0
    return j


@pytest.fixture(scope="module")
def lib():
    if not _lib.LIB_PATH.exists():
        import __graft_entry__ as ge
        ge.build()
    return _lib.load()


def test_symbols_and_the_request_struct(lib):
    for sym in ("nm_decode_pass", "nm_decode_pass_ok"):
        assert sym in _lib.EXPORTED_SYMBOLS
        assert hasattr(lib, sym), sym
    assert lib.nm_version() == 11
    assert _lib.NM_MAX_CELLS == 64
    # nm_decode_t: a pointer, three counts (+ padding to the next pointer), a pointer, five arrays of NM_MAX_EXP pointers
    assert C.sizeof(_lib.NmDecode) == 8 + 16 + 8 + 5 * _lib.NM_MAX_EXP * 8
    assert _lib.NmDecode.cgrid.offset == 24 and _lib.NmDecode.cz.offset == 32 and _lib.NmDecode.rowdev.offset == 32 + 4 * 32


def test_decode_pass_ok_truth_table(lib):
    for M in (1, 2, 3, 4):
        for bypass in (0, 1):
            ok = _probe(M=M)
            ok.single_bypass = bypass
            assert lib.nm_decode_pass_ok(C.byref(ok)) == 0, (M, bypass)
            ok.M_enc = M                                              # (M_enc = M says the same as M_enc = 0)
            assert lib.nm_decode_pass_ok(C.byref(ok)) == 0, (M, bypass)
    # the limits themselves are accepted: first hidden width 112, latent 32
    assert lib.nm_decode_pass_ok(C.byref(_probe(H=(112, 110), Z=32))) == 0
    assert lib.nm_decode_pass_ok(C.byref(_probe(M=1, H=(112, 110), Z=32))) == 0
    assert lib.nm_decode_pass_ok(C.byref(_probe(H=(113, 110)))) == _lib.NM_E_DEVPASS
    assert lib.nm_decode_pass_ok(C.byref(_probe(Z=33))) == _lib.NM_E_DEVPASS
    assert lib.nm_decode_pass_ok(C.byref(_probe(M=5))) == _lib.NM_E_DEVPASS
    assert lib.nm_decode_pass_ok(C.byref(_probe(M=0))) == _lib.NM_E_DEVPASS
    for M in (1, 3):
        for field, val in (("M_enc", M + 1), ("n_private", 1), ("tc_weight", 1e-4), ("w_off", 0), ("out_kind", 1), ("wide", 1)):
            bad = _probe(M=M)
            setattr(bad, field, val)
            assert lib.nm_decode_pass_ok(C.byref(bad)) == _lib.NM_E_DEVPASS, (M, field)
            assert lib.nm_latent_pass_ok(C.byref(bad)) == _lib.NM_E_DEVPASS, (M, field)   # the other half says the same
    assert lib.nm_decode_pass_ok(None) == _lib.NM_E_NULL


def test_launch_argument_errors_come_before_any_device_use(lib):
    p = 4096                                                          # (any non-null address: the checks come first)
    assert lib.nm_decode_pass(None, 1, p, 0, 1, 0, None) == _lib.NM_E_NULL
    assert lib.nm_decode_pass(p, 1, None, 0, 1, 0, None) == _lib.NM_E_NULL
    assert lib.nm_decode_pass(p, 0, p, 0, 1, 0, None) == _lib.NM_E_GEOMETRY
    assert lib.nm_decode_pass(p, 1, p, -1, 1, 0, None) == _lib.NM_E_GEOMETRY
    assert lib.nm_decode_pass(p, 1, p, 0, 0, 0, None) == _lib.NM_E_GEOMETRY


# the spec list of tests/test_cabi_latent_cpu.py, read off its parametrisation: the two halves admit the same models
_SPECS = [m for m in _latent_spec_test.pytestmark if m.name == "parametrize"][0].args[1]


@pytest.mark.parametrize("dims,hidden,Z,kind,want", _SPECS)
def test_job_check_agrees_with_library(lib, dims, hidden, Z, kind, want):
    spec = nm.ModelSpec(list(dims), list(hidden), Z, 3, True, kind)
    job = _bare_job(spec)
    assert job.decode_ok() == want
    assert (lib.nm_decode_pass_ok(C.byref(_descriptor(job))) == 0) == want
    assert job.decode_ok() == job.latent_ok()
    assert _bare_job(spec, latent_exports=True).decode_ok() == want


def test_total_correlation_and_the_environment_switch(lib, monkeypatch):
    tc = _bare_job(nm.ModelSpec([61, 90, 47], [64, 48], 12, 3, True, "mvtcae"), tc_weight=3e-4)
    assert not tc.decode_ok()
    assert lib.nm_decode_pass_ok(C.byref(_descriptor(tc))) == _lib.NM_E_DEVPASS
    spec = nm.ModelSpec([61, 90, 47], [64, 48], 12, 3, True, "multimodal")
    one = nm.ModelSpec([61], [64, 48], 12, 3, True, "multimodal")
    js = object.__new__(JobSet)
    js.jobs, js.wide = [_bare_job(spec), _bare_job(one)], False
    monkeypatch.delenv("NMHIP_DECODE", raising=False)
    assert js.decode_ok() and js._decode_refusal() is None
    assert js.decode_pick() == all(engine.DECODE_AUTO.get(m, False) for m in (3, 1))
    monkeypatch.setenv("NMHIP_DECODE", "1")                           # the classes' decode() route, forced on
    assert js.decode_ok() and js.decode_pick()
    monkeypatch.setenv("NMHIP_DECODE", "0")
    assert not js.decode_ok() and not js.decode_pick()
    assert "NMHIP_DECODE=0" in js._decode_refusal()
    with pytest.raises(ValueError, match="NMHIP_DECODE=0"):           # (the launch itself says so before it looks at a device)
        for j in js.jobs:
            j.dec_rows, j.dec_z = 1, torch.zeros(1)
        js.decode()
    monkeypatch.delenv("NMHIP_DECODE")
    monkeypatch.setenv("NMHIP_LATENT", "0")                           # (the encoder half's switch is not this kernel's)
    assert js.decode_ok()
    monkeypatch.delenv("NMHIP_LATENT")
    js.jobs.append(tc)
    assert not js.decode_ok() and "job 2" in js._decode_refusal()
    monkeypatch.setenv("NMHIP_DECODE", "1")
    assert not js.decode_pick()                                       # forcing the route does not widen what is admitted
    js.jobs, js.wide = [_bare_job(nm.ModelSpec([61, 90, 47], [300, 300], 12, 3, True, "multimodal"))], True
    assert not js.decode_ok() and "general-shape" in js._decode_refusal()


def _request(R=300, ra=512, G=3, Z=12, Cz=8, pitches=(64, 92), x=True, sqerr=True, rowdev=True):
    """The arguments of engine.check_decode_request for a valid request, host tensors of exactly the declared sizes."""
    cells, M = max(G, 1), len(pitches)
    return dict(n_rows=R, rows_alloc=ra, n_cells=G, Z=Z, Cz=Cz, pitches=list(pitches), z=torch.zeros(ra * Z),
                cgrid=torch.zeros(G * Cz, dtype=torch.bfloat16) if G else None,
                cz=[None if G else torch.zeros(ra * Cz, dtype=torch.bfloat16) for _ in range(M)],
                x=[torch.zeros(ra * p) if x else None for p in pitches],
                loc=[torch.zeros(cells * ra * p) for p in pitches],
                sqerr=[torch.zeros(cells * ra * p) if sqerr else None for p in pitches],
                rowdev=[torch.zeros(cells * ra) if rowdev else None for _ in pitches])


def test_request_validation_raises_before_the_upload():
    check = engine.check_decode_request
    for G in (0, 1, 3, 64):
        check(**_request(G=G))
    check(**_request(x=False, sqerr=False, rowdev=False))
    for G in (-1, 65, 1000):
        with pytest.raises(ValueError, match="n_cells"):
            check(**{**_request(), "n_cells": G})
    for ra in (300, 511, 513, 256):                                   # not a multiple of 256 / below n_rows
        with pytest.raises(ValueError, match="rows_alloc"):
            check(**{**_request(), "rows_alloc": ra})
    with pytest.raises(ValueError, match="taken against x"):
        check(**_request(x=False, sqerr=True, rowdev=False))
    with pytest.raises(ValueError, match="taken against x"):
        check(**_request(x=False, sqerr=False, rowdev=True))
    for what in ("loc", "sqerr", "rowdev"):
        r = _request()
        r[what][1] = r[what][1][:-1]                                  # one value short of [cells][rows_alloc][pitch]
        with pytest.raises(ValueError, match=what):
            check(**r)
    r = _request()
    r["loc"][0] = torch.zeros(512 * 64)                               # one cell's worth for a three-cell request
    with pytest.raises(ValueError, match="loc"):
        check(**r)
    r = _request()
    r["z"] = torch.zeros(300 * 12)                                    # n_rows rows, not rows_alloc
    with pytest.raises(ValueError, match="z must hold"):
        check(**r)
    r = _request()
    r["cgrid"] = None
    with pytest.raises(ValueError, match="c_grid"):
        check(**r)
    r = _request(G=0)
    r["cz"][1] = None
    with pytest.raises(ValueError, match="per-row covariates"):
        check(**r)
    r = _request()
    r["loc"] = [None, None]
    with pytest.raises(ValueError):
        check(**r)
    r = _request()
    r["loc"][0] = None                                                # a skipped decoder keeps no other export
    with pytest.raises(ValueError, match="without loc"):
        check(**r)
    r["sqerr"][0] = r["rowdev"][0] = None
    check(**r)


def test_enable_decode_exports_refuses_counts_before_it_allocates():
    job = _bare_job(nm.ModelSpec([61, 90, 47], [64, 48], 12, 3, True, "multimodal"))
    for G in (-1, 65):
        with pytest.raises(ValueError, match="n_cells"):
            job.enable_decode_exports(300, n_cells=G)
    with pytest.raises(ValueError, match="n_rows"):
        job.enable_decode_exports(0)
    with pytest.raises(ValueError, match="loc=False"):
        job.enable_decode_exports(300, loc=False)
    for dec in ((), (3,), (-1,)):
        with pytest.raises(ValueError, match="decoders"):
            job.enable_decode_exports(300, decoders=dec)
    with pytest.raises(ValueError, match="enable_decode_exports"):
        job.set_decode_inputs(torch.zeros(300, 12))


def test_pack_covariates_layout():
    """c | 1 | 0 per row in bf16, zero rows past the table: the layout nm_pack_table writes to Table.cz (the GPU test holds the
    bytes to a Table's)."""
    c = torch.tensor([[0.0, 1.0, 0.3], [2.0, 0.0, -1.7]])
    out = engine.pack_covariates(c, 8, 4, "cpu")
    assert out.dtype == torch.bfloat16 and tuple(out.shape) == (4, 8)
    want = torch.zeros(4, 8)
    want[:2, :3], want[:2, 3] = c.to(torch.bfloat16).float(), 1.0
    assert torch.equal(out.float(), want)
    assert float(out[0, 2]) != 0.3                                    # (0.3 rounds in bf16)
    with pytest.raises(ValueError):
        engine.pack_covariates(torch.zeros(2, 8), 8, 4, "cpu")
    with pytest.raises(ValueError):
        engine.pack_covariates(torch.zeros(5, 3), 8, 4, "cpu")
