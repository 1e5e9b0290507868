"""CPU-side checks of the chart pass's entry points (nm_chart_pass, nm_chart_pass_ok): they are exported, nm_chart_t and its
ctypes mirror agree, the library's truth table is nm_decode_pass_ok's over the job shapes of tests/test_cabi_decode_cpu.py,
the launch returns its argument errors before it touches a device, and the request rules the library cannot see are raised
by engine.check_chart_request before the upload.  No compute calls: no GPU here."""
import ctypes as C
import re
from pathlib import Path

import pytest
import torch

import multi_modal_normative_modeling_amd as nm
from multi_modal_normative_modeling_amd import _lib, engine, metrics
from multi_modal_normative_modeling_amd.engine import JobSet
from tests.test_cabi_decode_cpu import _SPECS, _bare_job as _bare_decode_job
from tests.test_cabi_devpass_multi_cpu import _descriptor, _probe


def _bare_job(spec, **kw):
    j = _bare_decode_job(spec, **kw)
    j.chart_rows = j.chart_z = None
    j._chart_epoch = 0
    return j


@pytest.fixture(scope="module")
def lib():
    if not _lib.LIB_PATH.exists():
        import __graft_entry__ as ge
        ge.build()
    return _lib.load()


def test_symbols_and_the_request_struct(lib):
    for sym in ("nm_chart_pass", "nm_chart_pass_ok"):
        assert sym in _lib.EXPORTED_SYMBOLS
        assert hasattr(lib, sym), sym
    # nm_chart_t: a pointer, three counts (+ padding to the next pointer), a pointer, three arrays of NM_MAX_EXP pointers
    S = _lib.NmChart
    assert C.sizeof(S) == 8 + 16 + 8 + 3 * _lib.NM_MAX_EXP * 8
    assert (S.z.offset, S.n_rows.offset, S.rows_alloc.offset, S.n_cells.offset, S.cgrid.offset) == (0, 8, 12, 16, 24)
    assert (S.part.offset, S.chart.offset, S.loc.offset) == (32, 32 + 8 * _lib.NM_MAX_EXP, 32 + 16 * _lib.NM_MAX_EXP)
    # the header states the same fields in the same order, and the same constants
    hdr = (Path(__file__).resolve().parents[1] / "include" / "nmhip.h").read_text()
    body = re.search(r"typedef struct nm_chart_t \{(.*?)\} nm_chart_t;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = re.findall(r"(\w+)(?:\[NM_MAX_EXP\])?\s*[,;]", body)
    assert names == [f[0] for f in S._fields_]
    assert int(re.search(r"#define NM_CHART_COLUMNS (\d+)", hdr).group(1)) == _lib.NM_CHART_COLUMNS == len(metrics.CHART_COLUMNS)
    assert int(re.search(r"#define NM_CHART_MAX_ROWS (\d+)", hdr).group(1)) == _lib.NM_CHART_MAX_ROWS == 1 << 20
    assert metrics.CHART_COLUMNS == ("mean", "var_latent", "n_rows", "status")


def test_chart_pass_ok_is_decode_pass_ok(lib):
    probes = [_probe(M=M) for M in (0, 1, 2, 3, 4, 5)] + [_probe(H=(112, 110), Z=32), _probe(H=(113, 110)), _probe(Z=33)]
    for M in (1, 3):
        for field, val in (("M_enc", M + 1), ("n_private", 1), ("tc_weight", 1e-4), ("w_off", 0), ("out_kind", 1), ("wide", 1),
                           ("single_bypass", 0)):
            p = _probe(M=M)
            setattr(p, field, val)
            probes.append(p)
    seen = set()
    for p in probes:
        got = lib.nm_chart_pass_ok(C.byref(p))
        assert got == lib.nm_decode_pass_ok(C.byref(p))
        seen.add(got)
    assert seen == {0, _lib.NM_E_DEVPASS}
    assert lib.nm_chart_pass_ok(None) == _lib.NM_E_NULL


@pytest.mark.parametrize("dims,hidden,Z,kind,want", _SPECS)
def test_job_check_agrees_with_library(lib, dims, hidden, Z, kind, want):
    job = _bare_job(nm.ModelSpec(list(dims), list(hidden), Z, 3, True, kind))
    assert job.chart_ok() == want == job.decode_ok()
    d = _descriptor(job)
    assert (lib.nm_chart_pass_ok(C.byref(d)) == 0) == want
    assert lib.nm_chart_pass_ok(C.byref(d)) == lib.nm_decode_pass_ok(C.byref(d))


def test_launch_argument_errors_come_before_any_device_use(lib):
    p = 4096                                                          # (any non-null address: the checks come first)
    assert lib.nm_chart_pass(None, 1, p, 0, 1, 1, 0, None) == _lib.NM_E_NULL
    assert lib.nm_chart_pass(p, 1, None, 0, 1, 1, 0, None) == _lib.NM_E_NULL
    assert lib.nm_chart_pass(p, 0, p, 0, 1, 1, 0, None) == _lib.NM_E_GEOMETRY
    assert lib.nm_chart_pass(p, 1, p, -1, 1, 1, 0, None) == _lib.NM_E_GEOMETRY
    assert lib.nm_chart_pass(p, 1, p, 0, 0, 1, 0, None) == _lib.NM_E_GEOMETRY
    assert lib.nm_chart_pass(p, 1, p, 0, 65536, 1, 0, None) == _lib.NM_E_GEOMETRY
    for cells in (0, -1, 65):
        assert lib.nm_chart_pass(p, 1, p, 0, 1, cells, 0, None) == _lib.NM_E_GEOMETRY


def test_environment_switches_and_refusal_wording(lib, monkeypatch):
    spec = nm.ModelSpec([61, 90, 47], [64, 48], 12, 3, True, "multimodal")
    js = object.__new__(JobSet)
    js.jobs, js.wide = [_bare_job(spec)], False
    monkeypatch.delenv("NMHIP_DECODE", raising=False)
    monkeypatch.delenv("NMHIP_CHART", raising=False)
    assert js.chart_ok()
    assert not any(engine.CHART_AUTO.values()) and not js.chart_pick()          # all off in this tree
    monkeypatch.setenv("NMHIP_CHART", "1")
    assert js.chart_pick()
    with pytest.raises(ValueError, match="enable_chart_exports"):
        js.chart()
    dm = _bare_job(nm.ModelSpec([61, 90, 47], [64, 48], 12, 3, True, "dmvae"))
    js.jobs.append(dm)
    assert not js.chart_ok() and not js.chart_pick()                  # forcing the route does not widen what is admitted
    for j in js.jobs:
        j.chart_rows, j.chart_z = 1, torch.zeros(1)
    with pytest.raises(ValueError, match="job 1: nm_decode_pass_ok refuses"):
        js.chart()
    js.jobs, js.wide = [_bare_job(nm.ModelSpec([61, 90, 47], [300, 300], 12, 3, True, "multimodal"))], True
    js.jobs[0].chart_rows, js.jobs[0].chart_z = 1, torch.zeros(1)
    with pytest.raises(ValueError, match="general-shape"):
        js.chart()


def _request(R=300, ra=512, G=3, Z=12, Cz=8, pitches=(64, 92), loc=True):
    """The arguments of engine.check_chart_request for a valid request, host tensors of exactly the declared sizes."""
    return dict(n_rows=R, rows_alloc=ra, n_cells=G, Z=Z, Cz=Cz, pitches=list(pitches), z=torch.zeros(ra * Z),
                cgrid=torch.zeros(G * Cz, dtype=torch.bfloat16),
                part=[torch.zeros(G * (ra // 128) * p * 2, dtype=torch.float64) for p in pitches],
                chart=[torch.zeros(G * p * 4, dtype=torch.float64) for p in pitches],
                loc=[torch.zeros(G * ra * p) if loc else None for p in pitches])


def test_request_validation_raises_before_the_upload():
    check = engine.check_chart_request
    for G in (1, 3, 64):
        check(**_request(G=G))
    check(**_request(loc=False))
    for G in (0, -1, 65):
        with pytest.raises(ValueError, match="n_cells"):
            check(**{**_request(), "n_cells": G})
    for ra in (300, 511, 513, 256):                                   # not a multiple of 256 / below n_rows
        with pytest.raises(ValueError, match="rows_alloc"):
            check(**{**_request(), "rows_alloc": ra})
    with pytest.raises(ValueError, match="rows_alloc"):
        check(**{**_request(), "n_rows": _lib.NM_CHART_MAX_ROWS + 1, "rows_alloc": _lib.NM_CHART_MAX_ROWS + 256})
    r = _request()
    r["part"][1] = None
    with pytest.raises(ValueError, match="chart without part"):
        check(**r)
    for what in ("part", "chart", "loc"):
        r = _request()
        r[what][1] = r[what][1][:-1]                                  # one value short of the declared shape
        with pytest.raises(ValueError, match=what):
            check(**r)
    r = _request()
    r["z"] = torch.zeros(300 * 12)                                    # n_rows rows, not rows_alloc
    with pytest.raises(ValueError, match="z must hold"):
        check(**r)
    r = _request()
    r["cgrid"] = r["cgrid"][:-1]
    with pytest.raises(ValueError, match="c_grid"):
        check(**r)
    r = _request(loc=False)
    r["part"], r["chart"] = [None, None], [None, None]
    with pytest.raises(ValueError, match="no decoder is wanted"):
        check(**r)
    r = _request()
    r["part"][0] = r["chart"][0] = r["loc"][0] = None                 # a skipped decoder
    check(**r)


def test_enable_chart_exports_refuses_counts_before_it_allocates():
    job = _bare_job(nm.ModelSpec([61, 90, 47], [64, 48], 12, 3, True, "multimodal"))
    for G in (0, -1, 65):
        with pytest.raises(ValueError, match="n_cells"):
            job.enable_chart_exports(300, G)
    for R in (0, _lib.NM_CHART_MAX_ROWS + 1):
        with pytest.raises(ValueError, match="n_rows"):
            job.enable_chart_exports(R, 3)
    for dec in ((), (3,), (-1,)):
        with pytest.raises(ValueError, match="decoders"):
            job.enable_chart_exports(300, 3, decoders=dec)
    with pytest.raises(ValueError, match="nothing is wanted"):
        job.enable_chart_exports(300, 3, chart=False)
    with pytest.raises(ValueError, match="enable_chart_exports"):
        job.set_chart_inputs(torch.zeros(300, 12), torch.zeros(3, 3))
