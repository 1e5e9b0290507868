"""CPU-side checks of the posterior-predictive pass's entry points (nm_devpass_draws, nm_devpass_draws_ok): they are exported,
the two table entries' layouts are the header's, the launch's status is decided on the host before the device is asked
anything, the predicate admits every case of the several-expert and the one-expert twins (bypass on or off) and agrees with
Job.draws_ok(), and the engine refuses a malformed request where it builds the tables.  No compute calls: no GPU here."""
import ctypes as C
import re
from pathlib import Path

import pytest

import multi_modal_normative_modeling_amd as nm
from multi_modal_normative_modeling_amd import _lib
from multi_modal_normative_modeling_amd.engine import Job, JobSet
from tests import twin_cases as T

ROOT = Path(__file__).resolve().parent.parent


@pytest.fixture(scope="module")
def lib():
    if not _lib.LIB_PATH.exists():
        import __graft_entry__ as ge
        ge.build()
    return _lib.load()


def _bare_job(spec, single_bypass=True, tc_weight=0.0):
    """A Job with the fields draws_ok() and enable_predictive_exports() read before they allocate, and no device behind it."""
    j = object.__new__(Job)
    j.spec, j.kmods = spec, spec.kernel_modalities()
    j.single_bypass, j.tc_weight = single_bypass, tc_weight
    j.seed, j.eps, j.eps_cap, j.n_draws = 11, None, 1, None
    return j


def _descriptor(job):
    """The fields of Job.struct() the predicate reads, filled as Job.struct() fills them."""
    s, d = job.spec, _lib.NmJob()
    d.M, d.M_enc, d.C, d.L, d.Z = len(job.kmods), s.M, s.net_c_dim, len(s.hidden), s.latent
    for i, h in enumerate(s.hidden):
        d.H[i] = h
    d.out_kind = 1 if s.is_dm else 0
    d.n_private = s.n_private
    d.w_off = 0 if s.kind == "weighted_dmvae" else -1
    d.wide = int(s.wide)
    d.tc_weight = job.tc_weight
    d.single_bypass = 1 if job.single_bypass else 0
    return d


def _spec(dims, hidden, Z, c_dim=3, kind="multimodal"):
    return nm.ModelSpec(list(dims), list(hidden), Z, c_dim, True, kind)


def test_symbols_and_limits(lib):
    for sym in ("nm_devpass_draws", "nm_devpass_draws_ok"):
        assert sym in _lib.EXPORTED_SYMBOLS
        assert hasattr(lib, sym), sym
    header = (ROOT / "include" / "nmhip.h").read_text()
    assert int(re.search(r"#define NM_MAX_DRAWS (\d+)", header).group(1)) == _lib.NM_MAX_DRAWS == 64


def _header_fields(name):
    header = (ROOT / "include" / "nmhip.h").read_text()
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), header, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    return re.findall(r"(\w+)(?:\[NM_MAX_EXP\])?;", body)


def test_table_entry_layouts_are_the_headers():
    assert _header_fields("nm_draw_t") == [f[0] for f in _lib.NmDraw._fields_]
    assert C.sizeof(_lib.NmDraw) == 16 and _lib.NmDraw.seed.offset == 0 and _lib.NmDraw.eps.offset == 8
    assert _header_fields("nm_pred_t") == [f[0] for f in _lib.NmPred._fields_]
    assert C.sizeof(_lib.NmPred) == 7 * 8 * _lib.NM_MAX_EXP
    for k, (name, _) in enumerate(_lib.NmPred._fields_):
        assert getattr(_lib.NmPred, name).offset == k * 8 * _lib.NM_MAX_EXP, name


def test_launch_status_is_decided_without_a_device(lib):
    """A missing descriptor array or table: NM_E_NULL; n_draws outside 1..64 and the geometry rules of every launch:
    NM_E_GEOMETRY -- all before anything is asked of a device (there is none here; the addresses are never read)."""
    jobs, draws, pred = 4096, 8192, 12288
    assert lib.nm_devpass_draws(None, 1, draws, 1, pred, 0, 1, 0, None) == _lib.NM_E_NULL
    assert lib.nm_devpass_draws(jobs, 1, None, 1, pred, 0, 1, 0, None) == _lib.NM_E_NULL
    assert lib.nm_devpass_draws(jobs, 1, draws, 1, None, 0, 1, 0, None) == _lib.NM_E_NULL
    for S in (0, -1, 65, 1 << 20):
        assert lib.nm_devpass_draws(jobs, 1, draws, S, pred, 0, 1, 0, None) == _lib.NM_E_GEOMETRY, S
    assert lib.nm_devpass_draws(jobs, 0, draws, 8, pred, 0, 1, 0, None) == _lib.NM_E_GEOMETRY
    assert lib.nm_devpass_draws(jobs, 1, draws, 8, pred, 0, 0, 0, None) == _lib.NM_E_GEOMETRY
    assert lib.nm_devpass_draws(jobs, 1, draws, 8, pred, -1, 1, 0, None) == _lib.NM_E_GEOMETRY
    assert lib.nm_devpass_draws_ok(None) == _lib.NM_E_NULL


@pytest.mark.parametrize("cs", T.cases("devpass_multi") + T.cases("devpass") + T.cases("latent"), ids=lambda cs: cs.id)
def test_predicate_admits_every_twin_case_and_agrees_with_the_job(lib, cs):
    """The whole domains of the several-expert pass, the one-expert pass and the encoder-only pass (1..4 experts, bypass on or
    off): admitted by the library and by Job.draws_ok() alike."""
    job = _bare_job(_spec(cs.dims, cs.hidden, cs.Z, cs.c_dim, cs.kind), single_bypass=cs.single_bypass)
    assert lib.nm_devpass_draws_ok(C.byref(_descriptor(job))) == 0
    assert job.draws_ok()


@pytest.mark.parametrize("dims,hidden,Z,kind,bypass,want", [
    ((70,), (112,), 32, "multimodal", True, True),                  # one expert at the limits
    ((70,), (112,), 32, "multimodal", False, True),                 # ... with the bypass off
    ((379,), (110, 110), 10, "single", True, True),                 # the cVAE class
    ((379,), (110, 110), 10, "regression", True, True),             # the regression script's unimodal pass
    ((40, 40, 40, 120), (112,), 32, "multimodal", True, True),
    ((70,), (113,), 32, "multimodal", True, False),
    ((70,), (112,), 33, "multimodal", True, False),
    ((61, 90, 47), (113, 48), 12, "multimodal", True, False),
    ((61, 90, 47), (64, 48), 33, "multimodal", True, False),
    ((61, 90, 47), (300, 300), 12, "multimodal", True, False),      # general-shape path
    ((61, 90, 47), (64, 48), 12, "endtoend", True, False),          # decoder-only modalities
    ((61, 90, 47), (64, 48), 12, "dmvae", True, False),             # private latent, sigmoid output
    ((61, 90, 47), (64, 48), 12, "weighted_dmvae", True, False),
])
def test_predicate_and_job_check_agree_on_the_edges(lib, dims, hidden, Z, kind, bypass, want):
    job = _bare_job(_spec(dims, hidden, Z, 3, kind), single_bypass=bypass)
    st = lib.nm_devpass_draws_ok(C.byref(_descriptor(job)))
    assert st == (0 if want else _lib.NM_E_DEVPASS)
    assert job.draws_ok() == want


def test_field_by_field_refusals(lib):
    for M in (1, 3):
        dims = (61, 90, 47)[:M]
        for field, val in (("M", 0), ("M", 5), ("M_enc", M + 1), ("n_private", 1), ("tc_weight", 1e-4), ("w_off", 0),
                           ("out_kind", 1), ("wide", 1)):
            d = _descriptor(_bare_job(_spec(dims, (112, 48), 12)))
            setattr(d, field, val)
            assert lib.nm_devpass_draws_ok(C.byref(d)) == _lib.NM_E_DEVPASS, (M, field, val)
            assert lib.nm_devpass_draws_ok(C.byref(d)) == lib.nm_latent_pass_ok(C.byref(d))
    tc = _bare_job(_spec((61, 90, 47), (64, 48), 12, 3, "mvtcae"), tc_weight=3e-4)
    assert not tc.draws_ok() and lib.nm_devpass_draws_ok(C.byref(_descriptor(tc))) == _lib.NM_E_DEVPASS


@pytest.mark.parametrize("kw,word", [
    ({"n_draws": 0}, "1 to 64"),
    ({"n_draws": 65}, "1 to 64"),
    ({"n_draws": 4, "seeds": [1, 2, 3]}, "one per draw"),
    ({"n_draws": 2, "eps": [None]}, "one tensor per draw"),
    ({"n_draws": 1, "seeds": [1], "eps": [None]}, "not both"),
])
def test_engine_refuses_a_malformed_request(kw, word):
    j = _bare_job(_spec((61, 90, 47), (64, 48), 12))
    with pytest.raises(ValueError, match=word):
        j.enable_predictive_exports(**kw)
    assert j.n_draws is None


def test_forward_draws_wants_the_exports_first_and_one_draw_count():
    js = object.__new__(JobSet)
    a, b = _bare_job(_spec((61, 90, 47), (64, 48), 12)), _bare_job(_spec((61, 90, 47), (64, 48), 12))
    js.jobs, js.wide = [a, b], False
    with pytest.raises(ValueError, match="enable_predictive_exports"):
        js.forward_draws()
    a.n_draws, b.n_draws = 4, 8
    with pytest.raises(ValueError, match="same number of draws"):
        js.forward_draws()
    b.n_draws = 4
    js.wide = True
    with pytest.raises(ValueError, match="general-shape"):
        js.forward_draws()
