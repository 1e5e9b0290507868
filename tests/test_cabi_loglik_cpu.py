"""CPU-side checks of the likelihood pass's entry points (nm_devpass_iw, nm_devpass_iw_ok, nm_iw_check): they are exported, the
request's layout is the header's, every status is decided on the host before the device is asked anything, the predicate is
the posterior-predictive pass's, and the engine refuses a malformed request where it builds the tables.  No compute calls: no
GPU here."""
import ctypes as C
import re
from pathlib import Path

import pytest

import multi_modal_normative_modeling_amd as nm
from multi_modal_normative_modeling_amd import _lib, metrics
from multi_modal_normative_modeling_amd.engine import Job, JobSet
from tests import twin_cases as T
from tests.test_cabi_draws_cpu import _bare_job, _descriptor, _spec

ROOT = Path(__file__).resolve().parent.parent


@pytest.fixture(scope="module")
def lib():
    if not _lib.LIB_PATH.exists():
        import __graft_entry__ as ge
        ge.build()
    return _lib.load()


def test_symbols_and_limits(lib):
    for sym in ("nm_devpass_iw", "nm_devpass_iw_ok", "nm_iw_check"):
        assert sym in _lib.EXPORTED_SYMBOLS
        assert hasattr(lib, sym), sym
    header = (ROOT / "include" / "nmhip.h").read_text()
    assert int(re.search(r"#define NM_MAX_IW_DRAWS (\d+)", header).group(1)) == _lib.NM_MAX_IW_DRAWS == 1024
    assert int(re.search(r"#define NM_IW_ROW_COLUMNS (\d+)", header).group(1)) == _lib.NM_IW_ROW_COLUMNS == 8
    assert metrics.LOGLIK_ROW_COLUMNS == ("log_px", "elbo", "ess", "kl_mc", "kl", "recon_ll", "logw_max", "logw_min")
    # the header names the columns in the export's order
    block = header[header.index("Exports per job: row"):header.index("and optionally recon_ll[m]")]
    assert re.findall(r"(\w+) =", block.split("=", 1)[1]) == list(metrics.LOGLIK_ROW_COLUMNS)[:6]


def test_request_layout_is_the_headers():
    header = (ROOT / "include" / "nmhip.h").read_text()
    body = re.search(r"typedef struct nm_iw_t \{(.*?)\} nm_iw_t;", header, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert re.findall(r"(\w+)(?:\[NM_MAX_EXP\])?;", body) == [f[0] for f in _lib.NmIw._fields_]
    E = _lib.NM_MAX_EXP
    assert _lib.NmIw.row.offset == 0 and _lib.NmIw.recon_ll.offset == 8 and _lib.NmIw.noise_var.offset == 8 + 8 * E
    assert _lib.NmIw.ll_const.offset == 8 + 16 * E and _lib.NmIw.dec_mask.offset == 8 + 20 * E
    assert C.sizeof(_lib.NmIw) == (8 + 20 * E + 4 + 7) // 8 * 8


def test_launch_status_is_decided_without_a_device(lib):
    """A missing descriptor array or table: NM_E_NULL; n_draws outside 1..1024 and the geometry rules of every launch:
    NM_E_GEOMETRY -- all before anything is asked of a device (there is none here; the addresses are never read)."""
    jobs, draws, iw = 4096, 8192, 12288
    assert lib.nm_devpass_iw(None, 1, draws, 1, iw, 0, 1, 0, None) == _lib.NM_E_NULL
    assert lib.nm_devpass_iw(jobs, 1, None, 1, iw, 0, 1, 0, None) == _lib.NM_E_NULL
    assert lib.nm_devpass_iw(jobs, 1, draws, 1, None, 0, 1, 0, None) == _lib.NM_E_NULL
    for S in (0, -1, 1025, 1 << 20):
        assert lib.nm_devpass_iw(jobs, 1, draws, S, iw, 0, 1, 0, None) == _lib.NM_E_GEOMETRY, S
    assert lib.nm_devpass_iw(jobs, 0, draws, 8, iw, 0, 1, 0, None) == _lib.NM_E_GEOMETRY
    assert lib.nm_devpass_iw(jobs, 1, draws, 8, iw, 0, 0, 0, None) == _lib.NM_E_GEOMETRY
    assert lib.nm_devpass_iw(jobs, 1, draws, 8, iw, -1, 1, 0, None) == _lib.NM_E_GEOMETRY
    assert lib.nm_devpass_iw_ok(None) == _lib.NM_E_NULL


def _request(M, mask=None, row=4096, noise=True):
    q = _lib.NmIw()
    q.row, q.dec_mask = row, (1 << M) - 1 if mask is None else mask
    for m in range(M):
        q.noise_var[m] = 8192 + 64 * m if noise else None
    return q


def test_request_status_is_decided_on_the_host(lib):
    """nm_iw_check on the host copies: a row export that is NULL or a wanted decoder without noise_var NM_E_NULL, an empty
    mask or a bit at or above M NM_E_GEOMETRY, a job outside the domain NM_E_DEVPASS (the addresses are never read)."""
    d = _descriptor(_bare_job(_spec((61, 90, 47), (64, 48), 12)))
    chk = lambda q, dd=d: lib.nm_iw_check(C.byref(dd), C.byref(q))
    assert chk(_request(3)) == 0
    assert lib.nm_iw_check(None, C.byref(_request(3))) == _lib.NM_E_NULL and lib.nm_iw_check(C.byref(d), None) == _lib.NM_E_NULL
    assert chk(_request(3, row=None)) == _lib.NM_E_NULL
    assert chk(_request(3, noise=False)) == _lib.NM_E_NULL
    for mask in (1, 2, 4, 5, 7):
        assert chk(_request(3, mask=mask)) == 0, mask
    q = _request(3, mask=2, noise=False)                     # only the wanted decoder needs its table
    assert chk(q) == _lib.NM_E_NULL
    q.noise_var[1] = 8192
    assert chk(q) == 0
    for mask in (0, 8, 15, 1 << 31):
        assert chk(_request(3, mask=mask)) == _lib.NM_E_GEOMETRY, mask
    wide = _descriptor(_bare_job(_spec((61, 90, 47), (300, 300), 12)))
    assert chk(_request(3), wide) == _lib.NM_E_DEVPASS


@pytest.mark.parametrize("cs", T.cases("devpass_multi") + T.cases("devpass") + T.cases("latent"), ids=lambda cs: cs.id)
def test_predicate_is_the_posterior_predictive_passes(lib, cs):
    d = _descriptor(_bare_job(_spec(cs.dims, cs.hidden, cs.Z, cs.c_dim, cs.kind), single_bypass=cs.single_bypass))
    assert lib.nm_devpass_iw_ok(C.byref(d)) == lib.nm_devpass_draws_ok(C.byref(d)) == 0


@pytest.mark.parametrize("dims,hidden,Z,kind", [
    ((70,), (113,), 32, "multimodal"), ((70,), (112,), 33, "multimodal"), ((61, 90, 47), (300, 300), 12, "multimodal"),
    ((61, 90, 47), (64, 48), 12, "endtoend"), ((61, 90, 47), (64, 48), 12, "dmvae"), ((61, 90, 47), (64, 48), 12, "weighted_dmvae"),
])
def test_predicate_refuses_what_lies_outside_the_domain(lib, dims, hidden, Z, kind):
    d = _descriptor(_bare_job(_spec(dims, hidden, Z, 3, kind)))
    assert lib.nm_devpass_iw_ok(C.byref(d)) == _lib.NM_E_DEVPASS


@pytest.mark.parametrize("kw,word", [
    ({"n_draws": 0}, "1 to 1024"),
    ({"n_draws": 1025}, "1 to 1024"),
    ({"n_draws": 4, "seeds": [1, 2, 3]}, "one per draw"),
    ({"n_draws": 2, "eps": [None]}, "one tensor per draw"),
    ({"n_draws": 1, "seeds": [1], "eps": [None]}, "not both"),
    ({"n_draws": 2, "decoders": []}, "decoders"),
    ({"n_draws": 2, "decoders": [3]}, "decoders"),
    ({"n_draws": 2, "decoders": [-1]}, "decoders"),
])
def test_engine_refuses_a_malformed_request(kw, word):
    j = _bare_job(_spec((61, 90, 47), (64, 48), 12))
    j.iw_draws = None
    with pytest.raises(ValueError, match=word):
        j.enable_likelihood_exports(**kw)
    assert j.iw_draws is None


def test_forward_loglik_wants_the_exports_first_and_one_draw_count():
    js = object.__new__(JobSet)
    a, b = _bare_job(_spec((61, 90, 47), (64, 48), 12)), _bare_job(_spec((61, 90, 47), (64, 48), 12))
    js.jobs, js.wide = [a, b], False
    with pytest.raises(ValueError, match="enable_likelihood_exports"):
        js.forward_loglik()
    a.iw_draws, b.iw_draws = 4, 8
    with pytest.raises(ValueError, match="same number of draws"):
        js.forward_loglik()
    b.iw_draws = 4
    js.wide = True
    with pytest.raises(ValueError, match="general-shape"):
        js.forward_loglik()


def test_the_drop_in_classes_carry_pred_loglik():
    for cls in ("cVAE_multimodal", "mmJSD", "cVAE_multimodal_regression", "cVAE"):
        assert callable(getattr(getattr(nm, cls), "pred_loglik")), cls
        assert callable(getattr(getattr(nm, cls), "pred_recon_draws")), cls
