"""CPU-side checks of the modality-subset pass's entry points (nm_devpass_subsets, nm_devpass_subsets_ok): they are exported,
the predicate is nm_devpass_multi_ok's over that twin's whole case list and the refused shapes, the launch's status is
decided on the host before the device is asked anything, the table entry's layout is the header's, and the engine refuses a
malformed subset list where it builds the table.  No compute calls: there is no GPU here."""
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


def _descriptor(dims, hidden, Z, c_dim, kind="multimodal"):
    """The fields of Job.struct() the predicates read, filled as Job.struct() fills them."""
    s, d = nm.ModelSpec(list(dims), list(hidden), Z, c_dim, True, kind), _lib.NmJob()
    d.M, d.M_enc, d.C, d.L, d.Z = len(s.kernel_modalities()), s.M, s.net_c_dim, len(s.hidden), s.latent
    for i, h in enumerate(s.hidden):
        d.H[i] = h
    d.out_kind = 1 if s.is_dm else 0
    d.n_private = s.n_private
    d.w_off = 0 if s.kind == "weighted_dmvae" else -1
    d.wide = int(s.wide)
    d.single_bypass = 1
    return d


def test_symbols_are_exported(lib):
    for sym in ("nm_devpass_subsets", "nm_devpass_subsets_ok"):
        assert sym in _lib.EXPORTED_SYMBOLS
        assert hasattr(lib, sym), sym
    assert _lib.NM_MAX_SUBSETS == (1 << _lib.NM_MAX_EXP) - 1


def test_subset_entry_layout_is_the_headers():
    """nm_subset_t: mask, a reserved word, the presence pointer, three pointer arrays of NM_MAX_EXP -- field by field in the
    header's order, no padding the mirror does not have."""
    header = (ROOT / "include" / "nmhip.h").read_text()
    body = re.search(r"typedef struct nm_subset_t \{(.*?)\} nm_subset_t;", header, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = re.findall(r"(\w+)(?:\[NM_MAX_EXP\])?;", body)
    assert names == [f[0] for f in _lib.NmSubset._fields_]
    assert C.sizeof(_lib.NmSubset) == 8 + 8 + 3 * 8 * _lib.NM_MAX_EXP
    assert _lib.NmSubset.present.offset == 8 and _lib.NmSubset.out_loc.offset == 16


@pytest.mark.parametrize("cs", T.cases("devpass_multi"), ids=lambda cs: cs.id)
def test_predicate_accepts_every_devpass_multi_case(lib, cs):
    d = _descriptor(cs.dims, cs.hidden, cs.Z, cs.c_dim, cs.kind)
    assert lib.nm_devpass_multi_ok(C.byref(d)) == 0
    assert lib.nm_devpass_subsets_ok(C.byref(d)) == 0


@pytest.mark.parametrize("why,dims,hidden,Z,kind", [
    ("wide", (61, 90, 47), (300, 300), 12, "multimodal"),
    ("H0 = 113", (61, 90, 47), (113, 48), 12, "multimodal"),
    ("Z = 33", (61, 90, 47), (64, 48), 33, "multimodal"),
    ("M = 1", (379,), (110, 110), 10, "multimodal"),
    ("end-to-end trunk", (61, 90, 47), (64, 48), 12, "endtoend"),
])
def test_predicate_refuses_what_devpass_multi_refuses(lib, why, dims, hidden, Z, kind):
    d = _descriptor(dims, hidden, Z, 3, kind)
    assert lib.nm_devpass_multi_ok(C.byref(d)) == _lib.NM_E_DEVPASS, why
    assert lib.nm_devpass_subsets_ok(C.byref(d)) == _lib.NM_E_DEVPASS, why
    assert lib.nm_devpass_subsets_ok(None) == _lib.NM_E_NULL


def test_field_by_field_the_two_predicates_agree(lib):
    for field, val in (("M", 1), ("M", 5), ("M_enc", 2), ("n_private", 1), ("tc_weight", 1e-4), ("w_off", 0), ("out_kind", 1),
                       ("wide", 1), ("Z", 32), ("Z", 33), ("single_bypass", 0)):
        d = _descriptor((61, 90, 47), (112, 48), 12, 3)
        setattr(d, field, val)
        assert lib.nm_devpass_subsets_ok(C.byref(d)) == lib.nm_devpass_multi_ok(C.byref(d)), (field, val)


def test_launch_status_is_decided_without_a_device(lib):
    """A missing descriptor array or table: NM_E_NULL; n_subsets outside 1..15 and the geometry rules of every launch:
    NM_E_GEOMETRY -- all before anything is asked of a device (there is none here; the addresses are never read)."""
    jobs, table = 4096, 8192
    assert lib.nm_devpass_subsets(None, 1, table, 1, 0, 1, 0, None) == _lib.NM_E_NULL
    assert lib.nm_devpass_subsets(jobs, 1, None, 1, 0, 1, 0, None) == _lib.NM_E_NULL
    for ns in (0, -1, 16, 1 << 20):
        assert lib.nm_devpass_subsets(jobs, 1, table, ns, 0, 1, 0, None) == _lib.NM_E_GEOMETRY, ns
    assert lib.nm_devpass_subsets(jobs, 0, table, 7, 0, 1, 0, None) == _lib.NM_E_GEOMETRY
    assert lib.nm_devpass_subsets(jobs, 1, table, 7, 0, 0, 0, None) == _lib.NM_E_GEOMETRY
    assert lib.nm_devpass_subsets(jobs, 1, table, 7, -1, 1, 0, None) == _lib.NM_E_GEOMETRY


def _bare_job(dims=(61, 90, 47)):
    """A Job with the fields enable_subset_exports() reads before it allocates, and no device behind it."""
    j = object.__new__(Job)
    j.spec = nm.ModelSpec(list(dims), [64, 48], 12, 3, True, "multimodal")
    j.kmods = j.spec.kernel_modalities()
    j.sub_masks = None
    return j


@pytest.mark.parametrize("subsets,word", [
    ([()], "empty"),                                                   # mask 0
    ([(0, 1), ()], "empty"),
    ([(0, 3)], "experts 0..2"),                                        # bit >= M
    ([(-1,)], "experts 0..2"),
    ([(0, 1), (1, 0)], "twice"),                                       # the same set in another order
    ([(2,), (0,), (2,)], "twice"),
    ([], "1 to 15"),
    ([(0,)] * 16, "1 to 15"),                                          # more than 15
])
def test_engine_refuses_a_malformed_subset_list(subsets, word):
    with pytest.raises(ValueError, match=word):
        _bare_job().enable_subset_exports(subsets)
    j = _bare_job()
    with pytest.raises(ValueError, match="decoders"):
        j.enable_subset_exports([(0,), (1,)], decoders=[(0,)])
    with pytest.raises(ValueError, match="decoders"):
        j.enable_subset_exports([(0,)], decoders=[(3,)])
    assert j.sub_masks is None


def test_a_bit_beyond_four_experts_is_refused():
    with pytest.raises(ValueError, match="experts 0..3"):
        _bare_job((40, 40, 40, 120)).enable_subset_exports([(0, 4)])


def test_forward_subsets_wants_the_subsets_first():
    js = object.__new__(JobSet)
    js.jobs, js.wide = [_bare_job()], False
    with pytest.raises(ValueError, match="enable_subset_exports"):
        js.forward_subsets()
