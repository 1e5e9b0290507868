"""nm_train_steps_head_split's host side, no GPU: the symbol in the header, the ctypes table and the built library; the
argument refusals that are decided before anything asks a device; the hand-off registry; JobSet's pick of the number of
workgroups per head model against a stubbed CU count."""
import ctypes as C
import re
import types
from pathlib import Path

import pytest

from multi_modal_normative_modeling_amd import _lib, engine

ROOT = Path(__file__).resolve().parent.parent
SYM = "nm_train_steps_head_split"


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    return _lib.load()


def test_symbol_declared_exported_and_built(lib):
    header = (ROOT / "include" / "nmhip.h").read_text()
    declared = set(re.findall(r"\b(nm_[a-z_0-9]+)\s*\(", header))
    assert SYM in declared
    assert SYM in _lib.EXPORTED_SYMBOLS
    assert hasattr(lib, SYM)
    assert len(getattr(lib, SYM).argtypes) == 7
    # the one-workgroup entry keeps its signature
    assert re.search(r"int nm_train_steps_head\(const nm_job_t\* jobs_dev, int n_jobs, int step0, int n_steps, int flags, void\* stream\);", header)
    assert len(lib.nm_train_steps_head.argtypes) == 6


def test_refusals_before_any_device_access(lib):
    """NM_E_NULL / NM_E_GEOMETRY in the order of the entry's checks; a non-NULL jobs pointer is never read on these paths and
    no device is asked for its CU count."""
    fake = C.c_void_p(0x1000)

    def launch(jobs=fake, n_jobs=5, parts=3, step0=0, n_steps=1, flags=0):
        return lib.nm_train_steps_head_split(jobs, n_jobs, parts, step0, n_steps, flags, None)

    assert launch(jobs=None) == _lib.NM_E_NULL
    assert launch(parts=1) == _lib.NM_E_GEOMETRY
    assert launch(parts=0) == _lib.NM_E_GEOMETRY
    assert launch(parts=_lib.NM_MAX_MOD + 1) == _lib.NM_E_GEOMETRY
    assert _lib.NM_MAX_MOD + 1 == 9
    assert launch(n_jobs=0) == _lib.NM_E_GEOMETRY
    assert launch(n_steps=0) == _lib.NM_E_GEOMETRY
    assert launch(step0=-1) == _lib.NM_E_GEOMETRY
    assert launch(flags=_lib.NM_F_GRADS, n_steps=2) == _lib.NM_E_GEOMETRY
    for st in (_lib.NM_E_NULL, _lib.NM_E_GEOMETRY, _lib.NM_E_RESIDENCY):
        assert lib.nm_status_string(st)


def test_handoff_registry_names_the_split_switch():
    assert engine._HANDOFF_KINDS[SYM] == "split"
    assert engine._HANDOFF_KINDS["nm_launch_split"] == "split"              # the launches before it keep their kinds
    assert engine._HANDOFF_KINDS["nm_launch_rowsplit"] == "rowsplit"


def _stub_set(n, M=3, cus=256, wide=False, layers=(), counts=None):
    """A JobSet of stand-in jobs (what the picks read of a job) on a chip of `cus` CUs."""
    counts = [M] * n if counts is None else counts
    jobs = [types.SimpleNamespace(kmods=[None] * m, spec=types.SimpleNamespace(wide=wide, classifier_layers=tuple(layers)),
                                  device="cpu") for m in counts]
    js = engine.JobSet(jobs)
    js.__dict__["_cus"] = cus
    return js


def test_pick_of_parts(lib, monkeypatch):
    monkeypatch.delenv("NMHIP_SPLIT", raising=False)
    assert _stub_set(1).head_split_parts() == 3
    assert _stub_set(5).head_split_parts() == 3                             # 8 x 3 = 24 workgroups
    assert _stub_set(20).head_split_parts() == 3                            # 24 x 3 = 72
    assert _stub_set(5, M=6, layers=(128, 64, 32)).head_split_parts() == 6  # 8 x 6 = 48
    assert _stub_set(20, M=6, layers=(128, 64, 32)).head_split_parts() == 6 # 24 x 6 = 144
    assert _stub_set(40, M=6, layers=(128, 64, 32)).head_split_parts() == 6 # 40 x 6 = 240
    assert _stub_set(41, M=6, layers=(128, 64, 32)).head_split_parts() == 1 # 48 x 6 = 288 > 256
    assert _stub_set(80).head_split_parts() == 3 and _stub_set(88).head_split_parts() == 1
    assert _stub_set(20, cus=64).head_split_parts() == 1                    # a smaller chip
    # what the persistent head kernel does not run at all, or not split
    assert _stub_set(5, wide=True).head_split_parts() == 1
    assert _stub_set(5, M=6, layers=(256, 128, 64)).head_split_parts() == 1
    assert _stub_set(5, M=6, layers=(128, 64, 32)).head_split_parts(fused=False) == 1
    assert _stub_set(0, counts=[3, 3, 2]).head_split_parts() == 1
    assert _stub_set(5, M=1).head_split_parts() == 1
    # the pick sits on top of split_parts(): the same switch turns both off
    for js in (_stub_set(5), _stub_set(20, M=6, layers=(128, 64, 32))):
        assert js.head_split_parts() == js.split_parts()
    monkeypatch.setenv("NMHIP_SPLIT", "0")                                  # (sweep --share-device sets it)
    assert _stub_set(5).head_split_parts() == 1
    assert _stub_set(5, M=6, layers=(128, 64, 32)).head_split_parts() == 1


def test_insisting_on_a_set_that_cannot_names_the_reason(lib, monkeypatch):
    monkeypatch.delenv("NMHIP_SPLIT", raising=False)
    assert _stub_set(5)._head_parts(True) == 3 and _stub_set(5)._head_parts(False) == 1 and _stub_set(5)._head_parts(None) == 3
    for js, fused, word in ((_stub_set(5, wide=True), True, "general-shape"),
                            (_stub_set(5, M=6, layers=(256, 128, 64)), True, "wider than 128"),
                            (_stub_set(5, M=6, layers=(128,)), False, "fused=False"),
                            (_stub_set(0, counts=[3, 2]), True, "differ"),
                            (_stub_set(88), True, "resident")):
        with pytest.raises(ValueError, match=word):
            js._head_parts(True, fused)
        assert js._head_parts(None, fused) == 1
