"""The mixed row-split launch's host side, no GPU: nm_rowsplit_groups (the group map of a launch whose jobs differ in their
number of modalities -- the reference's grid of 15 one-modality and 5 four-modality models, commands_list_deviation.sh:13-23),
the argument refusals of nm_launch_rowsplit_mixed that are decided before anything touches a device, JobSet's pick of k for
such a set, and the sweep's --one-launch switch."""
import ctypes as C
import re
import types
from pathlib import Path

import pytest

from multi_modal_normative_modeling_amd import _lib, engine, sweep

ROOT = Path(__file__).resolve().parent.parent
NEW = ("nm_launch_rowsplit_mixed", "nm_rowsplit_groups")


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    return _lib.load()


def test_symbols_declared_exported_and_built(lib):
    header = (ROOT / "include" / "nmhip.h").read_text()
    declared = set(re.findall(r"\b(nm_[a-z_0-9]+)\s*\(", header))
    for sym in NEW:
        assert sym in declared, sym
        assert sym in _lib.EXPORTED_SYMBOLS, sym
        assert hasattr(lib, sym), sym


def _groups(lib, counts, cap=128):
    arr = (C.c_int * max(len(counts), 1))(*counts)
    out = (C.c_int * max(cap, 1))(*([-7] * max(cap, 1)))
    n = lib.nm_rowsplit_groups(arr, len(counts), out, cap)
    return n, list(out)


def _unpack(e):
    return e & 0xFFFF, (e >> 16) & 0xFF, (e >> 24) & 0xFF          # job, part, the job's modality count


def test_group_map_of_the_grid(lib):
    """[1] * 15 + [4] * 5: 35 entries in set order, parts 0 .. M - 1 in order, each with its job's count, then 5 padding
    slots; nothing is written past the slots returned."""
    counts = [1] * 15 + [4] * 5
    n, out = _groups(lib, counts)
    assert n == 40
    want = [(j, m, M) for j, M in enumerate(counts) for m in range(M)]
    assert len(want) == 35
    assert [_unpack(e) for e in out[:35]] == want
    assert out[35:40] == [_lib.NM_RS_GROUP_PAD] * 5
    assert all(_unpack(e)[0] >= len(counts) for e in out[35:40])           # a padding slot names no job of the set
    assert out[40:] == [-7] * (len(out) - 40)
    # a permuted set: still set order
    counts = [4, 1, 2, 1, 3]
    n, out = _groups(lib, counts)
    assert n == 16
    assert [_unpack(e) for e in out[:11]] == [(j, m, M) for j, M in enumerate(counts) for m in range(M)]
    assert out[11:16] == [_lib.NM_RS_GROUP_PAD] * 5


def test_group_map_of_a_uniform_set_is_the_arithmetic_map(lib):
    """[3, 3, 3] -> group / 3, group % 3: what nm_launch_rowsplit's kernel computed from its one M."""
    n, out = _groups(lib, [3, 3, 3])
    assert n == 16
    assert [_unpack(e) for e in out[:9]] == [(g // 3, g % 3, 3) for g in range(9)]
    assert out[9:16] == [_lib.NM_RS_GROUP_PAD] * 7
    for M in (1, 2, 3, 4):
        for n_jobs in (1, 5, 8, 20, 128 // M):
            n, out = _groups(lib, [M] * n_jobs)
            assert n == (n_jobs * M + 7) // 8 * 8
            assert [_unpack(e) for e in out[:n_jobs * M]] == [(g // M, g % M, M) for g in range(n_jobs * M)]


def test_group_map_refusals(lib):
    assert _groups(lib, [1, 0, 2])[0] == _lib.NM_E_GEOMETRY
    assert _groups(lib, [1, _lib.NM_MAX_EXP + 1])[0] == _lib.NM_E_GEOMETRY
    assert _groups(lib, [1, -1])[0] == _lib.NM_E_GEOMETRY
    assert _groups(lib, [])[0] == _lib.NM_E_GEOMETRY
    assert _groups(lib, [4] * 32)[0] == 128                                  # the last set that fits
    assert _groups(lib, [4] * 32 + [1], cap=256)[0] == _lib.NM_E_RESIDENCY   # 129 groups -> 136 slots
    assert _groups(lib, [1] * 130, cap=256)[0] == _lib.NM_E_RESIDENCY
    assert _groups(lib, [1] * 15 + [4] * 5, cap=32)[0] == _lib.NM_E_GEOMETRY  # 40 slots do not fit 32
    n, out = _groups(lib, [1] * 15 + [4] * 5, cap=32)
    assert out == [-7] * 32                                                  # ... and nothing was written
    arr, out = (C.c_int * 2)(1, 1), (C.c_int * 8)()
    assert lib.nm_rowsplit_groups(None, 2, out, 8) == _lib.NM_E_NULL
    assert lib.nm_rowsplit_groups(arr, 2, None, 8) == _lib.NM_E_NULL
    for st in (_lib.NM_E_NULL, _lib.NM_E_GEOMETRY, _lib.NM_E_RESIDENCY):
        assert lib.nm_status_string(st)


def test_launch_refusals_before_any_device_access(lib):
    """The checks nm_launch_rowsplit makes before it asks for the CU count, in its order: the descriptor array, the counts,
    k, the flags.  (A non-NULL jobs pointer is never read on these paths.)"""
    train = _lib.NM_F_BACKWARD | _lib.NM_F_ADAM
    fake = C.c_void_p(0x1000)
    counts = (C.c_int * 3)(1, 4, 1)

    def launch(jobs=fake, n_jobs=3, job_M=counts, k=4, helpers=0, step0=0, n_steps=1, flags=train):
        return lib.nm_launch_rowsplit_mixed(jobs, n_jobs, job_M, k, helpers, step0, n_steps, flags, 0, None)

    assert launch(jobs=None) == _lib.NM_E_NULL
    assert launch(job_M=None) == _lib.NM_E_NULL
    assert launch(k=3) == _lib.NM_E_GEOMETRY
    assert launch(k=1) == _lib.NM_E_GEOMETRY
    assert launch(flags=_lib.NM_F_ADAM) == _lib.NM_E_GEOMETRY                    # no NM_F_BACKWARD
    assert launch(flags=_lib.NM_F_BACKWARD) == _lib.NM_E_GEOMETRY                # neither Adam nor gradients
    assert launch(flags=_lib.NM_F_BACKWARD | _lib.NM_F_GRADS, n_steps=2) == _lib.NM_E_GEOMETRY
    assert launch(n_jobs=0) == _lib.NM_E_GEOMETRY
    assert launch(step0=-1) == _lib.NM_E_GEOMETRY
    assert launch(job_M=(C.c_int * 3)(1, 0, 1)) == _lib.NM_E_GEOMETRY
    assert launch(job_M=(C.c_int * 3)(1, _lib.NM_MAX_EXP + 1, 1)) == _lib.NM_E_GEOMETRY
    many = (C.c_int * 130)(*([1] * 130))
    assert launch(n_jobs=130, job_M=many, k=2) == _lib.NM_E_RESIDENCY            # 136 slots: more than any map holds


def _stub_set(lib, counts, cus=256, ok=True):
    """A JobSet of stand-in jobs (what rowsplit_k / rowsplit_helpers read of a job), on a chip of `cus` CUs."""
    jobs = [types.SimpleNamespace(kmods=[None] * M, spec=types.SimpleNamespace(wide=False), device="cpu",
                                  rowsplit_ok=(lambda: ok)) for M in counts]
    js = engine.JobSet(jobs)
    js.__dict__["_cus"] = cus
    return js


def test_rowsplit_k_of_mixed_sets(lib, monkeypatch):
    monkeypatch.delenv("NMHIP_ROWSPLIT", raising=False)
    monkeypatch.delenv("NMHIP_RS_HELPERS", raising=False)
    grid = _stub_set(lib, [1] * 15 + [4] * 5)
    assert grid.rowsplit_k() == 1                           # the automatic pick of train() / grads(): as before
    assert grid.rowsplit_k(mixed=True) == 4                 # 35 groups -> 40 x 4 = 160 workgroups
    assert grid.rowsplit_helpers(4) == 2                    # 256 // 40 = 6 workgroups per group
    assert _stub_set(lib, [4] * 20 + [1] * 20).rowsplit_k(mixed=True) == 2     # 100 groups -> 104 x 2 = 208
    assert _stub_set(lib, [4] * 20 + [1] * 20).rowsplit_k() == 1
    assert _stub_set(lib, [4] * 30 + [1] * 10).rowsplit_k(mixed=True) == 1     # 130 groups
    assert _stub_set(lib, [1] * 15 + [4] * 5, ok=False).rowsplit_k(mixed=True) == 1
    # a uniform set: the same answer either way, today's rule
    for counts in ([3] * 20, [3] * 40, [3] * 96, [1] * 5):
        a, b = _stub_set(lib, counts).rowsplit_k(), _stub_set(lib, counts).rowsplit_k(mixed=True)
        assert a == b == {60: 4, 120: 2, 288: 1, 5: 4}[sum(counts)]
    assert _stub_set(lib, [3] * 5).rowsplit_helpers(4) == 12
    monkeypatch.setenv("NMHIP_ROWSPLIT", "2")
    assert grid.rowsplit_k(mixed=True) == 2
    monkeypatch.setenv("NMHIP_ROWSPLIT", "0")               # (bench.py --share-device, sweep --share-device)
    assert grid.rowsplit_k(mixed=True) == 1


def test_sweep_one_launch_switch_reaches_run_cells():
    """--one-launch auto passes nothing (the stand-in of tests/test_sweep_cpu.py has a fixed signature), on / off pass the
    keyword."""
    from tests.test_sweep_cpu import _stub_run_cells
    argv = ["-R", "HCPimage", "-P", "SM-T1w_sMRI", "UCA-gPoE", "-E", "3", "-K", "2", "-H", "64", "32", "7",
            "-Baselearningrate", "2e-4", "--subjects", "32"]
    seen = []

    def spy(*a, **kw):
        seen.append(kw.pop("one_launch", "absent"))
        return _stub_run_cells(*a, **kw)

    for extra, want in (([], "absent"), (["--one-launch", "auto"], "absent"), (["--one-launch", "on"], True),
                        (["--one-launch", "off"], False)):
        table = sweep.main(argv + extra, _run_cells=spy)
        assert table.shape == (4, sweep.N_METRICS)
        assert seen[-1] == want or (seen[-1] is want), (extra, seen[-1])
    assert sweep.main(argv, _run_cells=_stub_run_cells).shape == (4, sweep.N_METRICS)
    assert sweep.main(argv + ["--one-launch", "auto"], _run_cells=_stub_run_cells).shape == (4, sweep.N_METRICS)
    with pytest.raises(TypeError):
        sweep.main(argv + ["--one-launch", "on"], _run_cells=_stub_run_cells)
    with pytest.raises(SystemExit):
        sweep.main(argv + ["--one-launch", "maybe"], _run_cells=_stub_run_cells)
    import inspect
    assert inspect.signature(sweep.run_cells).parameters["one_launch"].default is None
