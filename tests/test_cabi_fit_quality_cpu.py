"""CPU-side checks of the model-fit entry points (nm_fit_quality, nm_fit_rank): they are exported and declared, the
pointer-table entry has the C layout, and every host-side refusal comes back with its code before a device is touched.  No
compute calls: no GPU here."""
import ctypes as C
import re
from pathlib import Path

import pytest

from multi_modal_normative_modeling_amd import _lib, metrics

ROOT = Path(__file__).resolve().parent.parent
NAMES = ("nm_fit_quality", "nm_fit_rank")


@pytest.fixture(scope="module")
def lib():
    if not _lib.LIB_PATH.exists():
        import __graft_entry__ as ge
        ge.build()
    return _lib.load()


def test_symbols_are_exported_and_declared(lib):
    header = (ROOT / "include" / "nmhip.h").read_text()
    for name in NAMES:
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name)
        assert re.search(r"\bint\s+%s\s*\(const nm_fit_set_t\* sets_dev, int n_sets, int D, int max_rows," % name, header), name
    assert lib.nm_version() == 11                                     # (a new entry point, no change to an old one)
    assert metrics.FIT_COLUMNS == ("rho", "p_rho", "smse", "expv", "msll", "rmse", "n_obs", "status")
    assert metrics.CALIBRATION_COLUMNS == ("bias", "mae", "mean_z", "sd_z", "skew_z", "kurt_z", "coverage", "n_var")
    assert metrics.FIT_RANK_COLUMNS == ("spearman", "p_spearman", "t_spearman", "n_obs", "n_tied_y", "n_tied_loc", "reserved", "status")
    for cols in (metrics.FIT_COLUMNS, metrics.CALIBRATION_COLUMNS, metrics.FIT_RANK_COLUMNS):
        assert len(cols) == _lib.NM_METRICS_STRIDE
    assert "< 2^63" in header                                         # the int64 bound at n = 8192 is stated


def test_table_entry_has_the_c_layout():
    S = _lib.NmFitSet
    assert C.sizeof(S) == 56
    assert [S.x.offset, S.loc.offset, S.var.offset, S.col_var.offset, S.group.offset, S.rows.offset, S.pitch.offset,
            S.loc_pitch.offset, S.var_pitch.offset] == [0, 8, 16, 24, 32, 40, 44, 48, 52]
    src = (ROOT / "multi_modal_normative_modeling_amd" / "csrc" / "nm_fit.inc").read_text()
    assert "static_assert(sizeof(nm_fit_set_t) == 56" in src
    assert '#include "nm_fit.inc"' in (ROOT / "multi_modal_normative_modeling_amd" / "csrc" / "nm_metrics.hip").read_text()


def test_argument_errors_come_first(lib):
    p = 4096                                                          # (any non-null address: the checks come first)
    E, N = _lib.NM_E_METRICS, _lib.NM_E_NULL
    big = _lib.NM_METRICS_MAX_N + 1
    good = dict(sets=p, n_sets=1, D=10, max_rows=100, mom=p, n_mom=1, ref=p, thr=1.96, fit=p, cal=p)

    def q(**kw):
        a = {**good, **kw}
        return lib.nm_fit_quality(a["sets"], a["n_sets"], a["D"], a["max_rows"], a["mom"], a["n_mom"], a["ref"], a["thr"],
                                  a["fit"], a["cal"], None)

    for k in ("sets", "fit", "cal"):
        assert q(**{k: None}) == N, k
    assert q(mom=None) == N                                           # ref_of without moments
    for kw in (dict(n_sets=0), dict(n_sets=-1), dict(D=0), dict(D=-3), dict(max_rows=0), dict(max_rows=big), dict(n_mom=0),
               dict(n_mom=-1), dict(thr=0.0), dict(thr=-1.0), dict(thr=float("nan")), dict(thr=float("inf")),
               dict(mom=None, ref=None, n_sets=0), dict(mom=None, ref=None, thr=0.0)):
        assert q(**kw) == E, kw
    f = lib.nm_fit_rank
    assert f(None, 1, 10, 100, p, None) == N and f(p, 1, 10, 100, None, None) == N
    for args in ((0, 10, 100), (-1, 10, 100), (1, 0, 100), (1, 10, 0), (1, 10, big), (1 << 20, 1 << 12, 100)):
        assert f(p, *args, p, None) == E, args
