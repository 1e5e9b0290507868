"""CPU-side checks of the normative z-map entry points (nm_cohort_moments, nm_normative_z, nm_cohort_cov, nm_mahalanobis): they
are exported and declared, the pointer-table entry has the C layout, the #defines agree with _lib, their argument errors come
back before a device is touched, metrics.* refuse malformed inputs with ValueErrors before they ask for a GPU, and the sweep's
parsers know the new flags.  No compute calls: no GPU here."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest
import torch

from multi_modal_normative_modeling_amd import _lib, metrics

ROOT = Path(__file__).resolve().parent.parent
NAMES = ("nm_cohort_moments", "nm_normative_z", "nm_cohort_cov", "nm_mahalanobis")


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
        assert re.search(r"\bint\s+%s\s*\(const nm_norm_set_t\* sets_dev, int n_sets," % name, header), name
    assert lib.nm_version() == 11
    assert metrics.COHORT_MOMENTS_COLUMNS == ("mean", "sd", "var", "n_ref", "min", "max", "n_nonfinite", "status")
    assert metrics.NORMATIVE_ROW_COLUMNS == ("n_hi", "n_lo", "mean_z", "mean_abs_z", "max_z", "argmax_z", "n_valid", "status")
    assert metrics.NORMATIVE_COL_COLUMNS == ("n_hi_x", "n_lo_x", "n_hi_y", "n_lo_y", "n_x", "n_y", "mean_z_x", "mean_z_y")
    for cols in (metrics.COHORT_MOMENTS_COLUMNS, metrics.NORMATIVE_ROW_COLUMNS, metrics.NORMATIVE_COL_COLUMNS):
        assert len(cols) == _lib.NM_METRICS_STRIDE


def test_table_entry_has_the_c_layout():
    S = _lib.NmNormSet
    assert C.sizeof(S) == 56
    assert [S.x.offset, S.sub.offset, S.group.offset, S.z.offset, S.rows.offset, S.pitch.offset, S.sub_pitch.offset,
            S.z_pitch.offset, S.row_off.offset, S.pad.offset] == [0, 8, 16, 24, 32, 36, 40, 44, 48, 52]
    src = (ROOT / "multi_modal_normative_modeling_amd" / "csrc" / "nm_normative.inc").read_text()
    assert "static_assert(sizeof(nm_norm_set_t) == 56" in src


def test_defines_agree_with_the_binding():
    header = (ROOT / "include" / "nmhip.h").read_text()
    for name in ("NM_NORM_MAX_D", "NM_NORM_ROWS_PER_WG", "NM_WIDE_MAX_LATENT", "NM_METRICS_MAX_N", "NM_METRICS_STRIDE"):
        m = re.search(r"^#define\s+%s\s+(\d+)\b" % name, header, flags=re.M)
        assert m and int(m.group(1)) == getattr(_lib, name), name
    assert (_lib.NM_NORM_MAX_D, _lib.NM_NORM_ROWS_PER_WG) == (4096, 32)


def test_argument_errors_come_first(lib):
    p = 4096                                                          # (any non-null address: the checks come first)
    E, N, L = _lib.NM_E_METRICS, _lib.NM_E_NULL, _lib.NM_E_LATENT
    big = _lib.NM_METRICS_MAX_N + 1
    f = lib.nm_cohort_moments
    assert f(None, 1, 10, 100, 1, p, None) == N and f(p, 1, 10, 100, 1, None, None) == N
    for args in ((0, 10, 100, 1), (-1, 10, 100, 1), (1, 0, 100, 1), (1, 10, 0, 1), (1, 10, big, 1), (1, 10, 100, 2), (1, 10, 100, -1)):
        assert f(p, *args, p, None) == E, args
    f = lib.nm_normative_z
    good = dict(sets=p, n_sets=1, D=10, max_rows=100, mom=p, n_mom=1, ref=None, thr=1.96, rows=p, cols=p)

    def z(**kw):
        a = {**good, **kw}
        return f(a["sets"], a["n_sets"], a["D"], a["max_rows"], a["mom"], a["n_mom"], a["ref"], a["thr"], a["rows"], a["cols"], None)

    for k in ("sets", "mom", "rows", "cols"):
        assert z(**{k: None}) == N, k
    for kw in (dict(n_sets=0), dict(D=0), dict(D=_lib.NM_NORM_MAX_D + 1), dict(max_rows=0), dict(max_rows=big), dict(n_mom=0),
               dict(thr=0.0), dict(thr=-1.0), dict(thr=float("nan")), dict(thr=float("inf"))):
        assert z(**kw) == E, kw
    f = lib.nm_cohort_cov
    assert f(None, 1, 10, 100, 0.0, p, p, p, None) == N
    for k in range(3):
        outs = [p, p, p]; outs[k] = None
        assert f(p, 1, 10, 100, 0.0, *outs, None) == N
    for Z in (0, -1, _lib.NM_WIDE_MAX_LATENT + 1):
        assert f(p, 1, Z, 100, 0.0, p, p, p, None) == L, Z
    for args in ((0, 10, 100, 0.0), (1, 10, 0, 0.0), (1, 10, big, 0.0), (1, 10, 100, -1e-3), (1, 10, 100, float("nan")),
                 (1, 10, 100, float("inf"))):
        assert f(p, *args, p, p, p, None) == E, args
    f = lib.nm_mahalanobis
    assert f(None, 1, 10, 100, p, p, p, 1, None, p, p, None) == N
    for k in range(3):
        ins = [p, p, p]; ins[k] = None
        assert f(p, 1, 10, 100, *ins, 1, None, p, p, None) == N
    assert f(p, 1, 10, 100, p, p, p, 1, None, None, p, None) == N and f(p, 1, 10, 100, p, p, p, 1, None, p, None, None) == N
    for Z in (0, _lib.NM_WIDE_MAX_LATENT + 1):
        assert f(p, 1, Z, 100, p, p, p, 1, None, p, p, None) == L
    for n_sets, max_rows, n_f in ((0, 100, 1), (1, 0, 1), (1, big, 1), (1, 100, 0)):
        assert f(p, n_sets, 10, max_rows, p, p, p, n_f, None, p, p, None) == E


def test_value_errors_before_a_gpu_is_asked_for():
    x, g = torch.zeros(6, 5), torch.zeros(6, dtype=torch.int32)
    mom = torch.zeros(1, 5, 8, dtype=torch.float64)
    tables = [
        dict(mats=[], groups=[]), dict(mats=[x], groups=[g, g]), dict(mats=[x.double()], groups=[g]),
        dict(mats=[x[0]], groups=[g[:1]]), dict(mats=[x, torch.zeros(6, 4)], groups=[g, g]), dict(mats=[x], groups=[g[:5]]),
        dict(mats=[torch.zeros(6, 10)[:, ::2]], groups=[g]),
        dict(mats=[torch.zeros(_lib.NM_METRICS_MAX_N + 1, 2)], groups=[torch.zeros(_lib.NM_METRICS_MAX_N + 1)]),
    ]
    subs = [dict(mats=[x], groups=[g], sub=[x, x]), dict(mats=[x], groups=[g], sub=[x.double()]),
            dict(mats=[x], groups=[g], sub=[torch.zeros(5, 5)]), dict(mats=[x], groups=[g], sub=[np.zeros((6, 5), np.float32)])]
    for kw in tables + subs + [dict(mats=[x], groups=[g], ddof=2), dict(mats=[x], groups=[g], ddof=-1), dict(mats=[x], groups=[g], ddof=0.5)]:
        with pytest.raises(ValueError):
            metrics.cohort_moments(**kw)
    bad_z = [dict(thr=0.0), dict(thr=-2.0), dict(thr=float("nan")), dict(thr=float("inf")), dict(moments=mom.float()),
             dict(moments=torch.zeros(1, 4, 8, dtype=torch.float64)), dict(moments=mom[0]), dict(ref_of=[0, 0]), dict(ref_of=[1]),
             dict(ref_of=[-1]), dict(mats=[x, x], groups=[g, g])]                     # (two sets, one moments row, no ref_of)
    for kw in tables + subs + [{**dict(mats=[x], groups=[g]), **b} for b in bad_z]:
        with pytest.raises(ValueError):
            metrics.normative_z(**{"moments": mom, **kw})
    wide = torch.zeros(3, _lib.NM_NORM_MAX_D + 1)
    with pytest.raises(ValueError):
        metrics.normative_z([wide], [g[:3]], torch.zeros(1, _lib.NM_NORM_MAX_D + 1, 8, dtype=torch.float64))
    for kw in tables + [dict(mats=[x], groups=[g], ridge=-1e-9), dict(mats=[x], groups=[g], ridge=float("nan")),
                        dict(mats=[torch.zeros(4, _lib.NM_WIDE_MAX_LATENT + 1)], groups=[g[:4]])]:
        with pytest.raises(ValueError):
            metrics.cohort_cov(**kw)
    mean, chol, st = torch.zeros(1, 5, dtype=torch.float64), torch.zeros(1, 5, 5, dtype=torch.float64), torch.zeros(1, dtype=torch.int32)
    bad_m = [dict(mats=[]), dict(mats=[x.double()]), dict(mats=[torch.zeros(4, _lib.NM_WIDE_MAX_LATENT + 1)]), dict(mean=mean.float()),
             dict(chol=chol[:, :4]), dict(status=st.long()), dict(mats=[x, x]), dict(ref_of=[2]), dict(mats=[torch.zeros(6, 4)])]
    for b in bad_m:
        with pytest.raises(ValueError):
            metrics.mahalanobis(**{**dict(mats=[x], mean=mean, chol=chol, status=st), **b})
    if not torch.cuda.is_available():                                 # well-formed input, no GPU: no quiet host path
        for call in (lambda: metrics.cohort_moments([x], [g], sub=[x]), lambda: metrics.normative_z([x], [g], mom),
                     lambda: metrics.cohort_cov([x], [g], ridge=1e-3), lambda: metrics.mahalanobis([x], mean, chol, st)):
            with pytest.raises(_lib.NmError):
                call()


def test_pointer_table_reads_views_where_they_lie():
    buf, loc = torch.zeros(40, 12), torch.zeros(40, 16)
    g = torch.zeros(40, dtype=torch.int32)
    views = [buf[:, :9], buf[5:31, :9], buf[7:8, :9], buf[:0, :9]]
    subs = [loc[:, :9], loc[5:31, :9], loc[7:8, :9], loc[:0, :9]]
    zs = [torch.zeros(len(v), 9) for v in views]
    table = metrics._norm_table(views, [g[:len(v)] for v in views], subs, zs)
    assert [t.x for t in table] == [buf.data_ptr(), buf.data_ptr() + 5 * 12 * 4, buf.data_ptr() + 7 * 12 * 4, None]
    assert [t.sub for t in table] == [loc.data_ptr(), loc.data_ptr() + 5 * 16 * 4, loc.data_ptr() + 7 * 16 * 4, None]
    assert [t.rows for t in table] == [40, 26, 1, 0] and [t.row_off for t in table] == [0, 40, 66, 67]
    assert [t.pitch for t in table] == [12, 12, 9, 9] and [t.sub_pitch for t in table] == [16, 16, 9, 0]
    assert [t.z_pitch for t in table] == [9, 9, 9, 0] and table[0].z == zs[0].data_ptr() and table[3].z is None
    bare = metrics._norm_table(views)
    assert all(t.sub is None and t.z is None and t.group is None for t in bare) and C.sizeof(bare) == 4 * 56


def test_sweep_parsers_know_the_new_flags(capsys):
    from multi_modal_normative_modeling_amd import sweep
    with pytest.raises(SystemExit) as e:
        sweep.main_test(["--help"])
    assert e.value.code == 0
    text = capsys.readouterr().out
    for flag in ("--normative {squared,signed}", "--z-thr", "--mahalanobis", "--ridge"):
        assert flag in text, flag
    with pytest.raises(SystemExit) as e:
        sweep.main_analysis(["--help"])
    assert e.value.code == 0
    assert "{reconstruction,latent,extreme,zmean,mahalanobis}" in capsys.readouterr().out
    refused = [(["--normative", "squared"], "--normative needs --roi-effect"),
               (["--roi-effect", "--normative", "cubed"], "invalid choice"),
               (["--roi-effect", "--normative", "signed", "--z-thr", "0"], "--z-thr must be finite and > 0"),
               (["--mahalanobis"], "--mahalanobis needs --latent"),
               (["--latent", "--mahalanobis", "--ridge", "-1"], "--ridge must be finite and >= 0")]
    for argv, why in refused:                                          # (refused by the parser: before a cohort or a GPU is asked for)
        with pytest.raises(SystemExit) as e:
            sweep.main_test(["--models-dir", "nowhere"] + argv)
        assert e.value.code == 2 and why in capsys.readouterr().err, argv
    with pytest.raises(SystemExit):
        sweep.main_analysis(["--models-dir", "nowhere", "--score", "zscore"])
    # the library functions refuse the same before any job is built
    with pytest.raises(ValueError):
        sweep.test_folds([], None, [], ["a"], "poe", "cpu", normative="squared")
    with pytest.raises(ValueError):
        sweep.test_folds([], None, [], ["a"], "poe", "cpu", roi_effect=True, normative="cubed")
    with pytest.raises(ValueError):
        sweep.test_folds([], None, [], ["a"], "poe", "cpu", roi_effect=True, normative="signed", z_thr=float("nan"))
    with pytest.raises(ValueError):
        sweep.latent_folds([], None, [], ["a"], "poe", "cpu", mahalanobis=True, ridge=-1.0)
