"""CPU-side checks of the normative centile entry points (nm_cohort_quantiles, nm_normative_centile_workspace,
nm_normative_centile): they are exported and declared, the #define agrees with _lib, their argument errors come back before a
device is touched, the workspace query is monotone, metrics.* refuse malformed inputs with ValueErrors before they ask for a
GPU, and the sweep's parsers know the new flags.  No compute calls: no GPU here."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest
import torch

from multi_modal_normative_modeling_amd import _lib, io, metrics

ROOT = Path(__file__).resolve().parent.parent
NAMES = ("nm_cohort_quantiles", "nm_normative_centile_workspace", "nm_normative_centile")


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
    assert re.search(r"\bint\s+nm_cohort_quantiles\s*\(const nm_norm_set_t\* sets_dev, int n_sets, int D, int max_rows, "
                     r"const double\* probs_host, int n_q,", header)
    assert re.search(r"\bsize_t\s+nm_normative_centile_workspace\s*\(int total_rows, int D\);", header)
    assert re.search(r"\bint\s+nm_normative_centile\s*\(const nm_norm_set_t\* sets_dev, int n_sets, int D, int max_rows, "
                     r"int total_rows, const int32_t\* ref_of,", header)
    assert lib.nm_version() == 11
    m = re.search(r"^#define\s+NM_CENT_MAX_Q\s+(\d+)\b", header, flags=re.M)
    assert m and int(m.group(1)) == _lib.NM_CENT_MAX_Q == 32
    assert C.sizeof(_lib.NmNormSet) == 56                               # (the table entry is the normative z-map's, unchanged)
    assert metrics.COHORT_QUANTILE_COLUMNS == ("median", "mad", "q1", "q3", "iqr", "n_ref", "n_nonfinite", "status")
    assert metrics.CENTILE_ROW_COLUMNS == ("n_hi", "n_lo", "mean_pct", "mean_abs_dev", "max_pct", "argmax_pct", "n_valid", "status")
    assert metrics.CENTILE_COL_COLUMNS == ("n_hi_x", "n_lo_x", "n_hi_y", "n_lo_y", "n_x", "n_y", "mean_pct_x", "mean_pct_y")
    for cols in (metrics.COHORT_QUANTILE_COLUMNS, metrics.CENTILE_ROW_COLUMNS, metrics.CENTILE_COL_COLUMNS):
        assert len(cols) == _lib.NM_METRICS_STRIDE == 8
    assert metrics.NORMATIVE_CENTILE_WORKSPACE_CAP == 1 << 30
    src = (ROOT / "multi_modal_normative_modeling_amd" / "csrc" / "nm_metrics.hip").read_text()
    assert '#include "nm_centile.inc"' in src
    inc = (ROOT / "multi_modal_normative_modeling_amd" / "csrc" / "nm_centile.inc").read_text()
    assert "#pragma clang fp contract(off)" in inc and "atomic" not in inc.replace("No atomics", "")


def test_workspace_query(lib):
    ws = lib.nm_normative_centile_workspace
    for args in ((-1, 10), (10, 0), (10, -3), (-5, -5)):
        assert ws(*args) == 0, args                                     # arguments no launch accepts
    last = 0
    for rows in (0, 1, 2, 127, 128, 129, 1000, 8192, 300000):
        got = ws(rows, 379)
        assert got >= rows * 379 * 2 and got > 0 and got >= last, rows
        last = got
    last = 0
    for D in (1, 2, 63, 64, 65, 1137, 4096, 100000):
        got = ws(1064, D)
        assert got >= 1064 * D * 2 and got >= last, D
        last = got
    assert ws(2 ** 31 - 1, 2 ** 31 - 1) >= (2 ** 31 - 1) ** 2 * 2       # (size_t arithmetic: no 32-bit wrap)


def test_argument_errors_come_first(lib):
    p = 4096                                                            # (any non-null address: the checks come first)
    E, N = _lib.NM_E_METRICS, _lib.NM_E_NULL
    big = _lib.NM_METRICS_MAX_N + 1
    probs = (C.c_double * 3)(0.0, 0.5, 1.0)
    good = dict(sets=p, n_sets=1, D=10, max_rows=100, probs=probs, n_q=3, q=p, st=p)

    def quant(**kw):
        a = {**good, **kw}
        return lib.nm_cohort_quantiles(a["sets"], a["n_sets"], a["D"], a["max_rows"], a["probs"], a["n_q"], a["q"], a["st"], None)

    for k in ("sets", "st", "probs", "q"):
        assert quant(**{k: None}) == N, k
    for kw in (dict(n_sets=0), dict(n_sets=-1), dict(D=0), dict(max_rows=0), dict(max_rows=big), dict(n_q=-1),
               dict(n_q=_lib.NM_CENT_MAX_Q + 1), dict(probs=(C.c_double * 3)(0.0, 1.5, 1.0)), dict(probs=(C.c_double * 3)(-1e-9, 0.5, 1.0)),
               dict(probs=(C.c_double * 3)(0.0, float("nan"), 1.0)), dict(n_sets=2 ** 22, D=2 ** 12)):
        assert quant(**kw) == E, kw
    need = lib.nm_normative_centile_workspace(50, 10)
    good = dict(sets=p, n_sets=1, D=10, max_rows=100, total=50, ref=None, tail=2.5, loo=0, ws=p, ws_bytes=need, rows=p, cols=p)

    def cent(**kw):
        a = {**good, **kw}
        return lib.nm_normative_centile(a["sets"], a["n_sets"], a["D"], a["max_rows"], a["total"], a["ref"], a["tail"], a["loo"],
                                        a["ws"], a["ws_bytes"], a["rows"], a["cols"], None)

    for k in ("sets", "ws", "rows", "cols"):
        assert cent(**{k: None}) == N, k
    for kw in (dict(n_sets=0), dict(D=0), dict(max_rows=0), dict(max_rows=big), dict(total=-1), dict(tail=0.0), dict(tail=50.0),
               dict(tail=-1.0), dict(tail=float("nan")), dict(tail=float("inf")), dict(loo=2), dict(loo=-1), dict(ws_bytes=need - 1),
               dict(ws_bytes=0), dict(n_sets=2 ** 22, D=2 ** 12, ws_bytes=2 ** 40)):
        assert cent(**kw) == E, kw


def test_value_errors_before_a_gpu_is_asked_for():
    x, g = torch.zeros(6, 5), torch.zeros(6, dtype=torch.int32)
    tables = [
        dict(mats=[], groups=[]), dict(mats=[x], groups=[g, g]), dict(mats=[x.double()], groups=[g]),
        dict(mats=[x[0]], groups=[g[:1]]), dict(mats=[x, torch.zeros(6, 4)], groups=[g, g]), dict(mats=[x], groups=[g[:5]]),
        dict(mats=[torch.zeros(6, 10)[:, ::2]], groups=[g]),
        dict(mats=[torch.zeros(_lib.NM_METRICS_MAX_N + 1, 2)], groups=[torch.zeros(_lib.NM_METRICS_MAX_N + 1)]),
        dict(mats=[x], groups=[g], sub=[x, x]), dict(mats=[x], groups=[g], sub=[x.double()]), dict(mats=[x], groups=[g], sub=[torch.zeros(5, 5)]),
    ]
    base = dict(mats=[x], groups=[g])
    bad_q = [dict(probs=[1.5]), dict(probs=[-0.1]), dict(probs=[float("nan")]), dict(probs=[0.5] * (_lib.NM_CENT_MAX_Q + 1))]
    for kw in tables + [{**base, **b} for b in bad_q]:
        with pytest.raises(ValueError):
            metrics.cohort_quantiles(**kw)
    bad_c = [dict(tail=0.0), dict(tail=50.0), dict(tail=-2.0), dict(tail=float("nan")), dict(tail=float("inf")), dict(loo=2),
             dict(loo="yes"), dict(ref_of=[0, 0]), dict(ref_of=[1]), dict(ref_of=[-2])]
    for kw in tables + [{**base, **b} for b in bad_c]:
        with pytest.raises(ValueError):
            metrics.normative_centile(**kw)
    for bad in (dict(stats=torch.zeros(1, 5, 8)), dict(stats=torch.zeros(5, 8, dtype=torch.float64)),
                dict(stats=torch.zeros(1, 5, 7, dtype=torch.float64)), dict(stats=np.zeros((1, 5, 8))),
                dict(stats=torch.zeros(1, 5, 8, dtype=torch.float64), scale=0.0),
                dict(stats=torch.zeros(1, 5, 8, dtype=torch.float64), scale=float("inf"))):
        with pytest.raises(ValueError):
            metrics.robust_moments(**bad)
    assert metrics._centile_ref_check([-1, 0, 1], 3) == [-1, 0, 1] and metrics._centile_ref_check(None, 2) == [0, 1]
    if not torch.cuda.is_available():                                   # well-formed input, no GPU: no quiet host path
        for call in (lambda: metrics.cohort_quantiles([x], [g], sub=[x]), lambda: metrics.cohort_quantiles([x], [g], ()),
                     lambda: metrics.normative_centile([x, x], [g, g], ref_of=[-1, 0], loo=True)):
            with pytest.raises(_lib.NmError):
                call()


def test_csv_writers(tmp_path):
    import pandas as pd
    cov = pd.DataFrame({"participant_id": ["a", "b", "c"], "DIA": [1, 0, 1], "AGE": [20.0, 30.0, 40.0], "PTGENDER": [0, 1, 0]})
    rois = ["r0", "r1"]
    pct, rows, cols = np.full((3, 2), 50.0, np.float32), np.zeros((3, 8)), np.ones((2, 8))
    q, st = np.arange(4.0).reshape(2, 2), np.zeros((2, 8))
    paths = io.write_centile_csvs(tmp_path, "m", cov, rois, pct, rows, cols, (0.05, 0.5), q, st)
    assert sorted(p.name for p in paths.values()) == ["centile_curve_m.csv", "centile_map_m.csv", "centile_pct_m.csv", "centile_subject_m.csv"]
    assert list(pd.read_csv(paths["curve"]).columns) == ["ROI", "q_0.05", "q_0.5"] + list(metrics.COHORT_QUANTILE_COLUMNS)
    assert list(pd.read_csv(paths["map"]).columns) == ["ROI"] + list(metrics.CENTILE_COL_COLUMNS)
    assert list(pd.read_csv(paths["subject"]).columns)[-8:] == list(metrics.CENTILE_ROW_COLUMNS)
    assert list(pd.read_csv(paths["pct"]).columns)[-2:] == rois and len(pd.read_csv(paths["pct"])) == 3
    with pytest.raises(ValueError):
        io.write_centile_csvs(tmp_path, "m", cov, rois, pct, rows, cols, (0.05,), q, st)


def test_sweep_parsers_know_the_new_flags(capsys):
    from multi_modal_normative_modeling_amd import sweep
    with pytest.raises(SystemExit) as e:
        sweep.main_test(["--help"])
    assert e.value.code == 0
    text = capsys.readouterr().out
    for flag in ("--centile {squared,signed}", "--tail", "--quantiles P [P ...]", "--centile-loo", "--robust", "--normative {squared,signed}"):
        assert flag in text, flag
    with pytest.raises(SystemExit) as e:
        sweep.main_analysis(["--help"])
    assert e.value.code == 0
    text = capsys.readouterr().out
    assert "--centile-score {tails,depth}" in text and "{reconstruction,latent,extreme,zmean,mahalanobis}" in text
    refused = [(["--centile", "squared"], "--centile needs --roi-effect"),
               (["--roi-effect", "--centile", "cubed"], "invalid choice"),
               (["--roi-effect", "--centile", "signed", "--tail", "0"], "--tail must lie inside (0, 50)"),
               (["--roi-effect", "--centile", "signed", "--tail", "50"], "--tail must lie inside (0, 50)"),
               (["--roi-effect", "--centile", "signed", "--quantiles", "0.5", "1.5"], "--quantiles"),
               (["--roi-effect", "--centile-loo"], "--centile-loo needs --centile"),
               (["--roi-effect", "--robust"], "--robust needs --normative")]
    for argv, why in refused:                                           # (refused by the parser: before a cohort or a GPU is asked for)
        with pytest.raises(SystemExit) as e:
            sweep.main_test(["--models-dir", "nowhere"] + argv)
        assert e.value.code == 2 and why in capsys.readouterr().err, argv
    for argv, why in ((["--centile-score", "tails", "--score", "latent"], "does not go with --score"),
                      (["--centile-score", "width"], "invalid choice"),
                      (["--centile-score", "depth", "--roi"], "does not go with --roi")):
        with pytest.raises(SystemExit) as e:
            sweep.main_analysis(["--models-dir", "nowhere"] + argv)
        assert e.value.code == 2 and why in capsys.readouterr().err, argv
    # the library function refuses the same before any job is built
    for kw in (dict(centile="squared"), dict(roi_effect=True, centile="cubed"), dict(roi_effect=True, centile="signed", tail=float("nan")),
               dict(roi_effect=True, centile="signed", tail=60.0), dict(roi_effect=True, centile="squared", quantiles=(0.5, 2.0)),
               dict(roi_effect=True, robust=True)):
        with pytest.raises(ValueError):
            sweep.test_folds([], None, [], ["a"], "poe", "cpu", **kw)
