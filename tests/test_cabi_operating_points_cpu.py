"""CPU-side checks of nm_operating_points: both symbols are exported and declared with the header's prototypes, the header's
constants are _lib's, the rule row is mirrored, every status code comes back before a device is touched (and is one of the
existing codes), metrics.operating_points refuses malformed inputs with ValueErrors before it asks for a GPU, and `analysis`
lists the new flags and refuses their conflicts.  No compute calls: no GPU here."""
import ctypes as C
import re
from pathlib import Path

import pytest
import torch

from multi_modal_normative_modeling_amd import _lib, metrics, sweep

ROOT = Path(__file__).resolve().parent.parent


@pytest.fixture(scope="module")
def lib():
    if not _lib.LIB_PATH.exists():
        import __graft_entry__ as ge
        ge.build()
    return _lib.load()


def test_symbols_constants_and_columns(lib):
    header = (ROOT / "include" / "nmhip.h").read_text()
    for name in ("nm_operating_points_workspace", "nm_operating_points"):
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name)
    assert re.search(r"\bsize_t\s+nm_operating_points_workspace\s*\(int n_sets, int n_rules\)\s*;", header)
    assert re.search(r"\bint\s+nm_operating_points\s*\(const float\* scores, const int32_t\* labels, const int32_t\* offsets, "
                     r"int n_sets, int max_set,\s*const nm_op_rule_t\* rules, int n_rules, const int32_t\* select_of, int n_eval, "
                     r"const int32_t\* eval_of,\s*double at_spec, double at_sens, double max_fpr, void\* workspace, "
                     r"size_t workspace_bytes,\s*double\* rules_out, double\* summary_out, double\* grid_out, int G, void\* stream\)\s*;",
                     header)
    names = ("NM_OP_ROC", "NM_OP_F1", "NM_OP_PR", "NM_OP_COST", "NM_OP_EER", "NM_OP_F1MAX", "NM_OP_SPEC", "NM_OP_MAX_RULES",
             "NM_OP_MAX_GRID", "NM_OP_MAX_LINSPACE")
    for name in names:
        assert re.search(r"^#define\s+%s\s+%d\s*$" % (name, getattr(_lib, name)), header, flags=re.M), name
    assert sorted(getattr(_lib, n) for n in names[:7]) == list(range(7))
    assert (_lib.NM_OP_MAX_RULES, _lib.NM_OP_MAX_GRID) == (16, 1024)
    assert C.sizeof(_lib.NmOpRule) == 40 and len(lib.nm_operating_points.argtypes) == 20
    assert metrics.OPERATING_POINT_COLUMNS == ("threshold", "accuracy", "recall", "specificity", "tp", "fp", "objective", "status")
    assert metrics.ROC_SUMMARY_COLUMNS == ("roc_auc", "average_precision", "pauc", "sens_at_spec", "spec_at_sens", "n_thresholds",
                                           "n_pos", "n_neg")
    assert len(metrics.OPERATING_POINT_COLUMNS) == len(metrics.ROC_SUMMARY_COLUMNS) == _lib.NM_METRICS_STRIDE == 8
    assert set(metrics.OPERATING_RULES) == {"roc", "f1", "pr", "cost", "eer", "f1max", "spec"}
    assert sorted(metrics.OPERATING_RULES.values()) == list(range(7))
    # no new status code: the range an older test pins
    assert all(-22 <= getattr(_lib, n) <= 0 for n in dir(_lib) if n.startswith("NM_E_"))


def test_workspace_query(lib):
    q = lib.nm_operating_points_workspace
    assert q(1, 1) >= 32 and q(300, 7) >= 300 * 7 * 32 and q(300, 16) > q(300, 7) > q(20, 7)
    for args in ((0, 1), (-1, 1), (1, 0), (1, _lib.NM_OP_MAX_RULES + 1)):
        assert q(*args) == 0, args


def test_argument_errors_come_first(lib):
    p = 4096                                                          # (any non-null address: the checks come first)

    def rule(kind=_lib.NM_OP_F1, n=100, a=0.0, b=1.0, cost_fn=1.0, cost_fp=1.0):
        r = (_lib.NmOpRule * 1)()
        r[0].kind, r[0].n, r[0].a, r[0].b, r[0].cost_fn, r[0].cost_fp = kind, n, a, b, cost_fn, cost_fp
        return r

    def f(scores=p, labels=p, offsets=p, n_sets=2, max_set=100, rules=rule(), n_rules=1, select_of=None, n_eval=2, eval_of=None,
          spec=0.9, sens=0.9, max_fpr=0.1, ws=p, ws_bytes=1 << 40, out=p, summary=None, grid=None, G=0):
        return lib.nm_operating_points(scores, labels, offsets, n_sets, max_set, rules, n_rules, select_of, n_eval, eval_of, spec, sens,
                                       max_fpr, ws, ws_bytes, out, summary, grid, G, None)

    for missing in ("scores", "labels", "offsets", "rules", "ws", "out"):
        assert f(**{missing: None}) == _lib.NM_E_NULL, missing
    assert f(G=10, grid=None) == _lib.NM_E_NULL
    for kw in (dict(n_sets=0), dict(n_sets=-1), dict(max_set=0), dict(max_set=_lib.NM_METRICS_MAX_N + 1), dict(n_rules=0),
               dict(n_rules=_lib.NM_OP_MAX_RULES + 1), dict(n_eval=0), dict(G=-1, grid=p), dict(G=_lib.NM_OP_MAX_GRID + 1, grid=p),
               dict(spec=-0.1), dict(spec=1.5), dict(sens=float("nan")), dict(sens=2.0), dict(max_fpr=0.0), dict(max_fpr=1.5),
               dict(max_fpr=float("nan")), dict(ws_bytes=0), dict(ws_bytes=lib.nm_operating_points_workspace(2, 1) - 1),
               dict(rules=rule(kind=7)), dict(rules=rule(kind=-1)), dict(rules=rule(n=1)), dict(rules=rule(n=0)),
               dict(rules=rule(n=_lib.NM_OP_MAX_LINSPACE + 1)), dict(rules=rule(a=float("inf"))), dict(rules=rule(b=float("nan"))),
               dict(rules=rule(kind=_lib.NM_OP_COST, n=1)), dict(rules=rule(kind=_lib.NM_OP_COST, cost_fn=float("nan"))),
               dict(rules=rule(kind=_lib.NM_OP_COST, cost_fp=float("inf"))), dict(rules=rule(kind=_lib.NM_OP_SPEC, a=1.5)),
               dict(rules=rule(kind=_lib.NM_OP_SPEC, a=float("nan")))):
        assert f(**kw) == _lib.NM_E_METRICS, kw
    assert b"metrics" in lib.nm_status_string(_lib.NM_E_METRICS)


def test_value_errors_come_before_the_device():
    s = torch.tensor([0.5, 1.0, 2.0, 0.25])
    l = torch.tensor([0, 1, 1, 0], dtype=torch.int32)
    big = _lib.NM_METRICS_MAX_N + 1
    bad = [
        (([], []), {}),
        (([s], [l, l]), {}),
        (([s], [l[:3]]), {}),
        (([torch.zeros(big)], [torch.zeros(big, dtype=torch.int32)]), {}),
        (([s], [l]), {"rules": ()}),
        (([s], [l]), {"rules": ("youden",)}),
        (([s], [l]), {"rules": ("roc",) * (_lib.NM_OP_MAX_RULES + 1)}),
        (([s], [l]), {"grid": (0.0, 1.0, 1)}),
        (([s], [l]), {"grid": (0.0, 1.0)}),
        (([s], [l]), {"grid": (0.0, 1.0, 2.5)}),
        (([s], [l]), {"grid": (0.0, float("inf"), 10)}),
        (([s], [l]), {"grid": (float("nan"), 1.0, 10)}),
        (([s], [l]), {"cost_fn": float("nan")}),
        (([s], [l]), {"cost_fp": float("inf")}),
        (([s], [l]), {"spec": 1.5}),
        (([s], [l]), {"sens": -0.5}),
        (([s], [l]), {"max_fpr": 0.0}),
        (([s], [l]), {"max_fpr": 1.5}),
        (([s], [l]), {"roc_grid": -1}),
        (([s], [l]), {"roc_grid": _lib.NM_OP_MAX_GRID + 1}),
        (([s, s], [l, l]), {"evaluate": [0, 2]}),
        (([s, s], [l, l]), {"select_of": [-1, 0]}),
        (([s, s], [l, l]), {"select_of": [0]}),                       # an entry without its selection set
        (([s, s], [l, l]), {"evaluate": []}),
    ]
    for args, kw in bad:
        with pytest.raises(ValueError):
            metrics.operating_points(*args, **kw)
    with pytest.raises(ValueError):
        metrics.classification_performance(s, l, method="youden")
    if not torch.cuda.is_available():                                 # well-formed input, no GPU: no quiet host path
        with pytest.raises(_lib.NmError):
            metrics.operating_points([s], [l], rules=tuple(metrics.OPERATING_RULES))
        with pytest.raises(_lib.NmError):
            metrics.classification_performance(s, l, method="eer")


def test_analysis_lists_the_flags_and_refuses_conflicts(capsys):
    with pytest.raises(SystemExit) as e:
        sweep.main_analysis(["--help"])
    assert e.value.code == 0
    text = capsys.readouterr().out
    for flag in ("--threshold-rule", "--threshold-from", "--cost-fn", "--cost-fp", "--spec", "--threshold-grid", "--roc-grid"):
        assert flag in text, flag
    base = ["--models-dir", "/nonexistent"]
    for bad in (["--threshold-from", "others"], ["--threshold-rule", "roc", "--roi"], ["--roc-grid", "7", "--roi"],
                ["--roc-grid", "1"], ["--roc-grid", str(_lib.NM_OP_MAX_GRID + 1)], ["--threshold-rule", "youden"],
                ["--threshold-rule", "f1", "--threshold-grid", "0", "1", "1"], ["--threshold-rule", "f1", "--threshold-grid", "0", "nan", "9"],
                ["--threshold-rule", "cost", "--threshold-grid", "0", "1", "7.5"], ["--threshold-rule", "spec", "--spec", "1.5"]):
        with pytest.raises(SystemExit) as e:
            sweep.main_analysis(base + bad)
        assert e.value.code == 2, bad
