"""CPU-side checks of nm_column_regress: it is exported and declared, the pointer-table entry has the C layout, the #defines
agree with _lib, its argument errors come back before a device is touched, and metrics.column_regress /
metrics.latent_pvalues refuse malformed inputs with ValueErrors before they ask for a GPU.  No compute calls: no GPU here."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest
import torch

from multi_modal_normative_modeling_amd import _lib, metrics

ROOT = Path(__file__).resolve().parent.parent


@pytest.fixture(scope="module")
def lib():
    if not _lib.LIB_PATH.exists():
        import __graft_entry__ as ge
        ge.build()
    return _lib.load()


def test_symbols_are_exported_and_declared(lib):
    for name in ("nm_column_regress", "nm_student_t_two_sided"):
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name)
    header = (ROOT / "include" / "nmhip.h").read_text()
    assert re.search(r"\bint\s+nm_column_regress\s*\(const nm_reg_set_t\*", header)
    assert re.search(r"\bdouble\s+nm_student_t_two_sided\s*\(double t, double df\)", header)
    assert metrics.COLUMN_REGRESS_COLUMNS == ("const", "coef", "se_const", "se_coef", "p_const", "p_coef", "n_obs", "n_iter")
    assert len(metrics.COLUMN_REGRESS_COLUMNS) == _lib.NM_METRICS_STRIDE
    assert metrics.COLUMN_REGRESS_KINDS == {"ols": _lib.NM_REG_OLS, "logit": _lib.NM_REG_LOGIT}


def test_table_entry_has_the_c_layout():
    S = _lib.NmRegSet
    assert C.sizeof(S) == 48
    assert [S.x.offset, S.target.offset, S.cov.offset, S.include.offset, S.rows.offset, S.pitch.offset, S.cov_pitch.offset,
            S.pad.offset] == [0, 8, 16, 24, 32, 36, 40, 44]


def test_defines_agree_with_the_binding():
    header = (ROOT / "include" / "nmhip.h").read_text()
    for name in ("NM_REG_OLS", "NM_REG_LOGIT", "NM_REG_MAX_COV", "NM_REG_MAX_ITER"):
        m = re.search(r"^#define\s+%s\s+(\d+)\b" % name, header, flags=re.M)
        assert m and int(m.group(1)) == getattr(_lib, name), name
    m = re.search(r"^#define\s+NM_REG_TOL\s+(\S+)", header, flags=re.M)
    assert m and float(m.group(1)) == _lib.NM_REG_TOL == 1e-8
    assert (_lib.NM_REG_OLS, _lib.NM_REG_LOGIT, _lib.NM_REG_MAX_COV, _lib.NM_REG_MAX_ITER) == (0, 1, 4, 35)


def test_argument_errors_come_first(lib):
    p = 4096                                                          # (any non-null address: the checks come first)
    f = lib.nm_column_regress
    assert f(None, 1, 10, 100, 0, 0, p, None) == _lib.NM_E_NULL
    assert f(p, 1, 10, 100, 0, 0, None, None) == _lib.NM_E_NULL
    for n_sets in (0, -1):
        assert f(p, n_sets, 10, 100, 0, 0, p, None) == _lib.NM_E_METRICS, n_sets
    for D in (0, -5):
        assert f(p, 1, D, 100, 0, 0, p, None) == _lib.NM_E_METRICS, D
    for max_rows in (0, -1, _lib.NM_METRICS_MAX_N + 1):
        assert f(p, 1, 10, max_rows, 0, 1, p, None) == _lib.NM_E_METRICS, max_rows
    for n_cov in (-1, _lib.NM_REG_MAX_COV + 1):
        assert f(p, 1, 10, 100, n_cov, 0, p, None) == _lib.NM_E_METRICS, n_cov
    for kind in (-1, 2, 7):
        assert f(p, 1, 10, 100, 0, kind, p, None) == _lib.NM_E_METRICS, kind


def test_column_regress_shape_errors():
    x = torch.zeros(6, 5)
    y = torch.zeros(6)
    bad = [
        dict(mats=[], targets=[]),                                            # no set at all
        dict(mats=[x], targets=[y, y]),                                       # a target too many
        dict(mats=[x.double()], targets=[y]),                                 # not fp32
        dict(mats=[x[0]], targets=[y[:1]]),                                   # not a matrix
        dict(mats=[x, torch.zeros(6, 4)], targets=[y, y]),                    # widths differ
        dict(mats=[torch.zeros(6, 0)], targets=[y]),                          # no column
        dict(mats=[x], targets=[y[:5]]),                                      # a row without its target
        dict(mats=[torch.zeros(6, 10)[:, ::2]], targets=[y]),                 # columns not contiguous
        dict(mats=[torch.zeros(_lib.NM_METRICS_MAX_N + 1, 2)], targets=[torch.zeros(_lib.NM_METRICS_MAX_N + 1)]),
        dict(mats=[x], targets=[y], kind="probit"),                           # an unknown kind
        dict(mats=[x], targets=[y], covariates=[torch.zeros(6, _lib.NM_REG_MAX_COV + 1)]),   # too many covariates
        dict(mats=[x], targets=[y], covariates=[torch.zeros(5, 2)]),          # a row without its covariates
        dict(mats=[x], targets=[y], covariates=[torch.zeros(6)]),             # covariates not [rows, q]
        dict(mats=[x, x], targets=[y, y], covariates=[torch.zeros(6, 2)]),    # one entry per set
        dict(mats=[x, x], targets=[y, y], covariates=[torch.zeros(6, 2), torch.zeros(6, 1)]),
        dict(mats=[x], targets=[y], include=[torch.zeros(5)]),                # a row without its include word
        dict(mats=[x, x], targets=[y, y], include=[None]),
    ]
    for kw in bad:
        with pytest.raises(ValueError):
            metrics.column_regress(**kw)
    with pytest.raises(ValueError):
        metrics.latent_pvalues(np.zeros(8), np.zeros(8), "continuous")        # latent is not [n, Z]
    with pytest.raises(ValueError):
        metrics.latent_pvalues(np.zeros((8, 3)), np.zeros(7), "categorical")  # a subject without its target
    with pytest.raises(ValueError):
        metrics.latent_pvalues(np.zeros((_lib.NM_METRICS_MAX_N + 1, 2)), np.zeros(_lib.NM_METRICS_MAX_N + 1), "continuous")
    if not torch.cuda.is_available():                                 # well-formed input, no GPU: no quiet host path
        with pytest.raises(_lib.NmError):
            metrics.column_regress([x], [y], kind="logit", covariates=[torch.zeros(6, 2)], include=[torch.ones(6)])
        with pytest.raises(_lib.NmError):
            metrics.latent_pvalues(np.zeros((8, 3)), np.zeros(8), "continuous")


def test_pointer_table_reads_views_where_they_lie():
    buf = torch.zeros(40, 12)
    y = torch.zeros(40)
    cov = torch.zeros(40, 2)
    inc = torch.ones(40, dtype=torch.int32)
    views = [buf[:, :9], buf[5:31, :9], buf[7:8, :9], buf[:0, :9]]
    table = metrics._reg_table(views, [y[:len(v)] for v in views], [cov[:len(v)] for v in views],
                               [inc, None, inc[:1], None], 2)
    esz = buf.element_size()
    assert [t.x for t in table] == [buf.data_ptr(), buf.data_ptr() + 5 * 12 * esz, buf.data_ptr() + 7 * 12 * esz, None]
    assert [t.rows for t in table] == [40, 26, 1, 0]
    assert [t.pitch for t in table] == [12, 12, 9, 9]
    assert [t.cov_pitch for t in table] == [2, 2, 2, 2]
    assert table[0].target == y.data_ptr() and table[0].cov == cov.data_ptr() and table[0].include == inc.data_ptr()
    assert table[1].include is None and table[3].target is None and table[3].cov is None
    assert C.sizeof(table) == 4 * 48
