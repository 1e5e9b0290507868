"""CPU-side checks of nm_roi_effect: it is exported and declared, its argument errors come back before a device is
touched, the pointer-table entry has the C layout, and metrics.roi_effect / metrics.cliff_delta refuse malformed inputs with
ValueErrors before they ask for a GPU.  No compute calls: no GPU here."""
import ctypes as C
import re
from pathlib import Path

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


def test_symbol_is_exported_and_declared(lib):
    assert "nm_roi_effect" in _lib.EXPORTED_SYMBOLS
    assert hasattr(lib, "nm_roi_effect")
    header = (ROOT / "include" / "nmhip.h").read_text()
    assert re.search(r"\bint\s+nm_roi_effect\s*\(const nm_roi_set_t\*", header)
    assert re.search(r"^#define\s+NM_ROI_Y_CHUNK\s+%d\s*$" % _lib.NM_ROI_Y_CHUNK, header, flags=re.M)
    # the table entry: two pointers, rows, pitch -- 24 bytes, as the C struct (a static_assert holds the library to it)
    assert C.sizeof(_lib.NmRoiSet) == 24
    assert [(_lib.NmRoiSet.x.offset), _lib.NmRoiSet.group.offset, _lib.NmRoiSet.rows.offset, _lib.NmRoiSet.pitch.offset] == [0, 8, 16, 20]
    assert metrics.ROI_EFFECT_COLUMNS == ("cliff_delta", "auc", "n_more", "n_less", "n_x", "n_y", "mean_x", "mean_y")
    assert len(metrics.ROI_EFFECT_COLUMNS) == _lib.NM_METRICS_STRIDE


def test_argument_errors_come_first(lib):
    p = 4096                                                          # (any non-null address: the checks come first)
    assert lib.nm_roi_effect(None, 1, 10, 100, p, None) == _lib.NM_E_NULL
    assert lib.nm_roi_effect(p, 1, 10, 100, None, None) == _lib.NM_E_NULL
    for n_sets in (0, -1):
        assert lib.nm_roi_effect(p, n_sets, 10, 100, p, None) == _lib.NM_E_METRICS, n_sets
    for D in (0, -5):
        assert lib.nm_roi_effect(p, 1, D, 100, p, None) == _lib.NM_E_METRICS, D
    for max_rows in (0, -1, _lib.NM_METRICS_MAX_N + 1):
        assert lib.nm_roi_effect(p, 1, 10, max_rows, p, None) == _lib.NM_E_METRICS, max_rows
    assert b"metrics" in lib.nm_status_string(_lib.NM_E_METRICS)


def test_roi_effect_shape_errors():
    x = torch.zeros(6, 5)
    g = torch.zeros(6, dtype=torch.int32)
    bad = [
        ([], []),                                                     # no set at all
        ([x], [g, g]),                                                # a group vector too many
        ([x.double()], [g]),                                          # not fp32
        ([x[0]], [g[:1]]),                                            # not a matrix
        ([x, torch.zeros(6, 4)], [g, g]),                             # widths differ
        ([torch.zeros(6, 0)], [g]),                                   # no column
        ([x], [g[:5]]),                                               # a row without its group word
        ([x.t().contiguous().t()], [g]),                              # columns not contiguous
        ([torch.zeros(6, 10)[:, ::2]], [g]),                          # ... a strided column view neither
        ([torch.zeros(_lib.NM_METRICS_MAX_N + 1, 2)], [torch.zeros(_lib.NM_METRICS_MAX_N + 1)]),
    ]
    for mats, groups in bad:
        with pytest.raises(ValueError):
            metrics.roi_effect(mats, groups)
    with pytest.raises(ValueError):
        metrics.cliff_delta([1.0, 2.0], [[1.0], [2.0]])
    with pytest.raises(ValueError):
        metrics.cliff_delta(torch.zeros(4, 3), torch.zeros(4, 2))
    with pytest.raises(ValueError):
        metrics.cliff_delta(torch.zeros(5000), torch.zeros(5000))
    if not torch.cuda.is_available():                                 # well-formed input, no GPU: no quiet host path
        with pytest.raises(_lib.NmError):
            metrics.roi_effect([x], [g])
        with pytest.raises(_lib.NmError):
            metrics.cliff_delta([1.0, 2.0], [0.5])


def test_pointer_table_reads_views_where_they_lie():
    buf = torch.zeros(40, 12)
    g = torch.zeros(40, dtype=torch.int32)
    views = [buf[:, :9], buf[5:31, :9], buf[7:8, :9], buf[:0, :9]]
    table = metrics._roi_table(views, [g[:len(v)] for v in views])
    esz = buf.element_size()
    assert [t.x for t in table] == [buf.data_ptr(), buf.data_ptr() + 5 * 12 * esz, buf.data_ptr() + 7 * 12 * esz, None]
    assert [t.rows for t in table] == [40, 26, 1, 0]
    assert [t.pitch for t in table] == [12, 12, 9, 9]               # (one row or none: the pitch is never used)
    assert table[3].group is None and table[0].group == g.data_ptr()
    assert C.sizeof(table) == 4 * 24
