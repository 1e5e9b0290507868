"""CPU-side checks of nm_roi_significance: both symbols are exported and declared, the header's constants are _lib's, the
workspace query is monotone and covers the rank table, every status code comes back before a device is touched, and
metrics.roi_significance / metrics.mann_whitney refuse malformed inputs with ValueErrors before they ask for a GPU.
No compute calls: no GPU here."""
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


def test_symbols_are_exported_and_declared(lib):
    header = (ROOT / "include" / "nmhip.h").read_text()
    for name in ("nm_roi_significance_workspace", "nm_roi_significance"):
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name)
    assert re.search(r"\bsize_t\s+nm_roi_significance_workspace\s*\(int n_sets, int D, int max_rows, int n_perm\)", header)
    assert re.search(r"\bint\s+nm_roi_significance\s*\(const nm_roi_set_t\*\s*sets_dev, int n_sets, int D, int max_rows, int n_perm, "
                     r"uint64_t seed,\s*void\* workspace, size_t workspace_bytes, double\* out, int32_t\* maxstat_out, void\* stream\)", header)
    for name in ("NM_ROI_MAX_PERM", "NM_ROI_PERM_CHUNK", "NM_ROI_ROW_CHUNK"):
        assert re.search(r"^#define\s+%s\s+%d\s*$" % (name, getattr(_lib, name)), header, flags=re.M), name
    assert _lib.NM_ROI_MAX_PERM == 65535
    assert metrics.ROI_SIGNIFICANCE_COLUMNS == ("u_x", "tie_term", "z", "p_mwu", "q_bh", "p_perm", "p_maxt", "n_perm")
    assert len(metrics.ROI_SIGNIFICANCE_COLUMNS) == _lib.NM_METRICS_STRIDE


def test_workspace_query_is_monotone_and_covers_the_ranks(lib):
    q = lib.nm_roi_significance_workspace
    base = (3, 70, 171, 130)
    for args in (base, (1, 1, 1, 0), (20, 1137, 1064, 10000), (1, 8192, 8192, 65535), (5, 379, 8192, 0)):
        assert q(*args) >= 2 * args[0] * args[1] * args[2], args
    for pos, grid in enumerate(([1, 2, 3, 4, 19, 20, 21], [1, 63, 64, 65, 128, 129, 379, 1137], [1, 31, 32, 33, 171, 256, 257, 8192],
                                [0, 1, 63, 64, 65, 128, 129, 1000, 65535])):
        sizes = []
        for v in grid:
            args = list(base)
            args[pos] = v
            sizes.append(q(*args))
        assert sizes == sorted(sizes) and sizes[0] > 0 and sizes[-1] > sizes[0], (pos, sizes)
    # arguments no launch accepts: nothing to allocate
    assert q(0, 70, 171, 1) == 0 and q(1, 0, 171, 1) == 0 and q(1, 70, 0, 1) == 0 and q(1, 70, 171, -1) == 0


def test_argument_errors_come_first(lib):
    p = 4096                                                          # (any non-null address: the checks come first)
    f = lib.nm_roi_significance
    big = 1 << 40
    assert f(None, 1, 10, 100, 5, 0, p, big, p, None, None) == _lib.NM_E_NULL
    assert f(p, 1, 10, 100, 5, 0, None, big, p, None, None) == _lib.NM_E_NULL
    assert f(p, 1, 10, 100, 5, 0, p, big, None, None, None) == _lib.NM_E_NULL
    for n_sets in (0, -1):
        assert f(p, n_sets, 10, 100, 5, 0, p, big, p, None, None) == _lib.NM_E_METRICS, n_sets
    for D in (0, -5, 8193):
        assert f(p, 1, D, 100, 5, 0, p, big, p, None, None) == _lib.NM_E_METRICS, D
    for max_rows in (0, -1, _lib.NM_METRICS_MAX_N + 1):
        assert f(p, 1, 10, max_rows, 5, 0, p, big, p, None, None) == _lib.NM_E_METRICS, max_rows
    for n_perm in (-1, _lib.NM_ROI_MAX_PERM + 1):
        assert f(p, 1, 10, 100, n_perm, 0, p, big, p, None, None) == _lib.NM_E_METRICS, n_perm
    need = lib.nm_roi_significance_workspace(2, 10, 100, 5)
    assert need > 0
    for short in (0, need - 1):
        assert f(p, 2, 10, 100, 5, 0, p, short, p, None, None) == _lib.NM_E_METRICS, short
    # more than 2^31 - 1 workgroups: 2^19 sets x 8192 columns in the rank pass; 40000 sets x 60000 permutations in the label pass
    assert f(p, 1 << 19, 8192, 1, 0, 0, p, 1 << 62, p, None, None) == _lib.NM_E_METRICS
    assert f(p, 40000, 1, 1, 60000, 0, p, 1 << 62, p, None, None) == _lib.NM_E_METRICS
    assert b"metrics" in lib.nm_status_string(_lib.NM_E_METRICS)


def test_roi_significance_value_errors_come_before_the_device():
    x = torch.zeros(6, 5)
    g = torch.zeros(6, dtype=torch.int32)
    bad = [
        (([], []), {}),                                               # no set at all
        (([x], [g, g]), {}),                                          # a group vector too many
        (([x.double()], [g]), {}),                                    # not fp32
        (([x[0]], [g[:1]]), {}),                                      # not a matrix
        (([x, torch.zeros(6, 4)], [g, g]), {}),                       # widths differ
        (([torch.zeros(6, 0)], [g]), {}),                             # no column
        (([x], [g[:5]]), {}),                                         # a row without its group word
        (([torch.zeros(6, 10)[:, ::2]], [g]), {}),                    # columns not contiguous
        (([torch.zeros(_lib.NM_METRICS_MAX_N + 1, 2)], [torch.zeros(_lib.NM_METRICS_MAX_N + 1)]), {}),
        (([torch.zeros(2, 8193)], [g[:2]]), {}),                      # wider than the BH sort takes
        (([x], [g]), {"n_perm": -1}),
        (([x], [g]), {"n_perm": _lib.NM_ROI_MAX_PERM + 1}),
        (([x], [g]), {"seed": -1}),
        (([x], [g]), {"seed": 1 << 64}),
    ]
    for args, kw in bad:
        with pytest.raises(ValueError):
            metrics.roi_significance(*args, **kw)
    with pytest.raises(ValueError):
        metrics.mann_whitney([1.0, 2.0], [[1.0], [2.0]])
    with pytest.raises(ValueError):
        metrics.mann_whitney(torch.zeros(4, 3), torch.zeros(4, 2))
    with pytest.raises(ValueError):
        metrics.mann_whitney(torch.zeros(5000), torch.zeros(5000))
    with pytest.raises(ValueError):
        metrics.mann_whitney([1.0, 2.0], [0.5], n_perm=70000)
    if not torch.cuda.is_available():                                 # well-formed input, no GPU: no quiet host path
        with pytest.raises(_lib.NmError):
            metrics.roi_significance([x], [g], n_perm=3)
        with pytest.raises(_lib.NmError):
            metrics.mann_whitney([1.0, 2.0], [0.5])
