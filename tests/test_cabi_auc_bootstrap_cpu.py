"""CPU-side checks of nm_auc_bootstrap: both symbols are exported and declared with the header's prototypes, the header's
constants are _lib's, the workspace query is positive and monotone, every status code comes back before a device is touched,
and metrics.auc_bootstrap / metrics.auc_compare refuse malformed inputs with ValueErrors before they ask for a GPU.
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
    for name in ("nm_auc_bootstrap_workspace", "nm_auc_bootstrap"):
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name)
    assert re.search(r"\bsize_t\s+nm_auc_bootstrap_workspace\s*\(int n_sets, int max_set, int n_boot, int n_pairs\)\s*;", header)
    assert re.search(r"\bint\s+nm_auc_bootstrap\s*\(const float\* scores, const int32_t\* labels, const int32_t\* offsets, "
                     r"const int32_t\* streams,\s*int n_sets, int max_set, int n_boot, int lo_index, int hi_index, uint64_t seed,\s*"
                     r"const int32_t\* pairs, int n_pairs, void\* workspace, size_t workspace_bytes,\s*"
                     r"double\* out, double\* pairs_out, int32_t\* boot_out, void\* stream\)\s*;", header)
    for name in ("NM_BOOT_MAX", "NM_BOOT_CHUNK"):
        assert re.search(r"^#define\s+%s\s+%d\s*$" % (name, getattr(_lib, name)), header, flags=re.M), name
    assert _lib.NM_BOOT_MAX == 16384 and _lib.NM_BOOT_MAX % _lib.NM_BOOT_CHUNK == 0
    assert len(lib.nm_auc_bootstrap.argtypes) == 18
    assert metrics.AUC_BOOTSTRAP_COLUMNS == ("roc_auc", "ci_lo", "ci_hi", "boot_mean", "boot_se", "n_boot", "n_pos", "n_neg")
    assert metrics.AUC_COMPARE_COLUMNS == ("delta_auc", "ci_lo", "ci_hi", "boot_mean", "boot_se", "p_boot", "n_le0", "n_ge0")
    assert len(metrics.AUC_BOOTSTRAP_COLUMNS) == len(metrics.AUC_COMPARE_COLUMNS) == _lib.NM_METRICS_STRIDE


def test_workspace_query_is_positive_and_monotone(lib):
    q = lib.nm_auc_bootstrap_workspace
    base = (3, 171, 130, 2)
    for args in (base, (1, 1, 1, 0), (256, 1064, 10000, 255), (1, 8192, 16384, 0)):
        # the group table (uint16 per score) and the distribution (int32 per resample) lie in it
        assert q(*args) >= args[0] * (2 * args[1] + 4 * args[2]), args
    for pos, grid in enumerate(([1, 2, 3, 4, 19, 20, 256], [1, 2, 63, 64, 65, 171, 1064, 8192], [1, 63, 64, 65, 129, 2000, 16384],
                                [0, 1, 2, 255, 100000])):
        sizes = []
        for v in grid:
            args = list(base)
            args[pos] = v
            sizes.append(q(*args))
        assert sizes == sorted(sizes) and sizes[0] > 0, (pos, sizes)
        assert pos == 3 or sizes[-1] > sizes[0], (pos, sizes)          # (a pair needs no room of its own)
    # arguments no launch accepts: nothing to allocate
    for args in ((0, 171, 130, 0), (-1, 171, 130, 0), (1, 0, 130, 0), (1, _lib.NM_METRICS_MAX_N + 1, 130, 0), (1, 171, 0, 0),
                 (1, 171, _lib.NM_BOOT_MAX + 1, 0), (1, 171, 130, -1)):
        assert q(*args) == 0, args


def test_argument_errors_come_first(lib):
    p = 4096                                                          # (any non-null address: the checks come first)
    big = 1 << 40

    def f(scores=p, labels=p, offsets=p, streams=None, n_sets=2, max_set=100, n_boot=50, lo=1, hi=48, seed=0, pairs=None, n_pairs=0,
          ws=p, ws_bytes=big, out=p, pairs_out=None, boot_out=None):
        return lib.nm_auc_bootstrap(scores, labels, offsets, streams, n_sets, max_set, n_boot, lo, hi, seed, pairs, n_pairs, ws, ws_bytes,
                                    out, pairs_out, boot_out, None)

    for missing in ("scores", "labels", "offsets", "ws", "out"):
        assert f(**{missing: None}) == _lib.NM_E_NULL, missing
    assert f(n_pairs=1, pairs=None, pairs_out=p) == _lib.NM_E_NULL
    assert f(n_pairs=1, pairs=p, pairs_out=None) == _lib.NM_E_NULL
    for n_sets in (0, -1):
        assert f(n_sets=n_sets) == _lib.NM_E_METRICS, n_sets
    for max_set in (0, -1, _lib.NM_METRICS_MAX_N + 1):
        assert f(max_set=max_set) == _lib.NM_E_METRICS, max_set
    for n_boot in (0, -1, _lib.NM_BOOT_MAX + 1):
        assert f(n_boot=n_boot, lo=0, hi=0) == _lib.NM_E_METRICS, n_boot
    assert f(n_pairs=-1) == _lib.NM_E_METRICS
    for lo, hi in ((-1, 48), (30, 29), (0, 50), (50, 50), (0, -1)):
        assert f(lo=lo, hi=hi) == _lib.NM_E_METRICS, (lo, hi)
    need = lib.nm_auc_bootstrap_workspace(2, 100, 50, 0)
    assert need > 0
    for short in (0, need - 1):
        assert f(ws_bytes=short) == _lib.NM_E_METRICS, short
    # more than 2^31 - 1 workgroups: 2^24 sets x 256 chunks in the resample pass; sets + pairs in the close pass
    assert f(n_sets=1 << 24, max_set=1, n_boot=_lib.NM_BOOT_MAX, lo=0, hi=0, ws_bytes=1 << 62) == _lib.NM_E_METRICS
    assert f(n_sets=1 << 20, max_set=1, n_boot=1, lo=0, hi=0, n_pairs=(1 << 31) - 1, pairs=p, pairs_out=p, ws_bytes=1 << 62) == _lib.NM_E_METRICS
    assert b"metrics" in lib.nm_status_string(_lib.NM_E_METRICS)


def test_value_errors_come_before_the_device():
    s = torch.tensor([0.5, 1.0, 2.0, 0.25])
    l = torch.tensor([0, 1, 1, 0], dtype=torch.int32)
    big = _lib.NM_METRICS_MAX_N + 1
    bad = [
        (([], []), {}),                                               # no set at all
        (([s], [l, l]), {}),                                          # a label vector too many
        (([s], [l[:3]]), {}),                                         # a score without its label
        (([torch.zeros(big)], [torch.zeros(big, dtype=torch.int32)]), {}),
        (([s], [l]), {"n_boot": 0}),
        (([s], [l]), {"n_boot": _lib.NM_BOOT_MAX + 1}),
        (([s], [l]), {"ci": 0.0}),
        (([s], [l]), {"ci": 1.0}),
        (([s], [l]), {"ci": -0.5}),
        (([s], [l]), {"seed": -1}),
        (([s], [l]), {"seed": 1 << 64}),
        (([s], [l]), {"streams": [-1]}),
        (([s], [l]), {"streams": [1 << 24]}),
        (([s], [l]), {"streams": [0, 1]}),                            # a stream id too many
        (([s, s], [l, l]), {"pairs": [(0, 2)]}),
        (([s, s], [l, l]), {"pairs": [(-1, 0)]}),
    ]
    for args, kw in bad:
        with pytest.raises(ValueError):
            metrics.auc_bootstrap(*args, **kw)
    with pytest.raises(ValueError):
        metrics.auc_compare(s, s[:3], l)
    with pytest.raises(ValueError):
        metrics.auc_compare(s, s, l[:3])
    with pytest.raises(ValueError):
        metrics.auc_compare(s, s, l, n_boot=_lib.NM_BOOT_MAX + 1)
    with pytest.raises(ValueError):
        metrics.auc_compare(s, s, l, ci=1.5)
    assert metrics.boot_indices(2000, 0.95) == (49, 1950) and metrics.boot_indices(1, 0.95) == (0, 0)
    if not torch.cuda.is_available():                                 # well-formed input, no GPU: no quiet host path
        with pytest.raises(_lib.NmError):
            metrics.auc_bootstrap([s], [l], n_boot=3)
        with pytest.raises(_lib.NmError):
            metrics.auc_compare(s, s, l, n_boot=3)
