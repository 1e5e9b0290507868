"""The shared host path of the table statistics on the device.  test_folds with every statistic switched on at once against five
calls that switch on one each: key by key and file by file the same bytes -- what a crossed key or writer in the loop the
statistics share (sweep.ROI_STATS: the three [D, 8] tables and the two maps alike, the z-map on its robust branch) would break,
and no per-feature test sees.  And the one per-row uploader: host words (one copy for all sets) and the same words already on
the device give the same tables.  The cohort of tests/table_stats_util.py: 120 subjects, three diagnoses, two folds, widths 40
and 23, one epoch."""
import filecmp
import tempfile
from pathlib import Path

import numpy as np
import pytest
import torch

from multi_modal_normative_modeling_amd import _lib, metrics, sweep
from tests.table_stats_util import trained_cohort

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
PERM = _lib.NM_ROI_PERM_CHUNK + 1
OPTIONS = {"roi_effect": {},
           "roi_significance": dict(roi_significance=True, roi_perm=PERM, roi_seed=31),
           "roi_regress": dict(roi_regress=("logit", "DIA"), roi_adjust=["AGE"]),
           "normative": dict(normative="signed", robust=True),
           "centile": dict(centile="signed", tail=5.0, quantiles=(0.1, 0.9), centile_loo=True)}


@pytest.fixture(scope="module")
def trained():
    return trained_cohort(120, 2, DEV)


def _files(root):
    return sorted(p.relative_to(root) for p in Path(root).rglob("*") if p.is_file())


def _same(a, b):
    """Arrays, None, or dicts of them ({modality: table}, a normative entry's {"z", "rows", ...}): the same values, NaN where NaN."""
    if isinstance(a, dict):
        return isinstance(b, dict) and list(a) == list(b) and all(_same(a[k], b[k]) for k in a)
    if a is None or b is None:
        return a is None and b is None
    return a.dtype == b.dtype and np.array_equal(a, b, equal_nan=True)


def test_everything_on_is_the_single_options(trained):
    cohort, folds, mods, jobs = trained
    assert PERM == 65
    with tempfile.TemporaryDirectory() as d:
        def run(name, **kw):
            dirs = [Path(d) / name / f"{k:03d}" for k in range(len(folds))]
            return sweep.test_folds(jobs, cohort, folds, mods, "gpoe", DEV, out_dirs=dirs, roi_effect=True, **kw)
        every = run("all", **{k: v for kw in OPTIONS.values() for k, v in kw.items()})
        single = {name: run(name, **kw) for name, kw in OPTIONS.items()}
        assert [list(r) for r in every] == [mods + [k for name in OPTIONS for k in (name, name + "_pooled")]] * len(folds)
        for name, res in single.items():
            for f, (r, r1) in enumerate(zip(every, res)):
                assert set(r1) == set(mods) | {"roi_effect", "roi_effect_pooled", name, name + "_pooled"}
                for key in r1:
                    assert _same(r[key], r1[key]), (name, f, key)
        # the files: every one of the run with everything on has the bytes of the single-option run that writes it, and there
        # is no other
        fa = _files(Path(d) / "all")
        seen = set()
        for name in OPTIONS:
            fs = _files(Path(d) / name)
            assert set(fs) <= set(fa), name
            for p in fs:
                assert filecmp.cmp(Path(d) / "all" / p, Path(d) / name / p, shallow=False), (name, p)
            seen |= set(fs)
        assert seen == set(fa)
        stems = ("roi_effect", "roi_significance", "roi_regress", "normative_z", "normative_subject", "normative_map",
                 "centile_pct", "centile_subject", "centile_map", "centile_curve")
        assert {Path(f"{k:03d}") / m / f"{s}_{m}.csv" for k in range(len(folds)) for m in mods for s in stems} <= seen


def _bits_equal(a, b):
    """torch.equal on the tables' bits (a height of 1 leaves NaN entries, which torch.equal on the values would refuse)."""
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.int64), b.contiguous().view(torch.int64))


def test_host_words_and_device_words_give_the_same_tables():
    rng = np.random.default_rng(65)
    heights, D = (1, 171), 65                                          # (one column past the kernels' 64-column tile)
    mats = [torch.from_numpy(rng.normal(size=(n, D)).astype(np.float32)).to(DEV) for n in heights]
    grp = [rng.choice([1, 0, -1], size=n, p=[0.45, 0.45, 0.1]).astype(np.int32) for n in heights]
    tgt = [rng.normal(size=n).astype(np.float32) for n in heights]
    inc = [None, (rng.random(171) < 0.9).astype(np.int32)]

    def dev(seq):
        return [None if v is None else torch.from_numpy(v).to(DEV) for v in seq]
    pairs = [(metrics.roi_effect(mats, grp), metrics.roi_effect(mats, dev(grp))),
             (metrics.column_regress(mats, tgt, kind="ols", include=inc), metrics.column_regress(mats, dev(tgt), kind="ols", include=dev(inc))),
             (metrics.cohort_moments(mats, grp), metrics.cohort_moments(mats, dev(grp)))]
    torch.cuda.synchronize()
    for host, device in pairs:
        assert host.shape == (2, D, 8) and host.dtype == torch.float64 and _bits_equal(host, device)
        assert torch.isfinite(host[1, :, 0]).all()                     # (the tall set is a real result, not a refusal)
