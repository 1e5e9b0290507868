"""The AUC bootstrap through the sweep: `analysis --bootstrap B [--against Q]` on the files two small procedures wrote for the
synthetic cohort (-K 2, a few training steps), against the yardstick computed from the reconstruction_error_*.csv files on
disk; group_analysis.csv and the returned table byte for byte as without the new flags; the two refusals."""
import shutil
import tempfile
from pathlib import Path

import numpy as np
import pytest

from multi_modal_normative_modeling_amd import metrics, sweep, workload
from tests import auc_bootstrap_ref as R

pytestmark = pytest.mark.gpu

P, Q = "SE-gPoE", "SM-T1w_sMRI"
K, BOOT, SEED, CI = 2, 130, 17, 0.9
COMMON = ["-K", str(K), "-H", "32", "24", "8"]
EXACT = [0, 1, 2, 5, 6, 7]


@pytest.fixture(scope="module")
def tree():
    """<dir>/HCPimage/<procedure>/<fold>/<modality>/reconstruction_error_<modality>.csv of both procedures."""
    d = Path(tempfile.mkdtemp())
    try:
        for proc in (P, Q):
            sweep.main(["-P", proc, "-E", "2", "--subjects", "300", "--out-dir", str(d), "--save-models", "--no-csv"] + COMMON)
            sweep.main_test(["-P", proc, "--subjects", "300", "--models-dir", str(d)] + COMMON)
        yield d
    finally:
        shutil.rmtree(d, ignore_errors=True)


def _sets(root, proc):
    """From the files on disk: per fold and pooled (scores fp32, patient flags), as `analysis` forms them."""
    import pandas as pd
    mods, _ = workload.procedure_modalities(proc, "HCPimage")
    sets = []
    for k in range(K):
        dfs = [pd.read_csv(root / "HCPimage" / proc / f"{k:03d}" / m / f"reconstruction_error_{m}.csv") for m in mods]
        err = sum(d["Reconstruction error"].to_numpy(dtype=np.float64) for d in dfs) / len(dfs)
        sets.append((err.astype(np.float32), (dfs[0]["DIA"].to_numpy() != 1).astype(np.int32)))
    sets.append((np.concatenate([s for s, _ in sets]), np.concatenate([l for _, l in sets])))
    return sets


def _held(got, ref, what):
    assert got.shape == ref.shape, what
    a, b = np.ascontiguousarray(got[:, EXACT]), np.ascontiguousarray(ref[:, EXACT])
    assert np.array_equal(a.view(np.int64), b.view(np.int64)), (what, a, b)
    for j in (3, 4):
        assert np.all(np.abs(got[:, j] - ref[:, j]) <= R.moment_bound(BOOT) * np.abs(ref[:, j])), (what, j)


def test_bootstrap_and_comparison_files_and_the_untouched_rest(tree, capsys):
    import pandas as pd
    root = tree / "HCPimage" / P
    args = ["-P", P, "--models-dir", str(tree)] + COMMON
    base = sweep.main_analysis(args)
    before = (root / "group_analysis.csv").read_bytes()
    listed = sorted(p.name for p in root.iterdir())
    boot = sweep.main_analysis(args + ["--bootstrap", str(BOOT), "--boot-seed", str(SEED), "--ci", str(CI)])
    assert (root / "group_analysis.csv").read_bytes() == before and boot.numpy().tobytes() == base.numpy().tobytes()
    assert sorted(p.name for p in root.iterdir()) == sorted(listed + ["group_analysis_bootstrap.csv"])
    both = sweep.main_analysis(args + ["--bootstrap", str(BOOT), "--boot-seed", str(SEED), "--ci", str(CI), "--against", Q])
    assert (root / "group_analysis.csv").read_bytes() == before and both.numpy().tobytes() == base.numpy().tobytes()
    assert sorted(p.name for p in root.iterdir()) == sorted(listed + ["group_analysis_bootstrap.csv", f"group_analysis_compare_{P}_vs_{Q}.csv"])
    text = capsys.readouterr().out
    assert "pooled: AUC " in text and f"{P} - {Q} pooled: delta AUC " in text

    lo, hi = R.boot_indices(BOOT, CI)
    sp, sq = _sets(tree, P), _sets(tree, Q)
    streams = list(range(K)) + [K]                                     # fold k: stream k; the pooled rows: stream n_splits
    assert all(min(l.sum(), len(l) - l.sum()) >= 1 for _, l in sp)
    df = pd.read_csv(root / "group_analysis_bootstrap.csv", float_precision="round_trip")
    assert list(df.columns) == ["fold"] + list(metrics.AUC_BOOTSTRAP_COLUMNS)
    assert [str(v) for v in df["fold"]] == [str(k) for k in range(K)] + ["pooled"]
    ref = np.stack([R.set_row(s, l, BOOT, lo, hi, SEED, k) for (s, l), k in zip(sp, streams)])
    _held(df.iloc[:, 1:].to_numpy(dtype=np.float64), ref, "bootstrap csv")
    assert np.array_equal(df["roc_auc"].to_numpy()[:K], base.numpy()[:, 0])
    dc = pd.read_csv(root / f"group_analysis_compare_{P}_vs_{Q}.csv", float_precision="round_trip")
    assert list(dc.columns) == ["fold", "auc_a", "auc_c"] + list(metrics.AUC_COMPARE_COLUMNS)
    assert [str(v) for v in dc["fold"]] == [str(v) for v in df["fold"]]
    refc = np.stack([R.pair_row((*a, k), (*c, k), BOOT, lo, hi, SEED) for a, c, k in zip(sp, sq, streams)])
    _held(dc.iloc[:, 3:].to_numpy(dtype=np.float64), refc, "compare csv")
    assert not np.isnan(refc).any()
    assert np.array_equal(dc["auc_a"].to_numpy(), df["roc_auc"].to_numpy())
    # (delta_auc is one division of the integer difference: within a rounding or two of the difference of the quotients)
    assert np.allclose(dc["auc_a"].to_numpy() - dc["auc_c"].to_numpy(), dc["delta_auc"].to_numpy(), rtol=0, atol=4 * 2.0 ** -53)


def test_against_needs_bootstrap(tree):
    with pytest.raises(SystemExit):
        sweep.main_analysis(["-P", P, "--models-dir", str(tree), "--against", Q] + COMMON)


def test_other_subjects_in_a_fold_are_refused(tree):
    import pandas as pd
    with tempfile.TemporaryDirectory() as d:
        other = Path(d) / "t"
        shutil.copytree(tree, other, ignore=shutil.ignore_patterns("*.pt", "*.pth", "*.bin"))
        f = other / "HCPimage" / Q / "001" / "T1w_sMRI" / "reconstruction_error_T1w_sMRI.csv"
        df = pd.read_csv(f)
        df.iloc[::-1].to_csv(f, index=False)                           # the same subjects in another order
        made = other / "HCPimage" / P / f"group_analysis_compare_{P}_vs_{Q}.csv"
        made.unlink(missing_ok=True)                                   # (the copy may hold an earlier test's)
        with pytest.raises(ValueError, match="fold 1 does not hold"):
            sweep.main_analysis(["-P", P, "--models-dir", str(other), "--bootstrap", "20", "--against", Q] + COMMON)
        assert not made.exists()
