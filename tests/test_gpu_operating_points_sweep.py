"""Operating points through the sweep: `analysis --threshold-rule R [--threshold-from others] [--roc-grid G]` on the files a
small procedure wrote for the synthetic cohort (-K 2, a few training steps): the three files with their columns, the `self`
rows against a direct metrics.operating_points call on the files' scores, the `others` thresholds against a pooled selection
made by hand without the fold's own subjects, identical files on a second run, and an untouched directory without the flags."""
import shutil
import tempfile
from pathlib import Path

import numpy as np
import pytest
import torch

from multi_modal_normative_modeling_amd import metrics, sweep, workload

pytestmark = pytest.mark.gpu

P = "SE-gPoE"
K, G, RULE = 2, 50, "f1max"
COMMON = ["-K", str(K), "-H", "32", "24", "8"]
NEW = [f"group_analysis_operating_{RULE}.csv", "group_analysis_curve.csv", "group_analysis_roc_curve.csv"]


@pytest.fixture(scope="module")
def tree():
    d = Path(tempfile.mkdtemp())
    try:
        sweep.main(["-P", P, "-E", "2", "--subjects", "300", "--out-dir", str(d), "--save-models", "--no-csv"] + COMMON)
        sweep.main_test(["-P", P, "--subjects", "300", "--models-dir", str(d)] + COMMON)
        yield d
    finally:
        shutil.rmtree(d, ignore_errors=True)


def _sets(root):
    """From the files on disk, per fold: scores fp32, patient flags, participant ids, as `analysis` forms them."""
    import pandas as pd
    mods, _ = workload.procedure_modalities(P, "HCPimage")
    sets = []
    for k in range(K):
        dfs = [pd.read_csv(root / f"{k:03d}" / m / f"reconstruction_error_{m}.csv") for m in mods]
        err = sum(d["Reconstruction error"].to_numpy(dtype=np.float64) for d in dfs) / len(dfs)
        sets.append((err.astype(np.float32), (dfs[0]["DIA"].to_numpy() != 1).astype(np.int32), dfs[0]["participant_id"].to_numpy()))
    return sets


def _read(path):
    import pandas as pd
    return pd.read_csv(path, float_precision="round_trip")


def _held_to_a_pool_by_hand(root, sets, do):
    """Fold k's row of the `others` file against a selection on the other folds' rows without fold k's own subjects."""
    for k in range(K):
        rest = [j for j in range(K) if j != k]
        keep = [~np.isin(sets[j][2], sets[k][2]) for j in rest]
        ps = np.concatenate([sets[j][0][m] for j, m in zip(rest, keep)])
        pl = np.concatenate([sets[j][1][m] for j, m in zip(rest, keep)])
        sk, lk = torch.from_numpy(sets[k][0]), torch.from_numpy(sets[k][1])
        hand, _ = metrics.operating_points([torch.from_numpy(ps), sk], [torch.from_numpy(pl), lk], rules=(RULE,),
                                           select_of=[0, 0], evaluate=[0, 1])
        hand = hand.cpu().numpy()
        assert do.iloc[k, 1:].to_numpy(dtype=np.float64).tobytes() == hand[1, 0].tobytes(), k
        pred = sets[k][0].astype(np.float64) >= hand[0, 0, 0]
        assert (do["tp"][k], do["fp"][k]) == ((pred & (sets[k][1] != 0)).sum(), (pred & (sets[k][1] == 0)).sum())


def test_files_self_rows_other_folds_and_the_untouched_rest(tree):
    root = tree / "HCPimage" / P
    args = ["-P", P, "--models-dir", str(tree)] + COMMON
    base = sweep.main_analysis(args)
    before = (root / "group_analysis.csv").read_bytes()
    listed = sorted(p.name for p in root.iterdir())
    again = sweep.main_analysis(args)
    assert sorted(p.name for p in root.iterdir()) == listed and again.numpy().tobytes() == base.numpy().tobytes()

    sets = _sets(root)
    sc = [torch.from_numpy(s) for s, _, _ in sets] + [torch.from_numpy(np.concatenate([s for s, _, _ in sets]))]
    la = [torch.from_numpy(l) for _, l, _ in sets] + [torch.from_numpy(np.concatenate([l for _, l, _ in sets]))]
    names = [str(k) for k in range(K)] + ["pooled"]

    # self: per fold and pooled, the direct call's bytes
    tab = sweep.main_analysis(args + ["--threshold-rule", RULE, "--roc-grid", str(G)])
    assert tab.numpy().tobytes() == base.numpy().tobytes() and (root / "group_analysis.csv").read_bytes() == before
    assert sorted(p.name for p in root.iterdir()) == sorted(listed + NEW)
    pts, summ, grid = (t.cpu().numpy() for t in metrics.operating_points(sc, la, rules=(RULE,), roc_grid=G))
    df = _read(root / NEW[0])
    assert list(df.columns) == ["fold"] + list(metrics.OPERATING_POINT_COLUMNS) and [str(v) for v in df["fold"]] == names
    assert df.iloc[:, 1:].to_numpy(dtype=np.float64).tobytes() == pts[:, 0].tobytes()
    dc = _read(root / NEW[1])
    assert list(dc.columns) == ["fold"] + list(metrics.ROC_SUMMARY_COLUMNS) and [str(v) for v in dc["fold"]] == names
    assert dc.iloc[:, 1:].to_numpy(dtype=np.float64).tobytes() == summ.tobytes()
    assert np.array_equal(dc["roc_auc"].to_numpy()[:K], base.numpy()[:, 0])
    dr = _read(root / NEW[2])
    assert list(dr.columns) == ["fpr", "mean_tpr", "sd_tpr"] + [f"tpr_fold_{k}" for k in range(K)] and len(dr) == G
    assert np.array_equal(dr["fpr"].to_numpy(), np.linspace(0, 1, G))
    assert dr.iloc[:, 3:].to_numpy(dtype=np.float64).T.tobytes() == grid[:K].tobytes()
    assert np.array_equal(dr["mean_tpr"].to_numpy(), grid[:K].mean(axis=0)) and np.array_equal(dr["sd_tpr"].to_numpy(), grid[:K].std(axis=0))
    assert dr["mean_tpr"].iloc[-1] == 1.0 and np.all(np.diff(dr["mean_tpr"].to_numpy()) >= 0)
    self_thr = df["threshold"].to_numpy()[:K]

    # others: fold k with the threshold of the other folds' rows, the fold's own subjects left out of them
    flags = ["--threshold-rule", RULE, "--threshold-from", "others", "--roc-grid", str(G)]
    sweep.main_analysis(args + flags)
    assert sorted(p.name for p in root.iterdir()) == sorted(listed + NEW)
    first = {n: (root / n).read_bytes() for n in NEW}
    do = _read(root / NEW[0])
    assert list(do.columns) == ["fold"] + list(metrics.OPERATING_POINT_COLUMNS) and [str(v) for v in do["fold"]] == names[:K]
    _held_to_a_pool_by_hand(root, sets, do)
    assert _read(root / NEW[1]).iloc[:, 1:].to_numpy(dtype=np.float64).tobytes() == summ.tobytes()
    assert not np.array_equal(do["threshold"].to_numpy(), self_thr)      # (another set of subjects chose it)
    sweep.main_analysis(args + flags)
    assert {n: (root / n).read_bytes() for n in NEW} == first
    for n in NEW:
        (root / n).unlink()
    assert sorted(p.name for p in root.iterdir()) == listed


def test_subjects_shared_between_folds_stay_out_of_the_pool(tree):
    """A cohort recipe that repeats subjects across test folds (the reference's puts every patient into every fold): the rows
    fold 0 shares with fold 1 must not help to choose fold 0's threshold, nor the other way round."""
    import pandas as pd
    mods, _ = workload.procedure_modalities(P, "HCPimage")
    with tempfile.TemporaryDirectory() as d:
        other = Path(d) / "t"
        shutil.copytree(tree, other, ignore=shutil.ignore_patterns("*.pt", "*.pth", "*.bin"))
        root = other / "HCPimage" / P
        for m in mods:                                                 # fold 1 also holds the first 40 subjects of fold 0
            f0, f1 = (root / f"{k:03d}" / m / f"reconstruction_error_{m}.csv" for k in (0, 1))
            pd.concat([pd.read_csv(f1), pd.read_csv(f0).iloc[:40]]).to_csv(f1, index=False)
        sets = _sets(root)
        assert np.isin(sets[1][2], sets[0][2]).sum() >= 40 and np.isin(sets[0][2], sets[1][2]).sum() >= 40
        sweep.main_analysis(["-P", P, "--models-dir", str(other), "--threshold-rule", RULE, "--threshold-from", "others"] + COMMON)
        _held_to_a_pool_by_hand(root, sets, _read(root / NEW[0]))


def test_flag_conflicts_are_refused(tree):
    args = ["-P", P, "--models-dir", str(tree)] + COMMON
    for bad in (["--threshold-from", "others"], ["--threshold-rule", "roc", "--roi"], ["--roc-grid", "1"], ["--roc-grid", "5000"],
                ["--threshold-rule", "f1", "--threshold-grid", "0", "1", "1"], ["--threshold-rule", "spec", "--spec", "1.5"]):
        with pytest.raises(SystemExit):
            sweep.main_analysis(args + bad)
