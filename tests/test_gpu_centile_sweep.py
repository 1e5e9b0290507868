"""The normative centiles through the sweep: test_folds(..., centile=...) per fold and pooled against the metrics calls made by
hand and against the yardstick (tests/centile_ref.py, bit for bit) on the tables the jobs exported, the files it writes (the
same bytes on a second run), the untouched default, robust=True, and the command line down to `analysis --centile-score`.
The cohort of tests/table_stats_util.py: 120 synthetic subjects with three diagnoses, two folds, two modalities of different
widths, one epoch."""
import filecmp
import shutil
import tempfile
from pathlib import Path

import numpy as np
import pytest
import torch

from multi_modal_normative_modeling_amd import io, metrics, prep, sweep
from tests import centile_ref as R
from tests.table_stats_util import same_bits, trained_cohort

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
PROBS = (0.025, 0.5, 0.975)
CENTILE_FILES = ("pct", "subject", "map", "curve")


@pytest.fixture(scope="module")
def trained():
    return trained_cohort(120, 2, DEV)


def _files(root):
    return sorted(p.relative_to(root) for p in Path(root).rglob("*") if p.is_file())


def _same(a, b):
    return np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)


def _check_set(t, g, tail, loo, what):
    """One {"pct", "rows", "cols", "q", "stats", "x", "sub"} dict against the metrics calls made by hand and the yardstick."""
    x = torch.from_numpy(t["x"]).to(DEV)
    sub = None if t["sub"] is None else [torch.from_numpy(t["sub"]).to(DEV)]
    q, st = metrics.cohort_quantiles([x], [g], PROBS, sub=sub)
    pct, rows, cols = metrics.normative_centile([x], [g], tail=tail, loo=loo, sub=sub)
    for name, got in (("q", q[0]), ("stats", st[0]), ("pct", pct[0]), ("rows", rows), ("cols", cols[0])):
        assert t[name].tobytes() == got.cpu().numpy().tobytes(), (what, name)
    wq, wst = R.cohort_quantiles(t["x"], g, PROBS, t["sub"])
    wpct, wrows, wcols = R.normative_centile([(t["x"], g, t["sub"])], None, tail, loo)[0]
    assert same_bits(t["q"], wq) and same_bits(t["stats"], wst) and same_bits(t["pct"], wpct), what
    assert same_bits(t["rows"], wrows) and same_bits(t["cols"], wcols), what
    assert t["pct"].dtype == np.float32 and np.all(wst[:, 7] == 0)


@pytest.mark.parametrize("kind,loo", [("squared", False), ("signed", True)])
def test_test_folds_centile(trained, kind, loo):
    import pandas as pd
    cohort, folds, mods, jobs = trained
    tail = 5.0
    with tempfile.TemporaryDirectory() as d:
        a, b, c = Path(d) / "a", Path(d) / "b", Path(d) / "c"
        dirs = {r: [r / f"{k:03d}" for k in range(2)] for r in (a, b, c)}
        kw = dict(roi_effect=True, centile=kind, tail=tail, quantiles=PROBS, centile_loo=loo)
        res = sweep.test_folds(jobs, cohort, folds, mods, "gpoe", DEV, out_dirs=dirs[a], **kw)
        base = sweep.test_folds(jobs, cohort, folds, mods, "gpoe", DEV, out_dirs=dirs[b], roi_effect=True)
        sweep.test_folds(jobs, cohort, folds, mods, "gpoe", DEV, out_dirs=dirs[c], **kw)
        # every key and file from before: the same bytes; the new files: the same bytes on a second run
        for r, r0 in zip(res, base):
            assert set(r) == set(r0) | {"centile", "centile_pooled"}
            assert all(r[m].tobytes() == r0[m].tobytes() for m in mods)
            assert all(_same(r["roi_effect"][m], r0["roi_effect"][m]) for m in mods)
        fa, fb, fc = _files(a), _files(b), _files(c)
        assert fa == fc and all(filecmp.cmp(a / p, c / p, shallow=False) for p in fa)
        assert all(filecmp.cmp(a / p, b / p, shallow=False) for p in fb)
        assert sorted(set(fa) - set(fb)) == sorted(Path(f"{k:03d}") / m / f"centile_{w}_{m}.csv" for k in range(2) for m in mods
                                                   for w in CENTILE_FILES)
        grp = [sweep.roi_groups(cohort.dia[te]) for _, te in folds]
        for i, m in enumerate(mods):
            D = (40, 23)[i]
            for k in range(3):
                t = res[k]["centile"][m] if k < 2 else res[0]["centile_pooled"][m]
                g = grp[k] if k < 2 else np.concatenate(grp)
                assert t["pct"].shape == (len(g), D) and t["rows"].shape == (len(g), 8) and t["cols"].shape == (D, 8)
                assert t["q"].shape == (D, len(PROBS)) and t["stats"].shape == (D, 8) and (t["sub"] is None) == (kind == "squared")
                if k == 2:
                    assert _same(t["x"], np.concatenate([res[f]["centile"][m]["x"] for f in range(2)]))
                _check_set(t, g, tail, loo, f"{kind} {m} set {k}")
                # every subject of any group is ranked; without leave-one-out the controls' mean rank is 50 by construction
                assert np.all(t["rows"][:, 6] == D) and np.all(t["rows"][:, 7] == 0)
                assert np.all(t["cols"][:, 4] == (g == 1).sum()) and np.all(t["cols"][:, 5] == (g == 0).sum())
                if not loo:
                    assert np.max(np.abs(t["cols"][:, 7] - 50.0)) < 1e-9
                assert np.all(t["q"][:, 0] <= t["q"][:, 1]) and np.all(t["q"][:, 1] <= t["q"][:, 2]) and _same(t["q"][:, 1], t["stats"][:, 0])
                if k < 2:
                    te = folds[k][1]
                    rd = {w: pd.read_csv(dirs[a][k] / m / f"centile_{w}_{m}.csv", float_precision="round_trip") for w in CENTILE_FILES}
                    assert list(rd["pct"].columns) == io.META_COLS + [f"{m}_{j}" for j in range(D)] and len(rd["pct"]) == len(te)
                    assert list(rd["subject"].columns) == io.META_COLS + list(metrics.CENTILE_ROW_COLUMNS)
                    assert list(rd["map"].columns) == ["ROI"] + list(metrics.CENTILE_COL_COLUMNS) and len(rd["map"]) == D
                    assert list(rd["curve"].columns) == ["ROI"] + [io.quantile_column(p) for p in PROBS] + list(metrics.COHORT_QUANTILE_COLUMNS)
                    assert list(rd["pct"]["participant_id"]) == list(cohort.iid[te]) and list(rd["subject"]["DIA"]) == list(cohort.dia[te])
                    assert _same(rd["pct"].iloc[:, 4:].to_numpy(dtype=np.float32), t["pct"])
                    assert _same(rd["subject"].iloc[:, 4:].to_numpy(dtype=np.float64), t["rows"])
                    assert _same(rd["map"].iloc[:, 1:].to_numpy(dtype=np.float64), t["cols"])
                    assert _same(rd["curve"].iloc[:, 1:].to_numpy(dtype=np.float64), np.concatenate([t["q"], t["stats"]], axis=1))
            assert all(r["centile_pooled"][m] is res[0]["centile_pooled"][m] for r in res)
    with pytest.raises(ValueError):
        sweep.test_folds(jobs, cohort, folds, mods, "gpoe", DEV, centile=kind)


def test_robust_changes_only_the_normative_files(trained):
    cohort, folds, mods, jobs = trained
    with tempfile.TemporaryDirectory() as d:
        a, b = Path(d) / "a", Path(d) / "b"
        dirs_a, dirs_b = [a / f"{k:03d}" for k in range(2)], [b / f"{k:03d}" for k in range(2)]
        kw = dict(roi_effect=True, normative="squared", centile="squared", quantiles=PROBS)
        plain = sweep.test_folds(jobs, cohort, folds, mods, "gpoe", DEV, out_dirs=dirs_a, **kw)
        robust = sweep.test_folds(jobs, cohort, folds, mods, "gpoe", DEV, out_dirs=dirs_b, robust=True, **kw)
        fa, fb = _files(a), _files(b)
        assert fa == fb
        differ = [p for p in fa if not filecmp.cmp(a / p, b / p, shallow=False)]
        assert differ and all(p.name.startswith("normative_") for p in differ), differ
        for k in range(2):
            for m in mods:
                t, c = robust[k]["normative"][m], robust[k]["centile"][m]
                want = R.robust_moments(c["stats"])
                assert same_bits(t["moments"], want) and np.all(want[:, 7] == 0)
                z = (t["x"].astype(np.float64) - want[:, 0]) / want[:, 1]
                assert np.allclose(t["z"], z.astype(np.float32), rtol=1e-6, atol=0) and not _same(t["z"], plain[k]["normative"][m]["z"])
                assert all(plain[k]["centile"][m][n].tobytes() == c[n].tobytes() for n in ("pct", "rows", "cols", "q", "stats"))
    with pytest.raises(ValueError):
        sweep.test_folds(jobs, cohort, folds, mods, "gpoe", DEV, roi_effect=True, robust=True)


def test_command_line_with_and_without_the_flags():
    """`sweep test --roi-effect` writes exactly the files it wrote before unless the new flags are given; with them the named
    files per fold and all folds, and `analysis --centile-score tails / depth` scores their columns: the AUC is
    metrics.posthoc_metrics' on the same column."""
    import pandas as pd
    with tempfile.TemporaryDirectory() as d:
        a, b = Path(d) / "a", Path(d) / "b"
        sweep.main(["-P", "SE-gPoE", "-E", "2", "-K", "2", "-H", "32", "24", "8", "--subjects", "300", "--out-dir", str(a),
                    "--save-models", "--no-csv"])
        shutil.copytree(a, b)
        common = ["-P", "SE-gPoE", "-K", "2", "-H", "32", "24", "8", "--subjects", "300", "--roi-effect"]
        ea = sweep.main_test(common + ["--models-dir", str(a)])
        eb = sweep.main_test(common + ["--models-dir", str(b), "--centile", "squared", "--tail", "5", "--quantiles", "0.1", "0.9",
                                       "--centile-loo"])
        assert all(np.array_equal(ea[m], eb[m]) for m in ea)
        fa, fb = _files(a), _files(b)
        base = Path("HCPimage") / "SE-gPoE"
        mods = list(prep.HCP_MODALITIES)
        want = [base / f"{k:03d}" / m / f"centile_{w}_{m}.csv" for k in (0, 1) for m in mods for w in CENTILE_FILES]
        want += [base / m / f"centile_{w}_{m}.csv" for m in mods for w in CENTILE_FILES]
        assert sorted(set(fb) - set(fa)) == sorted(want) and set(fa) <= set(fb)
        assert not any("centile" in p.name for p in fa)
        for p in fa:
            if p.suffix == ".csv":
                assert filecmp.cmp(a / p, b / p, shallow=False), p
        m0 = mods[0]
        assert len(pd.read_csv(b / base / m0 / f"centile_subject_{m0}.csv")) == 300
        assert list(pd.read_csv(b / base / m0 / f"centile_curve_{m0}.csv").columns)[:3] == ["ROI", "q_0.1", "q_0.9"]
        before = _files(b)
        for kind, column in (("tails", None), ("depth", "mean_abs_dev")):
            tab = sweep.main_analysis(["-P", "SE-gPoE", "-K", "2", "--models-dir", str(b), "--centile-score", kind]).numpy()
            out = pd.read_csv(b / base / f"group_analysis_centile_{kind}.csv", float_precision="round_trip")
            assert list(out.columns) == ["fold"] + list(metrics.POSTHOC_COLUMNS) and list(out["fold"]) == [0, 1]
            for k in (0, 1):
                dfs = [pd.read_csv(b / base / f"{k:03d}" / m / f"centile_subject_{m}.csv") for m in mods]
                s = sum(((f["n_hi"] + f["n_lo"]) if column is None else f[column]).to_numpy(dtype=np.float64) for f in dfs) / len(dfs)
                pos = (dfs[0]["DIA"].to_numpy() != 1).astype(np.int32)
                ref = metrics.posthoc_metrics([torch.as_tensor(s, dtype=torch.float32)], [torch.as_tensor(pos)]).cpu().numpy()[0]
                assert np.isfinite(s).all() and tab[k].tobytes() == ref.tobytes() and tab[k, 0] == out["roc_auc"][k], (kind, k)
                assert 0.0 < tab[k, 0] < 1.0
        assert sorted(set(_files(b)) - set(before)) == sorted(base / f"group_analysis_centile_{s}.csv" for s in ("tails", "depth"))
        # --bootstrap rides on the same scores
        sweep.main_analysis(["-P", "SE-gPoE", "-K", "2", "--models-dir", str(b), "--centile-score", "tails", "--bootstrap", "200"])
        boot = pd.read_csv(b / base / "group_analysis_centile_tails_bootstrap.csv")
        assert list(boot["fold"]) == ["0", "1", "pooled"] and np.all(boot["ci_lo"] <= boot["roc_auc"]) and np.all(boot["roc_auc"] <= boot["ci_hi"])
