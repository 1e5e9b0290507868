"""The normative z-map through the sweep: test_folds(..., normative=...) per fold and pooled and latent_folds(..., mahalanobis=True)
against the yardstick (tests/normative_ref.py) on the tables the jobs exported, the files they write, the untouched default, and
the command line down to `analysis --score extreme / mahalanobis`.  The cohort of tests/table_stats_util.py: 120
synthetic subjects with three diagnoses, two folds, two modalities of different widths, one epoch.  The closeness rules are those
of tests/test_gpu_normative.py; the Mahalanobis bound 1e-9 is stated for condition numbers <= 1e3 and grows in proportion above
(the error is Z x cond x 2^-52): the yardstick's condition number is printed and enters the bound."""
import filecmp
import shutil
import tempfile
from pathlib import Path

import numpy as np
import pytest
import torch

from multi_modal_normative_modeling_amd import io, metrics, prep, sweep
from oracle import metrics_ref
from tests import normative_ref as R
from tests.table_stats_util import trained_cohort

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
THR = 1.96


@pytest.fixture(scope="module")
def trained():
    return trained_cohort(120, 2, DEV)


def _files(root):
    return sorted(p.relative_to(root) for p in Path(root).rglob("*") if p.is_file())


def _same(a, b):
    return np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)


def _check_set(t, g, what):
    """One {"z", "rows", "cols", "moments", "x", "sub"} dict against the yardstick on its own x / sub."""
    x, sub = t["x"], t["sub"]
    mom = R.moments(x, g, sub, 1)
    z = R.z_table(x, mom, sub)
    with np.errstate(invalid="ignore"):                            # the conditions the exact counts rest on (inputs, not the kernel)
        assert not np.any(np.abs(np.abs(z) - THR) < 1e-6) and not np.any(np.abs(mom[:, 0]) / mom[:, 1] > 1e3)
    worst = [R.close(t["moments"], mom, "moments"), R.close(t["z"], z, "z32"), R.close(t["rows"], R.row_summary(z, THR), "rows"),
             R.close(t["cols"], R.col_summary(z, g, mom, THR), "cols")]
    print(what, "worst error / bound (moments, z, rows, cols):", worst, "n_ref", mom[0, 3])
    assert max(worst) <= 1.0, what
    assert np.all(mom[:, 7] == 0) and t["z"].dtype == np.float32


@pytest.mark.parametrize("kind", ["squared", "signed"])
def test_test_folds_normative(trained, monkeypatch, kind):
    import pandas as pd
    cohort, folds, mods, jobs = trained
    evs = []
    inner = sweep._fold_eval_job

    def spy(*a, **k):
        ev, xs = inner(*a, **k)
        evs.append((ev, xs))
        return ev, xs
    with tempfile.TemporaryDirectory() as d:
        a, b = Path(d) / "a", Path(d) / "b"
        dirs_a, dirs_b = [a / f"{k:03d}" for k in range(2)], [b / f"{k:03d}" for k in range(2)]
        monkeypatch.setattr(sweep, "_fold_eval_job", spy)
        res = sweep.test_folds(jobs, cohort, folds, mods, "gpoe", DEV, out_dirs=dirs_a, roi_effect=True, normative=kind, z_thr=THR)
        monkeypatch.undo()
        base = sweep.test_folds(jobs, cohort, folds, mods, "gpoe", DEV, out_dirs=dirs_b, roi_effect=True)
        # every key and file from before: the same bytes
        for r, r0 in zip(res, base):
            assert set(r) == set(r0) | {"normative", "normative_pooled"}
            assert all(r[m].tobytes() == r0[m].tobytes() for m in mods)
            assert all(_same(r["roi_effect"][m], r0["roi_effect"][m]) and _same(r["roi_effect_pooled"][m], r0["roi_effect_pooled"][m])
                       for m in mods)
        fa, fb = _files(a), _files(b)
        assert all(filecmp.cmp(a / p, b / p, shallow=False) for p in fb)
        assert sorted(set(fa) - set(fb)) == sorted(Path(f"{k:03d}") / m / f"normative_{w}_{m}.csv" for k in range(2) for m in mods
                                                   for w in ("z", "subject", "map"))
        grp = [sweep.roi_groups(cohort.dia[te]) for _, te in folds]
        for i, m in enumerate(mods):
            D = (40, 23)[i]
            for k in range(3):
                t = res[k]["normative"][m] if k < 2 else res[0]["normative_pooled"][m]
                g = grp[k] if k < 2 else np.concatenate(grp)
                assert t["z"].shape == (len(g), D) and t["rows"].shape == (len(g), 8) and t["cols"].shape == (D, 8)
                # the tables that were scored are the jobs' own exports
                if k < 2:
                    ev, xs = evs[k]
                    n = len(g)
                    if kind == "squared":
                        assert t["sub"] is None and _same(t["x"], ev.out_sqerr[i][:n].cpu().numpy())
                    else:
                        assert _same(t["x"], xs[i]) and _same(t["sub"], ev.out_loc[i][:n].cpu().numpy())
                else:
                    assert _same(t["x"], np.concatenate([res[f]["normative"][m]["x"] for f in range(2)]))
                _check_set(t, g, f"{kind} {m} set {k}")
                # every subject of any group is scored; the controls' mean z is zero by construction
                assert np.all(t["rows"][:, 6] == D) and np.all(t["rows"][:, 7] == 0)
                assert np.all(t["cols"][:, 4] == (g == 1).sum()) and np.all(t["cols"][:, 5] == (g == 0).sum())
                assert np.nanmax(np.abs(t["cols"][:, 7])) < 1e-9
                if k < 2:
                    te = folds[k][1]
                    zf = pd.read_csv(dirs_a[k] / m / f"normative_z_{m}.csv", float_precision="round_trip")
                    sf = pd.read_csv(dirs_a[k] / m / f"normative_subject_{m}.csv", float_precision="round_trip")
                    mf = pd.read_csv(dirs_a[k] / m / f"normative_map_{m}.csv", float_precision="round_trip")
                    assert list(zf.columns) == io.META_COLS + [f"{m}_{j}" for j in range(D)] and len(zf) == len(te)
                    assert list(sf.columns) == io.META_COLS + list(metrics.NORMATIVE_ROW_COLUMNS) and len(sf) == len(te)
                    assert list(mf.columns) == ["ROI"] + list(metrics.NORMATIVE_COL_COLUMNS) and len(mf) == D
                    assert list(zf["participant_id"]) == list(cohort.iid[te]) and list(sf["DIA"]) == list(cohort.dia[te])
                    assert _same(zf.iloc[:, 4:].to_numpy(dtype=np.float32), t["z"]) and _same(sf.iloc[:, 4:].to_numpy(dtype=np.float64), t["rows"])
                    assert _same(mf.iloc[:, 1:].to_numpy(dtype=np.float64), t["cols"])
            assert all(r["normative_pooled"][m] is res[0]["normative_pooled"][m] for r in res)
    with pytest.raises(ValueError):
        sweep.test_folds(jobs, cohort, folds, mods, "gpoe", DEV, normative=kind)


def test_latent_folds_mahalanobis(trained, monkeypatch, capsys):
    import pandas as pd
    cohort, folds, mods, jobs = trained
    pairs = []
    inner = sweep._fold_latent_jobs

    def spy(*a, **k):
        pr = inner(*a, **k)
        pairs.append(pr)
        return pr
    with tempfile.TemporaryDirectory() as d:
        a, b = Path(d) / "a", Path(d) / "b"
        dirs_a, dirs_b = [a / f"{k:03d}" for k in range(2)], [b / f"{k:03d}" for k in range(2)]
        monkeypatch.setattr(sweep, "_fold_latent_jobs", spy)
        res = sweep.latent_folds(jobs, cohort, folds, mods, "gpoe", DEV, out_dirs=dirs_a, name="SE-gPoE", mahalanobis=True, ridge=1e-3)
        monkeypatch.undo()
        base = sweep.latent_folds(jobs, cohort, folds, mods, "gpoe", DEV, out_dirs=dirs_b, name="SE-gPoE")
        for r, r0 in zip(res, base):
            assert set(r0) == {"mu", "var", "z", "score"} and set(r) == set(r0) | {"mahalanobis"}
            assert all(r[k].tobytes() == r0[k].tobytes() for k in r0)
        fa, fb = _files(a), _files(b)
        assert len(fb) == 4 and all(filecmp.cmp(a / p, b / p, shallow=False) for p in fb)
        assert sorted(set(fa) - set(fb)) == sorted(Path(f"{k:03d}") / "latent_mahalanobis_SE-gPoE.csv" for k in range(2))
        for k, (tr, te) in enumerate(folds):
            trn_mu = pairs[k][0].out_mu[:len(tr)].cpu().numpy()
            mean, L, st = R.cov_chol(trn_mu, np.zeros(len(tr), dtype=np.int32), ridge=1e-3)
            assert st == 0
            cond = np.linalg.cond(L @ L.T)
            want = np.sqrt(R.mahalanobis(res[k]["mu"], mean, L, st))
            worst = R.close(res[k]["mahalanobis"], want, "rel", tol=1e-9 * max(1.0, cond / 1e3))
            print("fold", k, "cond", cond, "worst error / bound", worst, "mean d", want.mean())
            assert worst <= 1.0 and res[k]["mahalanobis"].dtype == np.float64 and res[k]["mahalanobis"].shape == (len(te),)
            df = pd.read_csv(dirs_a[k] / "latent_mahalanobis_SE-gPoE.csv", float_precision="round_trip")
            assert list(df.columns) == io.META_COLS + ["d2", "d"] and list(df["participant_id"]) == list(cohort.iid[te])
            assert _same(df["d"].to_numpy(dtype=np.float64), res[k]["mahalanobis"])
        # a train cohort without a factor: NaN and a line that says which fold and why
        capsys.readouterr()
        few = [(tr[:5], te) for tr, te in folds[:1]]                # 5 subjects, Z = 8, no ridge
        out = sweep.latent_folds(jobs[:1], cohort, few, mods, "gpoe", DEV, mahalanobis=True)
        assert np.isnan(out[0]["mahalanobis"]).all() and "fold 0: no Mahalanobis distance" in capsys.readouterr().out
    with pytest.raises(ValueError):
        sweep.latent_folds(jobs, cohort, folds, mods, "gpoe", DEV, mahalanobis=True, ridge=-1.0)


def test_command_line_with_and_without_the_flags(capsys):
    """`sweep test --latent --roi-effect` writes exactly the files it wrote before unless the new flags are given; with them the
    named files per fold and all folds, and `analysis --score extreme / zmean / mahalanobis` scores their columns: the AUC is the
    oracle's on the same column."""
    import pandas as pd
    with tempfile.TemporaryDirectory() as d:
        a, b = Path(d) / "a", Path(d) / "b"
        sweep.main(["-P", "SE-gPoE", "-E", "2", "-K", "2", "-H", "32", "24", "8", "--subjects", "300", "--out-dir", str(a),
                    "--save-models", "--no-csv"])
        shutil.copytree(a, b)
        common = ["-P", "SE-gPoE", "-K", "2", "-H", "32", "24", "8", "--subjects", "300", "--latent", "--roi-effect"]
        ea = sweep.main_test(common + ["--models-dir", str(a)])
        eb = sweep.main_test(common + ["--models-dir", str(b), "--normative", "squared", "--z-thr", "2.5", "--mahalanobis",
                                       "--ridge", "1e-3"])
        assert all(np.array_equal(ea[m], eb[m]) for m in ea)
        fa, fb = _files(a), _files(b)
        base = Path("HCPimage") / "SE-gPoE"
        mods = list(prep.HCP_MODALITIES)
        want = [base / f"{k:03d}" / m / f"normative_{w}_{m}.csv" for k in (0, 1) for m in mods for w in ("z", "subject", "map")]
        want += [base / m / f"normative_{w}_{m}.csv" for m in mods for w in ("z", "subject", "map")]
        want += [base / f"{k:03d}" / "latent_mahalanobis_SE-gPoE.csv" for k in (0, 1)] + [base / "latent_mahalanobis_SE-gPoE.csv"]
        assert sorted(set(fb) - set(fa)) == sorted(want) and set(fa) <= set(fb)
        for p in fa:
            if p.suffix == ".csv":
                assert filecmp.cmp(a / p, b / p, shallow=False), p
        assert len(pd.read_csv(b / base / "latent_mahalanobis_SE-gPoE.csv")) == 300
        assert len(pd.read_csv(b / base / mods[0] / f"normative_subject_{mods[0]}.csv")) == 300
        # the pooled map is the launch on the all-folds squared errors against their own controls
        for m in mods[:1]:
            allf = pd.read_csv(b / base / m / f"reconstruction_error_roi_{m}.csv", float_precision="round_trip")
            got = pd.read_csv(b / base / m / f"normative_map_{m}.csv", float_precision="round_trip").iloc[:, 1:].to_numpy(dtype=np.float64)
            assert np.all(got[:, 4] + got[:, 5] == 300) and np.all(got[:, 4] == (allf["DIA"].to_numpy() != 1).sum())
        before = _files(b)
        for score, column in (("extreme", None), ("zmean", "mean_abs_z"), ("mahalanobis", "d")):
            tab = sweep.main_analysis(["-P", "SE-gPoE", "-K", "2", "--models-dir", str(b), "--score", score]).numpy()
            out = pd.read_csv(b / base / f"group_analysis_{score}.csv", float_precision="round_trip")
            assert list(out.columns) == ["fold"] + list(metrics.POSTHOC_COLUMNS) and list(out["fold"]) == [0, 1]
            for k in (0, 1):
                if score == "mahalanobis":
                    dfs = [pd.read_csv(b / base / f"{k:03d}" / "latent_mahalanobis_SE-gPoE.csv")]
                    s = dfs[0]["d"].to_numpy(dtype=np.float64)
                else:
                    dfs = [pd.read_csv(b / base / f"{k:03d}" / m / f"normative_subject_{m}.csv") for m in mods]
                    s = sum(((f["n_hi"] + f["n_lo"]) if column is None else f[column]).to_numpy(dtype=np.float64) for f in dfs) / len(dfs)
                ref = metrics_ref.posthoc_metrics(s.astype(np.float32), (dfs[0]["DIA"].to_numpy() != 1).astype(int))
                # (the device's AUC is the exactly rounded integer trapezoid sum, the oracle's a float sum of at most n + 1 terms
                # <= 1: they agree to (n + 1) 2^-53 < 1e-13)
                assert np.isfinite(s).all() and abs(tab[k, 0] - ref[0]) <= 1e-13 and tab[k, 0] == out["roc_auc"][k], (score, k)
                assert tab[k, 6] == ref[6] and tab[k, 7] == ref[7] and 0.0 < tab[k, 0] < 1.0, (score, k)
        assert sorted(set(_files(b)) - set(before)) == sorted(base / f"group_analysis_{s}.csv" for s in ("extreme", "zmean", "mahalanobis"))
        # --bootstrap rides on the same scores
        sweep.main_analysis(["-P", "SE-gPoE", "-K", "2", "--models-dir", str(b), "--score", "extreme", "--bootstrap", "200"])
        boot = pd.read_csv(b / base / "group_analysis_extreme_bootstrap.csv")
        assert list(boot["fold"]) == ["0", "1", "pooled"] and np.all(boot["ci_lo"] <= boot["roc_auc"]) and np.all(boot["roc_auc"] <= boot["ci_hi"])
