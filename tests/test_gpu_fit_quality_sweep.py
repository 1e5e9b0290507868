"""The model-fit statistics through the sweep: test_folds(..., roi_effect=True, fit=True, fit_rank=True), plain and after a
posterior-predictive pass (draws=4), per fold and pooled, recomputed with the yardstick (tests/fit_quality_ref.py) from the
tables the jobs exported and from train moments formed in numpy; the files it writes (the same bytes on a second run), the
untouched default, and the command line down to `analysis --fit`.  The cohort of tests/table_stats_util.py: 120 synthetic
subjects with three diagnoses, two folds, two modalities of widths 40 and 23, one epoch."""
import filecmp
import shutil
import tempfile
from pathlib import Path

import numpy as np
import pytest
import torch

from multi_modal_normative_modeling_amd import io, metrics, prep, sweep
from tests import fit_quality_ref as R
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


def _train_moments(x):
    """The trivial model of a fold in numpy: the [D, 8] moments row of the scaled train table, ddof 0."""
    v = np.asarray(x, dtype=np.float64)
    out = np.zeros((v.shape[1], 8))
    out[:, 0], out[:, 2], out[:, 3], out[:, 4], out[:, 5] = v.mean(0), v.var(0), len(v), v.min(0), v.max(0)
    out[:, 1] = np.sqrt(out[:, 2])
    return out


@pytest.mark.parametrize("draws", [None, 4])
def test_test_folds_fit(trained, draws):
    import pandas as pd
    cohort, folds, mods, jobs = trained
    with tempfile.TemporaryDirectory() as d:
        a, b, c = Path(d) / "a", Path(d) / "b", Path(d) / "c"
        dirs = {r: [r / f"{k:03d}" for k in range(2)] for r in (a, b, c)}
        kw = dict(roi_effect=True, fit=True, fit_rank=True, draws=draws)
        res = sweep.test_folds(jobs, cohort, folds, mods, "gpoe", DEV, out_dirs=dirs[a], **kw)
        base = sweep.test_folds(jobs, cohort, folds, mods, "gpoe", DEV, out_dirs=dirs[b], roi_effect=True, draws=draws)
        sweep.test_folds(jobs, cohort, folds, mods, "gpoe", DEV, out_dirs=dirs[c], **kw)
        # every key and file from before: the same bytes; the new files: the same bytes on a second run
        for r, r0 in zip(res, base):
            assert set(r) == set(r0) | {"fit", "fit_pooled"}
            assert all(r[m].tobytes() == r0[m].tobytes() for m in mods)
            assert all(_same(r["roi_effect"][m], r0["roi_effect"][m]) for m in mods)
        fa, fb, fc = _files(a), _files(b), _files(c)
        assert fa == fc and all(filecmp.cmp(a / p, c / p, shallow=False) for p in fa)
        assert all(filecmp.cmp(a / p, b / p, shallow=False) for p in fb)
        assert sorted(set(fa) - set(fb)) == sorted(Path(f"{k:03d}") / m / f"fit_quality_{m}.csv" for k in range(2) for m in mods)
        grp = [sweep.roi_groups(cohort.dia[te]) for _, te in folds]
        for i, m in enumerate(mods):
            D = (40, 23)[i]
            for k in range(3):
                t = res[k]["fit"][m] if k < 2 else res[0]["fit_pooled"][m]
                g = grp[k] if k < 2 else np.concatenate(grp)
                assert t["fit"].shape == t["cal"].shape == t["rank"].shape == (D, 8) and t["x"].shape == t["loc"].shape == (len(g), D)
                if k < 2:
                    triv = _train_moments(prep.fold_train_tables(cohort, mods, folds[k][0])[0][i])
                    assert t["col_var"].shape == (D,) and t["col_var"].dtype == np.float32 and (t["var"] is None) == (draws is None)
                    if draws is not None:
                        assert _same(t["loc"], res[k]["predictive"][m]["mean"]) and _same(t["var"], res[k]["predictive"][m]["var"])
                else:
                    triv = None                                         # rows of several scalers: no trivial model
                    parts = [res[f]["fit"][m] for f in range(2)]
                    assert t["col_var"] is None and _same(t["x"], np.concatenate([p["x"] for p in parts]))
                    assert _same(t["loc"], np.concatenate([p["loc"] for p in parts]))
                    want_var = [np.broadcast_to(p["col_var"], p["x"].shape) if p["var"] is None else p["var"] + p["col_var"] for p in parts]
                    assert t["var"].dtype == np.float32 and _same(t["var"], np.concatenate(want_var))
                fit, cal = R.quality(t["x"], t["loc"], g, t["var"], t["col_var"], triv, thr=THR)
                rk = R.rank(t["x"], t["loc"], g)
                worst = [R.close(t["fit"], fit, "fit"), R.close(t["cal"], cal, "cal"), R.close(t["rank"], rk, "rank")]
                print(f"draws={draws} {m} set {k}: worst error / bound (fit, cal, rank)", worst, "median rho",
                      float(np.median(fit[:, 0])), "msll", float(np.nanmedian(fit[:, 4])) if k < 2 else None)
                assert max(worst) <= 1.0, (m, k)
                assert np.all(fit[:, 6] == (g == 0).sum()) and np.all(fit[:, 7] == (0 if k < 2 else 4))
                assert np.isnan(t["fit"][:, 4]).all() == (k == 2) and np.isfinite(t["cal"]).all() and np.isfinite(t["rank"][:, :3]).all()
                if k < 2:
                    rd = pd.read_csv(dirs[a][k] / m / f"fit_quality_{m}.csv", float_precision="round_trip")
                    assert list(rd.columns) == ["ROI"] + io.fit_csv_columns(rank=True) and list(rd["ROI"]) == [f"{m}_{j}" for j in range(D)]
                    assert _same(rd.iloc[:, 1:].to_numpy(dtype=np.float64), np.concatenate([t["fit"], t["cal"], t["rank"]], axis=1))
            assert all(r["fit_pooled"][m] is res[0]["fit_pooled"][m] for r in res)
        # without fit_rank: no rank table, eight columns fewer, the other sixteen unchanged
        plain = sweep.test_folds(jobs, cohort, folds, mods, "gpoe", DEV, roi_effect=True, fit=True, draws=draws)
        for m in mods:
            assert plain[0]["fit"][m]["rank"] is None
            assert all(plain[0]["fit"][m][n].tobytes() == res[0]["fit"][m][n].tobytes() for n in ("fit", "cal"))
    for bad in (dict(fit=True), dict(roi_effect=True, fit_rank=True), dict(roi_effect=True, fit=True, z_thr=0.0)):
        with pytest.raises(ValueError):
            sweep.test_folds(jobs, cohort, folds, mods, "gpoe", DEV, **bad)


def test_command_line_with_and_without_the_flags(capsys):
    """`sweep test --roi-effect` writes exactly the files it wrote before unless the new flags are given; with them
    fit_quality_<m>.csv per fold and pooled, and `analysis --fit` reproduces the fold means in fp64."""
    import pandas as pd
    with tempfile.TemporaryDirectory() as d:
        a, b = Path(d) / "a", Path(d) / "b"
        sweep.main(["-P", "SE-gPoE", "-E", "2", "-K", "2", "-H", "32", "24", "8", "--subjects", "300", "--out-dir", str(a),
                    "--save-models", "--no-csv"])
        shutil.copytree(a, b)
        common = ["-P", "SE-gPoE", "-K", "2", "-H", "32", "24", "8", "--subjects", "300", "--roi-effect"]
        ea = sweep.main_test(common + ["--models-dir", str(a)])
        capsys.readouterr()
        eb = sweep.main_test(common + ["--models-dir", str(b), "--fit", "--fit-rank"])
        printed = capsys.readouterr().out
        assert all(np.array_equal(ea[m], eb[m]) for m in ea)
        fa, fb = _files(a), _files(b)
        base = Path("HCPimage") / "SE-gPoE"
        mods = list(prep.HCP_MODALITIES)
        want = [base / f"{k:03d}" / m / f"fit_quality_{m}.csv" for k in (0, 1) for m in mods] + [base / m / f"fit_quality_{m}.csv" for m in mods]
        assert sorted(set(fb) - set(fa)) == sorted(want) and set(fa) <= set(fb)
        assert not any("fit_quality" in p.name for p in fa)
        for p in fa:
            if p.suffix == ".csv":
                assert filecmp.cmp(a / p, b / p, shallow=False), p
        for m in mods:
            line = [ln for ln in printed.splitlines() if f" {m}: pooled model fit on the controls" in ln]
            assert len(line) == 1 and all(f"{k} " in line[0] for k in sweep.FIT_SUMMARY)
            pooled = pd.read_csv(b / base / m / f"fit_quality_{m}.csv")
            assert list(pooled.columns) == ["ROI"] + io.fit_csv_columns(rank=True)
            assert np.all(pooled["status"] == 4) and pooled["msll"].isna().all() and pooled["rho"].notna().all()
            fold0 = pd.read_csv(b / base / "000" / m / f"fit_quality_{m}.csv")
            assert np.all(fold0["status"] == 0) and fold0["msll"].notna().all() and np.all(fold0["n_obs"] == fold0["n_var"])
        before = _files(b)
        out = sweep.main_analysis(["-P", "SE-gPoE", "-K", "2", "--models-dir", str(b), "--fit"])
        text = capsys.readouterr().out
        assert text.count("model fit on the controls, median over ROIs of the fold means") == 1
        assert sorted(set(_files(b)) - set(before)) == sorted(base / f"group_analysis_fit_{m}.csv" for m in mods)
        for m in mods:
            folds = [pd.read_csv(b / base / f"{k:03d}" / m / f"fit_quality_{m}.csv", float_precision="round_trip") for k in (0, 1)]
            tab = np.stack([f[list(sweep.FIT_ANALYSIS)].to_numpy(dtype=np.float64) for f in folds])
            got = pd.read_csv(b / base / f"group_analysis_fit_{m}.csv", float_precision="round_trip")
            assert list(got.columns) == ["ROI"] + [f"{k}_{s}" for k in sweep.FIT_ANALYSIS for s in ("mean", "sd")]
            assert list(got["ROI"]) == list(folds[0]["ROI"]) and _same(out[m], tab)
            for j, k in enumerate(sweep.FIT_ANALYSIS):
                assert _same(got[f"{k}_mean"].to_numpy(), tab[:, :, j].mean(0)) and _same(got[f"{k}_sd"].to_numpy(), tab[:, :, j].std(0))
                assert f"{k} {float(np.nanmedian(tab[:, :, j].mean(0))):.4f}" in text
        with pytest.raises(SystemExit):
            sweep.main_analysis(["-P", "SE-gPoE", "-K", "2", "--models-dir", str(b), "--fit", "--roi"])
