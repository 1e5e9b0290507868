"""The normative chart and the trajectory z-scores through the sweep: test_folds(..., trajectory=S) on the trained synthetic
cohort of tests/table_stats_util.py (two folds, two modalities of different widths), S = 32 prior rows -- the files and their
headers, 54 chart rows, trajectory_z against (x - mean[cell]) / sd_pred[cell] recomputed in numpy fp64 from the WRITTEN chart,
the row order, identical bytes on a rerun, the chart against the drop-in class's normative_trajectory arithmetic, the
untouched default -- and the command line down to `analysis --trajectory-score zmean`."""
import filecmp
import shutil
import tempfile
from pathlib import Path

import numpy as np
import pandas as pd
import pytest
import torch

from multi_modal_normative_modeling_amd import io, metrics, prep, sweep
from tests.table_stats_util import trained_cohort

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
S, THR = 32, 1.96


@pytest.fixture(scope="module")
def trained():
    return trained_cohort(120, 2, DEV)


@pytest.fixture(scope="module")
def run(trained):
    """test_folds with the chart on (directory a), again (b: the rerun) and without it (c); results and directories, shared."""
    cohort, folds, mods, jobs = trained
    d = tempfile.mkdtemp()
    dirs = {k: [Path(d) / k / f"{f:03d}" for f in range(2)] for k in "abc"}
    res = sweep.test_folds(jobs, cohort, folds, mods, "gpoe", DEV, out_dirs=dirs["a"], trajectory=S, traj_seed=3, z_thr=THR)
    again = sweep.test_folds(jobs, cohort, folds, mods, "gpoe", DEV, out_dirs=dirs["b"], trajectory=S, traj_seed=3, z_thr=THR)
    base = sweep.test_folds(jobs, cohort, folds, mods, "gpoe", DEV, out_dirs=dirs["c"])
    yield Path(d), dirs, res, again, base
    shutil.rmtree(d)


def _files(root):
    return sorted(p.relative_to(root) for p in Path(root).rglob("*") if p.is_file())


NEW = ("normative_trajectory_mean", "normative_trajectory_sd", "trajectory_z", "trajectory_subject", "trajectory_map")


def test_files_headers_and_the_untouched_default(trained, run):
    cohort, folds, mods, _ = trained
    root, dirs, res, again, base = run
    fa, fb, fc = _files(root / "a"), _files(root / "b"), _files(root / "c")
    assert fa == fb and all(filecmp.cmp(root / "a" / p, root / "b" / p, shallow=False) for p in fa)      # a rerun: identical bytes
    assert sorted(set(fa) - set(fc)) == sorted(Path(f"{k:03d}") / m / f"{w}_{m}.csv" for k in range(2) for m in mods for w in NEW)
    assert set(fc) <= set(fa) and all(filecmp.cmp(root / "a" / p, root / "c" / p, shallow=False) for p in fc)
    for r, r0 in zip(res, base):
        assert set(r) == set(r0) | {"trajectory"} and all(r[m].tobytes() == r0[m].tobytes() for m in mods)
    for k, (_, te) in enumerate(folds):
        for i, m in enumerate(mods):
            D = (40, 23)[i]
            rois = [f"{m}_{j}" for j in range(D)]
            for w in ("mean", "sd"):
                df = pd.read_csv(dirs["a"][k] / m / f"normative_trajectory_{w}_{m}.csv")
                assert list(df.columns) == io.TRAJECTORY_CHART_COLUMNS + rois and len(df) == 54
                assert list(df["cell"]) == list(range(54)) and int(df["n_test"].sum()) == len(te)
            zf = pd.read_csv(dirs["a"][k] / m / f"trajectory_z_{m}.csv")
            sf = pd.read_csv(dirs["a"][k] / m / f"trajectory_subject_{m}.csv")
            mf = pd.read_csv(dirs["a"][k] / m / f"trajectory_map_{m}.csv")
            assert list(zf.columns) == io.META_COLS + rois and len(zf) == len(te)
            assert list(sf.columns) == io.META_COLS + list(metrics.NORMATIVE_ROW_COLUMNS) and len(sf) == len(te)
            assert list(mf.columns) == ["ROI"] + list(metrics.NORMATIVE_COL_COLUMNS) and len(mf) == D
            assert list(zf["participant_id"]) == list(cohort.iid[te]) == list(sf["participant_id"])     # the test ids' order
            assert list(sf["DIA"]) == list(cohort.dia[te])


def test_trajectory_z_is_the_written_chart_applied_to_the_subject_s_own_cell(trained, run):
    cohort, folds, mods, _ = trained
    _, dirs, res, _, _ = run
    rt = dict(float_precision="round_trip")
    for k, (_, te) in enumerate(folds):
        cell, a_bin, _ = sweep.trajectory_cells(cohort.age[te], cohort.gender[te])
        g = sweep.roi_groups(cohort.dia[te])
        for i, m in enumerate(mods):
            mean = pd.read_csv(dirs["a"][k] / m / f"normative_trajectory_mean_{m}.csv", **rt)
            sd = pd.read_csv(dirs["a"][k] / m / f"normative_trajectory_sd_{m}.csv", **rt)
            assert np.array_equal(mean["n_test"], np.bincount(cell, minlength=54))
            for b in np.unique(a_bin):
                ages = cohort.age[te][a_bin == b]
                assert mean["age_lo"][2 * b] == ages.min() and mean["age_hi"][2 * b + 1] == ages.max()
            mu, sg = mean.iloc[:, 6:].to_numpy(np.float64), sd.iloc[:, 6:].to_numpy(np.float64)
            e = res[k]["trajectory"][m]
            assert np.array_equal(mu, e["mean"]) and np.array_equal(sg, e["sd_pred"]) and np.array_equal(e["cell"], cell)
            assert (e["sd_pred"] == np.sqrt(e["var_latent"] + e["noise_var"][None, :])).all() and (sg > 0).all()
            # (x and z are fp32 values written as their shortest decimal text: read back THROUGH fp32 they are the values that
            #  were scored and stored, exactly; read as fp64 the text is up to half an fp32 ulp off, which x - mean amplifies)
            x = pd.read_csv(dirs["a"][k] / m / f"normalized_{m}.csv", **rt).iloc[:, 4:].to_numpy(np.float32).astype(np.float64)
            z = pd.read_csv(dirs["a"][k] / m / f"trajectory_z_{m}.csv", **rt).iloc[:, 4:].to_numpy(np.float32).astype(np.float64)
            want = (x - mu[cell]) / sg[cell]
            # z travels as fp32 text: one rounding of the fp64 quotient (2^-24 relative; 2^-23 allows the last bit)
            err = np.abs(z - want) / np.abs(want)
            print(f"fold {k} {m}: max relative error {err.max():.3e} (bound {2.0 ** -23:.3e}), max |z| {np.abs(want).max():.3f}")
            assert err.max() <= 2.0 ** -23
            assert np.array_equal(z.astype(np.float32), e["z"])
            # the per-subject summary and the map follow from the z-scores
            rows = pd.read_csv(dirs["a"][k] / m / f"trajectory_subject_{m}.csv", **rt)
            assert not np.any(np.abs(np.abs(want) - THR) < 1e-5)
            assert np.array_equal(rows["n_hi"], (want > THR).sum(1)) and np.array_equal(rows["n_lo"], (want < -THR).sum(1))
            np.testing.assert_allclose(rows["mean_abs_z"], np.abs(want).mean(1), rtol=1e-6)
            cols = pd.read_csv(dirs["a"][k] / m / f"trajectory_map_{m}.csv", **rt)
            assert np.array_equal(cols["n_hi_x"], (want[g == 1] > THR).sum(0)) and np.array_equal(cols["n_lo_y"], (want[g == 0] < -THR).sum(0))
            assert np.all(cols["n_x"] == (g == 1).sum()) and np.all(cols["n_y"] == (g == 0).sum())
            np.testing.assert_allclose(cols["mean_z_x"], want[g == 1].mean(0), rtol=1e-5, atol=1e-6)


def test_chart_is_the_moments_of_the_decoded_prior_rows(trained, run):
    """The chart of fold k: S rows keyed traj_seed + k, decoded under the 54 cells by the fold's model, mean and ddof-1 variance
    over the rows per cell -- restated with a decode launch of its own and fp64 numpy."""
    import multi_modal_normative_modeling_amd as nm
    cohort, folds, mods, jobs = trained
    _, _, res, _, _ = run
    grid = torch.from_numpy(sweep.trajectory_grid())
    for k, job in enumerate(jobs):
        z = torch.randn(S, 8, generator=torch.Generator().manual_seed(3 + k))
        job.enable_decode_exports(S, 54)
        job.set_decode_inputs(z, c_grid=grid, x=None)
        nm.JobSet([job]).decode()
        torch.cuda.synchronize()
        for i, m in enumerate(mods):
            loc = job.dec_loc[i].cpu().numpy().astype(np.float64)
            e = res[k]["trajectory"][m]
            np.testing.assert_allclose(e["mean"], loc.mean(1), rtol=1e-12, atol=1e-12)
            np.testing.assert_allclose(e["var_latent"], loc.var(1, ddof=1), rtol=1e-9, atol=1e-15)
            assert not np.array_equal(e["mean"][0], e["mean"][1]) and not np.array_equal(e["mean"][0], e["mean"][2])
    assert not np.array_equal(res[0]["trajectory"][mods[0]]["mean"], res[1]["trajectory"][mods[0]]["mean"])


def test_command_line_with_and_without_the_flag():
    with tempfile.TemporaryDirectory() as d:
        a, b = Path(d) / "a", Path(d) / "b"
        sweep.main(["-P", "SE-gPoE", "-E", "2", "-K", "2", "-H", "32", "24", "8", "--subjects", "300", "--out-dir", str(a),
                    "--save-models", "--no-csv"])
        shutil.copytree(a, b)
        common = ["-P", "SE-gPoE", "-K", "2", "-H", "32", "24", "8", "--subjects", "300"]
        ea = sweep.main_test(common + ["--models-dir", str(a)])
        eb = sweep.main_test(common + ["--models-dir", str(b), "--trajectory", str(S), "--traj-seed", "5"])
        assert all(np.array_equal(ea[m], eb[m]) for m in ea)
        fa, fb = _files(a), _files(b)
        base = Path("HCPimage") / "SE-gPoE"
        mods = list(prep.HCP_MODALITIES)
        assert not any("trajectory" in p.name for p in fa)
        assert sorted(set(fb) - set(fa)) == sorted(base / f"{k:03d}" / m / f"{w}_{m}.csv" for k in (0, 1) for m in mods for w in NEW)
        for p in fa:
            if p.suffix == ".csv":                                       # without the flag: exactly the files from before
                assert filecmp.cmp(a / p, b / p, shallow=False), p
        before = _files(b)
        tab = sweep.main_analysis(["-P", "SE-gPoE", "-K", "2", "--models-dir", str(b), "--trajectory-score", "zmean"]).numpy()
        out = pd.read_csv(b / base / "group_analysis_trajectory_zmean.csv", float_precision="round_trip")
        assert list(out.columns) == ["fold"] + list(metrics.POSTHOC_COLUMNS) and list(out["fold"]) == [0, 1]
        assert sorted(set(_files(b)) - set(before)) == [base / "group_analysis_trajectory_zmean.csv"]
        from oracle import metrics_ref
        for k in (0, 1):
            dfs = [pd.read_csv(b / base / f"{k:03d}" / m / f"trajectory_subject_{m}.csv") for m in mods]
            s = sum(f["mean_abs_z"].to_numpy(dtype=np.float64) for f in dfs) / len(dfs)
            ref = metrics_ref.posthoc_metrics(s.astype(np.float32), (dfs[0]["DIA"].to_numpy() != 1).astype(int))
            assert np.isfinite(s).all() and abs(tab[k, 0] - ref[0]) <= 1e-13 and tab[k, 0] == out["roc_auc"][k], k
        with pytest.raises(SystemExit):
            sweep.main_test(common + ["--models-dir", str(a), "--trajectory", "40"])
