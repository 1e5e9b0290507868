"""`test --trajectory S [--traj-seed N]` and `analysis --trajectory-score zmean | extreme`: flag parsing and every refusal, the
27 x 2 covariate grid against prep.one_hot_covariates, the cell sort and its way back, the hand-built moments table, the
pooling of the per-cell column summaries, the CSV writers on synthetic arrays and the analysis wiring.  No device: nothing
here launches a kernel."""
import numpy as np
import pandas as pd
import pytest
import torch

from multi_modal_normative_modeling_amd import io, metrics, prep, sweep


def _exits(call, argv, capsys, *words):
    with pytest.raises(SystemExit) as e:
        call(argv)
    assert e.value.code == 2
    err = capsys.readouterr().err
    for w in words:
        assert w in err, (w, err)


def test_check_trajectory():
    assert sweep.check_trajectory(None) == (None, 0) and sweep.check_trajectory(None, 5) == (None, 0)
    assert sweep.check_trajectory(16) == (16, 0) and sweep.check_trajectory(4096, 7, 29) == (4096, 7)
    for bad in (0, 8, 15, 17, 100, 4097, 4112, 32.5, -16):
        with pytest.raises(ValueError, match="multiple of 16"):
            sweep.check_trajectory(bad)
    for bad in (-1, 0.5, 2 ** 62, None):
        with pytest.raises(ValueError, match="traj_seed"):
            sweep.check_trajectory(32, bad)
    for c_dim in (0, 3):
        with pytest.raises(ValueError, match="net_c_dim"):
            sweep.check_trajectory(32, 0, c_dim)


def test_test_folds_refuses_before_anything_runs():
    cohort = prep.synthetic_cohort(n=20, d=8)
    with pytest.raises(ValueError, match="multiple of 16"):
        sweep.test_folds([], cohort, [], ["T1w"], "poe", "cuda:0", trajectory=20)
    with pytest.raises(ValueError, match="traj_seed"):
        sweep.test_folds([], cohort, [], ["T1w"], "poe", "cuda:0", trajectory=32, traj_seed=-2)
    with pytest.raises(ValueError, match="z_thr"):
        sweep.test_folds([], cohort, [], ["T1w"], "poe", "cuda:0", trajectory=32, z_thr=0.0)


def test_test_command_refusals(tmp_path, capsys):
    base = ["-P", "SE-gPoE", "--models-dir", str(tmp_path)]
    for bad in ("0", "8", "40", "4112"):
        _exits(sweep.main_test, base + ["--trajectory", bad], capsys, "--trajectory must be a multiple of 16 from 16 to 4096")
    _exits(sweep.main_test, base + ["--traj-seed", "3"], capsys, "--traj-seed needs --trajectory")
    _exits(sweep.main_test, base + ["--trajectory", "32", "--traj-seed", "-1"], capsys, "--traj-seed must lie inside")
    _exits(sweep.main_test, base + ["--trajectory", "32", "--z-thr", "0"], capsys, "--z-thr")
    _exits(sweep.main_test, base + ["--trajectory", "many"], capsys, "--trajectory")


def test_grid_rows_are_the_one_hot_rows_of_subjects_in_the_cell():
    grid = sweep.trajectory_grid()
    assert grid.shape == (54, 29) and grid.dtype == np.float32
    assert (grid.sum(1) == 2).all() and len({tuple(r) for r in grid}) == 54
    for cell in range(54):
        assert grid[cell, cell // 2] == 1 and grid[cell, 27 + cell % 2] == 1
    rng = np.random.default_rng(3)
    for n in (54, 61, 300):
        age, gender = rng.uniform(20, 90, n).round(1), rng.integers(0, 2, n)
        cell, a, s = sweep.trajectory_cells(age, gender)
        assert np.array_equal(cell, a * 2 + s) and cell.min() >= 0 and cell.max() < 54
        assert np.array_equal(grid[cell], prep.one_hot_covariates(age, gender))       # every subject: its own cell's grid row
        frame = sweep.trajectory_cell_frame(age, cell, a)
        assert list(frame.columns) == io.TRAJECTORY_CHART_COLUMNS and len(frame) == 54
        assert int(frame["n_test"].sum()) == n and np.array_equal(frame["n_test"], np.bincount(cell, minlength=54))
        for b in range(27):
            lo, hi = frame["age_lo"][2 * b], frame["age_hi"][2 * b]
            assert (lo, hi) == (age[a == b].min(), age[a == b].max()) and frame["age_lo"][2 * b + 1] == lo
    few = sweep.trajectory_cell_frame(np.array([30.0, 40.0]), np.array([0, 53]), np.array([0, 26]))
    assert np.isnan(few["age_lo"][2]) and np.isnan(few["age_hi"][3]) and few["age_lo"][0] == 30 and few["age_hi"][53] == 40


def test_cell_sort_and_its_way_back():
    rng = np.random.default_rng(5)
    for n in (1, 7, 200):
        cell = rng.integers(0, 54, n)
        order, inverse, spans = sweep.cell_order(cell)
        assert np.array_equal(np.sort(order), np.arange(n)) and np.array_equal(order[inverse], np.arange(n))
        sc = cell[order]
        assert (np.diff(sc) >= 0).all()
        for c in np.unique(cell):                                       # stable: a cell's rows keep their order
            assert np.array_equal(order[sc == c], np.flatnonzero(cell == c))
        assert [c for c, _, _ in spans] == sorted(set(cell.tolist()))
        assert spans[0][1] == 0 and spans[-1][2] == n and all(a[2] == b[1] for a, b in zip(spans, spans[1:]))
        assert all((sc[a:b] == c).all() and b > a for c, a, b in spans)
        payload = rng.normal(size=(n, 3))
        assert np.array_equal(payload[order][inverse], payload)
    assert sweep.cell_order(np.zeros(0, dtype=np.int64))[2] == []


def test_chart_moments_is_a_moments_table_as_robust_moments_builds_one():
    mean = torch.tensor([[0.5, -1.0, 2.0], [0.0, 1.0, float("nan")]], dtype=torch.float64)
    sd = torch.tensor([[1.0, 0.0, 0.25], [2.0, float("inf"), 1.0]], dtype=torch.float64)
    mom = sweep.chart_moments(mean, sd, 48)
    assert tuple(mom.shape) == (2, 3, 8) and mom.dtype == torch.float64 and len(metrics.COHORT_MOMENTS_COLUMNS) == 8
    assert torch.equal(mom[..., 0].nan_to_num(9), mean.nan_to_num(9)) and torch.equal(mom[..., 1], sd)
    assert torch.equal(mom[..., 2], sd * sd) and (mom[..., 3] == 48).all()
    assert torch.isnan(mom[..., 4]).all() and torch.isnan(mom[..., 5]).all() and (mom[..., 6] == 0).all()
    assert mom[..., 7].tolist() == [[0.0, -2.0, 0.0], [0.0, -2.0, -2.0]]
    stats = torch.zeros(2, 3, 8, dtype=torch.float64)
    stats[..., 0], stats[..., 1], stats[..., 5] = mean.nan_to_num(0), 1.0, 48
    ref = metrics.robust_moments(stats, scale=1.0)                        # the same column order
    assert torch.equal(ref[..., 0], stats[..., 0]) and torch.equal(ref[..., 3], mom[..., 3])


def test_pool_cell_columns():
    cols = np.zeros((3, 2, 8))
    cols[:, :, :6] = np.arange(36).reshape(3, 2, 6)
    cols[:, :, 6], cols[:, :, 7] = [[1.0, 2.0], [3.0, 4.0], [5.0, 6.0]], np.nan
    cols[:, :, 5] = 0                                                    # no controls anywhere
    out = sweep.pool_cell_columns(cols)
    assert out.shape == (2, 8) and np.array_equal(out[:, :6], cols[:, :, :6].sum(0))
    n = cols[:, :, 4]
    np.testing.assert_allclose(out[:, 6], (cols[:, :, 6] * n).sum(0) / n.sum(0), rtol=1e-15)
    assert np.isnan(out[:, 7]).all()
    one = sweep.pool_cell_columns(cols[:1])
    assert np.array_equal(one[:, :7], cols[0, :, :7])


def test_trajectory_csv_layouts(tmp_path):
    n, d = 9, 5
    rng = np.random.default_rng(0)
    cov = pd.DataFrame({"participant_id": np.arange(n), "DIA": rng.integers(1, 3, n), "AGE": rng.integers(20, 80, n),
                        "PTGENDER": rng.integers(0, 2, n), "extra": 1})
    rois = [f"roi{k}" for k in range(d)]
    cell, a, _ = sweep.trajectory_cells(cov["AGE"].to_numpy(), cov["PTGENDER"].to_numpy())
    cells = sweep.trajectory_cell_frame(cov["AGE"].to_numpy(), cell, a)
    mean, sd = rng.normal(size=(54, d)), rng.uniform(0.5, 2, size=(54, d))
    paths = io.write_trajectory_chart_csvs(tmp_path / "m", "T1w", rois, cells, mean, sd)
    assert [p.name for p in paths.values()] == ["normative_trajectory_mean_T1w.csv", "normative_trajectory_sd_T1w.csv"]
    for k, tab in (("mean", mean), ("sd", sd)):
        df = pd.read_csv(paths[k], float_precision="round_trip")
        assert list(df.columns) == io.TRAJECTORY_CHART_COLUMNS + rois and len(df) == 54
        assert np.array_equal(df[rois].to_numpy(), tab) and np.array_equal(df["cell"], np.arange(54))
        assert np.array_equal(df["age_bin"], np.arange(54) // 2) and np.array_equal(df["gender_bin"], np.arange(54) % 2)
        assert int(df["n_test"].sum()) == n and df["age_lo"].isna().sum() == 2 * (27 - len(set(a.tolist())))
    with pytest.raises(ValueError):
        io.write_trajectory_chart_csvs(tmp_path / "m", "T1w", rois, cells, mean[:10], sd)
    z = rng.normal(size=(n, d)).astype(np.float32)
    rows, cols = rng.normal(size=(n, 8)), rng.normal(size=(d, 8))
    got = io.write_trajectory_csvs(tmp_path / "m", "T1w", cov, rois, z, rows, cols)
    ref = io.write_normative_csvs(tmp_path / "m", "T1w", cov, rois, z, rows, cols)
    assert [p.name for p in got.values()] == [f"trajectory_{k}_T1w.csv" for k in ("z", "subject", "map")]
    for k in ("z", "subject", "map"):                                   # the layouts of the normative_* counterparts, byte for byte
        assert got[k].read_bytes() == ref[k].read_bytes() and got[k] != ref[k]
    assert list(pd.read_csv(got["subject"]).columns) == io.META_COLS + list(metrics.NORMATIVE_ROW_COLUMNS)


def test_analysis_command_refusals(tmp_path, capsys):
    base = ["-P", "SE-gPoE", "--models-dir", str(tmp_path), "-K", "3"]
    _exits(sweep.main_analysis, base + ["--trajectory-score", "depth"], capsys, "--trajectory-score")
    _exits(sweep.main_analysis, base + ["--trajectory-score", "zmean", "--score", "latent"], capsys, "--trajectory-score", "--score")
    _exits(sweep.main_analysis, base + ["--trajectory-score", "zmean", "--centile-score", "tails"], capsys, "--trajectory-score",
           "--centile-score")
    _exits(sweep.main_analysis, base + ["--trajectory-score", "extreme", "--predictive-score", "z2"], capsys, "--trajectory-score")
    _exits(sweep.main_analysis, base + ["--trajectory-score", "extreme", "--roi"], capsys, "--trajectory-score", "--roi")
    _exits(sweep.main_analysis, base + ["--trajectory-score", "zmean", "--given", "loo"], capsys, "--given", "--trajectory-score")


@pytest.mark.parametrize("kind", ["zmean", "extreme"])
def test_analysis_names_what_to_run_first(tmp_path, kind):
    with pytest.raises(FileNotFoundError, match="--trajectory S") as e:
        sweep.main_analysis(["-P", "SE-gPoE", "--models-dir", str(tmp_path), "-K", "3", "--trajectory-score", kind])
    assert "trajectory_subject_" in str(e.value) and "`test` subcommand" in str(e.value)


def test_trajectory_score_wiring():
    """--trajectory-score is a flag of its own (two ANALYSIS_SCORES entries): --score still refuses the names."""
    with pytest.raises(SystemExit):
        sweep.main_analysis(["-P", "SE-gPoE", "--models-dir", ".", "--score", "trajectory_zmean"])
    assert sweep.TRAJECTORY_SCORES == ("zmean", "extreme")
    assert {f"trajectory_{k}" for k in sweep.TRAJECTORY_SCORES} <= set(sweep.ANALYSIS_SCORES)
    df = pd.DataFrame({"n_hi": [1.0, 2.0], "n_lo": [0.0, 3.0], "mean_abs_z": [0.5, 1.5]})
    pat, col, hint = sweep.ANALYSIS_SCORES["trajectory_zmean"]
    assert pat == "trajectory_subject_{m}.csv" and list(col(df)) == [0.5, 1.5] and "--trajectory S" in hint
    pat, col, hint = sweep.ANALYSIS_SCORES["trajectory_extreme"]
    assert pat == "trajectory_subject_{m}.csv" and list(col(df)) == [1.0, 5.0]
