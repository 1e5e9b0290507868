"""`test --draws S [--draw-seed N]` and `analysis --predictive-score msq | z2`: every refusal and its message, the file layouts
of io.write_predictive_csvs, and that the analysis names what to run first.  No device: nothing here launches a kernel."""
import numpy as np
import pandas as pd
import pytest

from multi_modal_normative_modeling_amd import _lib, io, prep, sweep, workload


def _exits(call, argv, capsys, *words):
    with pytest.raises(SystemExit) as e:
        call(argv)
    assert e.value.code == 2
    err = capsys.readouterr().err
    for w in words:
        assert w in err, (w, err)


def test_check_draws():
    assert sweep.check_draws(None) == (None, None)
    assert sweep.check_draws(1) == (1, None) and sweep.check_draws(64, 7) == (64, 7)
    assert sweep.check_draws(8, 2 ** 64 - 1) == (8, 2 ** 64 - 1)
    for bad in (0, -3, 65, 2.5):
        with pytest.raises(ValueError, match="1 to 64"):
            sweep.check_draws(bad)
    with pytest.raises(ValueError, match="needs draws"):
        sweep.check_draws(None, 3)
    for bad in (-1, 2 ** 64, 0.5):
        with pytest.raises(ValueError, match="draw_seed"):
            sweep.check_draws(4, bad)
    assert _lib.NM_MAX_DRAWS == 64


def test_test_folds_refuses_before_anything_runs():
    cohort = prep.synthetic_cohort(n=20, d=8)
    with pytest.raises(ValueError, match="1 to 64"):
        sweep.test_folds([], cohort, [], ["T1w"], "poe", "cuda:0", draws=65)
    with pytest.raises(ValueError, match="needs draws"):
        sweep.test_folds([], cohort, [], ["T1w"], "poe", "cuda:0", draw_seed=5)


def test_test_command_refusals(tmp_path, capsys):
    base = ["-P", "SE-gPoE", "--models-dir", str(tmp_path)]
    _exits(sweep.main_test, base + ["--draws", "0"], capsys, "--draws must be 1 to 64")
    _exits(sweep.main_test, base + ["--draws", "65"], capsys, "--draws must be 1 to 64")
    _exits(sweep.main_test, base + ["--draw-seed", "3"], capsys, "--draw-seed needs --draws")
    _exits(sweep.main_test, base + ["--draws", "4", "--draw-seed", "-1"], capsys, "--draw-seed must lie inside")
    _exits(sweep.main_test, base + ["--draws", "many"], capsys, "--draws")


def test_analysis_command_refusals(tmp_path, capsys):
    base = ["-P", "SE-gPoE", "--models-dir", str(tmp_path), "-K", "3"]
    _exits(sweep.main_analysis, base + ["--predictive-score", "var"], capsys, "--predictive-score")
    _exits(sweep.main_analysis, base + ["--predictive-score", "z2", "--score", "latent"], capsys, "--predictive-score", "--score")
    _exits(sweep.main_analysis, base + ["--predictive-score", "z2", "--centile-score", "tails"], capsys, "--predictive-score",
           "--centile-score")
    _exits(sweep.main_analysis, base + ["--predictive-score", "msq", "--roi"], capsys, "--predictive-score", "--roi")
    _exits(sweep.main_analysis, base + ["--predictive-score", "msq", "--given", "loo"], capsys, "--given", "--predictive-score")


@pytest.mark.parametrize("kind,fname", [("msq", "reconstruction_error_mc_"), ("z2", "predictive_subject_")])
def test_analysis_names_what_to_run_first(tmp_path, kind, fname):
    with pytest.raises(FileNotFoundError, match="--draws S") as e:
        sweep.main_analysis(["-P", "SE-gPoE", "--models-dir", str(tmp_path), "-K", "3", "--predictive-score", kind])
    assert fname in str(e.value) and "`test` subcommand" in str(e.value)


def test_the_score_choice_list_of_analysis_is_unchanged():
    """--predictive-score is a flag of its own: --score still refuses the predictive names."""
    with pytest.raises(SystemExit):
        sweep.main_analysis(["-P", "SE-gPoE", "--models-dir", ".", "--score", "predictive_msq"])
    assert sweep.PREDICTIVE_SCORES == ("msq", "z2")
    assert {f"predictive_{k}" for k in sweep.PREDICTIVE_SCORES} <= set(sweep.ANALYSIS_SCORES)


def test_predictive_csv_layouts(tmp_path):
    n, d = 9, 5
    rng = np.random.default_rng(0)
    cov = pd.DataFrame({"participant_id": np.arange(n), "DIA": rng.integers(1, 3, n), "AGE": rng.integers(20, 80, n),
                        "PTGENDER": rng.integers(0, 2, n), "extra": 1})
    cols = [f"roi{k}" for k in range(d)]
    x = rng.normal(size=(n, d)).astype(np.float32)
    x_hat = rng.normal(size=(n, d)).astype(np.float32)
    z = rng.normal(size=(n, d)).astype(np.float32)
    msq = (x - x_hat) ** 2
    paths = io.write_predictive_csvs(tmp_path / "m", "T1w", cov, cols, x_hat, msq, z)
    assert tuple(paths) == io.PREDICTIVE_KINDS
    assert all(p.name == f"{k}_T1w.csv" and p.exists() for k, p in paths.items())
    for kind in ("reconstruction_mc", "reconstruction_error_roi_mc", "predictive_z"):
        assert list(pd.read_csv(paths[kind]).columns) == io.META_COLS + cols
    # one draw: msq IS (x - x_hat)^2, and the per-subject file is the reconstruction_error_ file of write_test_csvs byte for byte
    ref = io.write_test_csvs(tmp_path / "m", "T1w", cov, cols, x, x_hat)
    assert paths["reconstruction_error_mc"].read_bytes() == ref["reconstruction_error"].read_bytes()
    assert paths["reconstruction_error_roi_mc"].read_bytes() == ref["reconstruction_error_roi"].read_bytes()
    sub = pd.read_csv(paths["predictive_subject"])
    assert list(sub.columns) == io.META_COLS + ["Mean squared error", "Mean z2", "Max abs z", "Max abs z ROI"]
    np.testing.assert_allclose(sub["Mean z2"], (z.astype(np.float64) ** 2).mean(axis=1), rtol=1e-6)
    np.testing.assert_allclose(sub["Max abs z"], np.abs(z).max(axis=1), rtol=1e-6)
    assert list(sub["Max abs z ROI"]) == [cols[i] for i in np.abs(z).argmax(axis=1)]
    assert len(workload.procedure_modalities("SE-gPoE")[0]) >= 2
