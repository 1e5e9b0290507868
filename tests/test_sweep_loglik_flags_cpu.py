"""`test --loglik S [--loglik-seed N]` and `analysis --loglik-score logpx | elbo`: the flags parse, every refusal and its
message, the layout of io.write_loglik_csv, the model-selection table, and that the analysis names what to run first.  No
device: nothing here launches a kernel."""
import numpy as np
import pandas as pd
import pytest

from multi_modal_normative_modeling_amd import _lib, io, metrics, prep, sweep


def _exits(call, argv, capsys, *words):
    with pytest.raises(SystemExit) as e:
        call(argv)
    assert e.value.code == 2
    err = capsys.readouterr().err
    for w in words:
        assert w in err, (w, err)


def test_check_loglik():
    assert sweep.check_loglik(None) == (None, None)
    assert sweep.check_loglik(1) == (1, None) and sweep.check_loglik(1024, 7) == (1024, 7)
    assert sweep.check_loglik(8, 2 ** 64 - 1) == (8, 2 ** 64 - 1)
    for bad in (0, -3, 1025, 2.5):
        with pytest.raises(ValueError, match="1 to 1024"):
            sweep.check_loglik(bad)
    with pytest.raises(ValueError, match="needs loglik"):
        sweep.check_loglik(None, 3)
    for bad in (-1, 2 ** 64, 0.5):
        with pytest.raises(ValueError, match="loglik_seed"):
            sweep.check_loglik(4, bad)
    assert _lib.NM_MAX_IW_DRAWS == 1024


def test_test_folds_refuses_before_anything_runs():
    cohort = prep.synthetic_cohort(n=20, d=8)
    with pytest.raises(ValueError, match="1 to 1024"):
        sweep.test_folds([], cohort, [], ["T1w"], "poe", "cuda:0", loglik=1025)
    with pytest.raises(ValueError, match="needs loglik"):
        sweep.test_folds([], cohort, [], ["T1w"], "poe", "cuda:0", loglik_seed=5)


def test_test_command_refusals(tmp_path, capsys):
    base = ["-P", "SE-gPoE", "--models-dir", str(tmp_path)]
    _exits(sweep.main_test, base + ["--loglik", "0"], capsys, "--loglik must be 1 to 1024")
    _exits(sweep.main_test, base + ["--loglik", "1025"], capsys, "--loglik must be 1 to 1024")
    _exits(sweep.main_test, base + ["--loglik-seed", "3"], capsys, "--loglik-seed needs --loglik")
    _exits(sweep.main_test, base + ["--loglik", "4", "--loglik-seed", "-1"], capsys, "--loglik-seed must lie inside")
    _exits(sweep.main_test, base + ["--loglik", "many"], capsys, "--loglik")


def test_analysis_command_refusals(tmp_path, capsys):
    base = ["-P", "SE-gPoE", "--models-dir", str(tmp_path), "-K", "3"]
    _exits(sweep.main_analysis, base + ["--loglik-score", "ess"], capsys, "--loglik-score")
    _exits(sweep.main_analysis, base + ["--loglik-score", "elbo", "--score", "latent"], capsys, "--loglik-score", "--score")
    _exits(sweep.main_analysis, base + ["--loglik-score", "elbo", "--centile-score", "tails"], capsys, "--loglik-score",
           "--centile-score")
    _exits(sweep.main_analysis, base + ["--loglik-score", "logpx", "--predictive-score", "z2"], capsys, "--loglik-score",
           "--predictive-score")
    _exits(sweep.main_analysis, base + ["--loglik-score", "logpx", "--trajectory-score", "zmean"], capsys, "--loglik-score",
           "--trajectory-score")
    _exits(sweep.main_analysis, base + ["--loglik-score", "logpx", "--roi"], capsys, "--loglik-score", "--roi")
    _exits(sweep.main_analysis, base + ["--loglik-score", "logpx", "--given", "loo"], capsys, "--given", "--loglik-score")
    _exits(sweep.main_analysis, base + ["--loglik-score", "logpx", "--fit"], capsys, "--fit")


@pytest.mark.parametrize("kind", sweep.LOGLIK_SCORES)
def test_analysis_names_what_to_run_first(tmp_path, kind):
    with pytest.raises(FileNotFoundError, match="--loglik S") as e:
        sweep.main_analysis(["-P", "SE-gPoE", "--models-dir", str(tmp_path), "-K", "3", "--loglik-score", kind])
    assert "loglik_SE-gPoE.csv" in str(e.value) and "`test` subcommand" in str(e.value)


def test_the_score_choice_list_of_analysis_is_unchanged():
    """--loglik-score is a flag of its own (two ANALYSIS_SCORES entries): --score still refuses the names."""
    with pytest.raises(SystemExit):
        sweep.main_analysis(["-P", "SE-gPoE", "--models-dir", ".", "--score", "loglik_logpx"])
    assert sweep.LOGLIK_SCORES == ("logpx", "elbo")
    assert {f"loglik_{k}" for k in sweep.LOGLIK_SCORES} <= set(sweep.ANALYSIS_SCORES)
    d = pd.DataFrame({"log_px": [-3.0, -1.0], "elbo": [-4.0, -2.0]})
    pat, col, hint = sweep.ANALYSIS_SCORES["loglik_logpx"]
    assert pat == "loglik_{p}.csv" and list(col(d)) == [3.0, 1.0] and "--loglik" in hint      # improbable = deviant
    assert list(sweep.ANALYSIS_SCORES["loglik_elbo"][1](d)) == [4.0, 2.0]


def _frame(rng, n, shift=0.0):
    return pd.DataFrame({"participant_id": np.arange(n), "DIA": rng.integers(0, 2, n), "AGE": rng.integers(20, 80, n),
                         "PTGENDER": rng.integers(0, 2, n), "extra": 1}), rng.normal(size=(n, 8)).astype(np.float32) + shift


def test_loglik_csv_layout_and_the_model_selection_table(tmp_path):
    rng = np.random.default_rng(0)
    root = tmp_path / "SE-gPoE"
    want = []
    for k in range(3):
        cov, row = _frame(rng, 11 + k, shift=float(k))
        rec = {"T1w": row[:, 5] * 0.5, "T2w": row[:, 5] * 0.5}
        path = io.write_loglik_csv(root / f"{k:03d}", "SE-gPoE", cov, row, metrics.LOGLIK_ROW_COLUMNS, rec)
        assert path.name == "loglik_SE-gPoE.csv"
        df = pd.read_csv(path, float_precision="round_trip")
        assert list(df.columns) == io.META_COLS + list(metrics.LOGLIK_ROW_COLUMNS) + ["recon_ll_T1w", "recon_ll_T2w"]
        assert np.array_equal(df[list(metrics.LOGLIK_ROW_COLUMNS)].to_numpy(dtype=np.float32), row)
        ctl = cov["DIA"].to_numpy() == 1
        dec = row.astype(str).astype(np.float64)                       # (the decimal strings the file holds, as fp64)
        want.append([dec[ctl, 1].mean(), dec[ctl, 0].mean()])
    want = np.array(want)
    tab = sweep._analysis_loglik(root, "SE-gPoE", 5, 1)                # (folds 3 and 4 have no file: skipped)
    assert list(tab.columns) == ["procedure", "folds", "elbo_mean", "elbo_sd", "log_px_mean", "log_px_sd"]
    assert int(tab["folds"][0]) == 3
    np.testing.assert_allclose(tab[["elbo_mean", "elbo_sd", "log_px_mean", "log_px_sd"]].to_numpy()[0],
                               [want[:, 0].mean(), want[:, 0].std(), want[:, 1].mean(), want[:, 1].std()], rtol=1e-12)
    assert pd.read_csv(root / "group_analysis_loglik.csv").shape == (1, 6)
