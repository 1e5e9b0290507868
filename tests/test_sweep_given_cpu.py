"""The --given flags of the sweep's `test` and `analysis` commands and sweep.given_subsets behind them: what the keywords
expand to, what is refused and with which words -- before any device or model file is touched (there is no GPU here)."""
import numpy as np
import pytest

from multi_modal_normative_modeling_amd import io, prep, sweep, workload

MODS3 = ["T1w", "T2w", "fMRI"]


def test_keywords_expand_in_the_procedures_order():
    assert sweep.given_subsets("single", MODS3) == [("T1w", (0,)), ("T2w", (1,)), ("fMRI", (2,))]
    assert sweep.given_subsets("loo", MODS3) == [("T2w+fMRI", (1, 2)), ("T1w+fMRI", (0, 2)), ("T1w+T2w", (0, 1))]
    every = sweep.given_subsets("all", MODS3)
    assert len(every) == 7 and len({idx for _, idx in every}) == 7 and every[-1] == ("T1w+T2w+fMRI", (0, 1, 2))
    assert len(sweep.given_subsets("all", MODS3 + ["FDG"])) == 15
    # names in any order name the same set, its tag in the procedure's order; a set asked twice is listed once
    assert sweep.given_subsets(["fMRI+T1w"], MODS3) == [("T1w+fMRI", (0, 2))]
    assert sweep.given_subsets([("fMRI", "T1w"), "T1w+fMRI", "loo"], MODS3) == [("T1w+fMRI", (0, 2)), ("T2w+fMRI", (1, 2)), ("T1w+T2w", (0, 1))]
    assert sweep.given_subsets(["loo", "single"], ["a", "b"]) == [("b", (1,)), ("a", (0,))]
    assert io.given_filename("T1w", "T2w+fMRI") == "reconstruction_error_T1w_given_T2w+fMRI.csv"


def test_what_given_subsets_refuses():
    with pytest.raises(ValueError, match="several"):
        sweep.given_subsets("loo", ["T1w"])
    with pytest.raises(ValueError, match="PET"):
        sweep.given_subsets("T1w+PET", MODS3)
    with pytest.raises(ValueError, match="modalities are"):
        sweep.given_subsets([""], MODS3)


def test_test_folds_refuses_given_for_one_modality_before_anything_runs():
    with pytest.raises(ValueError, match="several"):
        sweep.test_folds([], prep.synthetic_cohort(n=20, d=8), [], ["T1w"], "poe", "cuda:0", given="single")


def _exits(call, argv, capsys, *words):
    with pytest.raises(SystemExit) as e:
        call(argv)
    assert e.value.code == 2
    err = capsys.readouterr().err
    for w in words:
        assert w in err, (w, err)


def test_test_command_parses_given_and_refuses_it_where_it_makes_no_sense(tmp_path, capsys):
    base = ["--models-dir", str(tmp_path)]
    _exits(sweep.main_test, ["-P", "SM-T1w", "--given", "loo"] + base, capsys, "--given", "several")
    _exits(sweep.main_test, ["-P", "SE-gPoE", "--given", "T1w+PET"] + base, capsys, "--given", "PET")
    _exits(sweep.main_test, ["-P", "SE-gPoE", "--given"] + base, capsys, "--given")


def test_analysis_given_names_what_to_run_first(tmp_path, capsys):
    base = ["--models-dir", str(tmp_path), "-K", "3"]
    mods = workload.procedure_modalities("SE-gPoE")[0]
    assert len(mods) >= 2
    _exits(sweep.main_analysis, ["-P", "SE-gPoE", "--given", "all"] + base, capsys, "`test` subcommand", "--given", "first",
           io.given_filename(mods[0], mods[0]))
    _exits(sweep.main_analysis, ["-P", f"SM-{mods[0]}", "--given", "single"] + base, capsys, "--given", "several")
    _exits(sweep.main_analysis, ["-P", "SE-gPoE", "--given", "loo", "--roi"] + base, capsys, "--given", "--roi")
    _exits(sweep.main_analysis, ["-P", "SE-gPoE", "--given", "loo", "--score", "latent"] + base, capsys, "--given", "--score")


def test_given_csv_has_the_layout_of_the_reconstruction_error_file(tmp_path):
    import pandas as pd
    n, d = 9, 5
    cohort = prep.synthetic_cohort(n=n, d=d)
    meta = sweep._meta_frame(cohort, np.arange(n))
    rng = np.random.default_rng(0)
    x, x_hat = rng.normal(size=(n, d)).astype(np.float32), rng.normal(size=(n, d)).astype(np.float32)
    plain = io.write_test_csvs(tmp_path, "T1w", meta, [f"r{i}" for i in range(d)], x, x_hat)["reconstruction_error"]
    given = io.write_given_csv(tmp_path, "T1w", "T1w+T2w", meta, x, x_hat)
    assert given.name == "reconstruction_error_T1w_given_T1w+T2w.csv"
    assert given.read_text() == plain.read_text()
    assert list(pd.read_csv(given).columns) == io.META_COLS + ["Reconstruction error"]
