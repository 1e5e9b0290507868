"""The command-line surface of the FI evaluation scores: `sweep regression --scores` / `--score-latent` / `--draws` /
`--draw-seed` reach the runner, their exclusions, and without `--scores` the runner is called with the arguments it always
had (a stub runner; no GPU)."""
from pathlib import Path

import pytest

from multi_modal_normative_modeling_amd import sweep

OLD = {"out_dir", "modalities", "combine", "lr", "hidden", "latent", "folds", "n_splits", "epochs"}


def _stub(calls):
    def runner(cohort, folds, n_splits, epochs, device, **kw):
        calls.append(dict(kw, folds=list(folds), n_splits=n_splits, epochs=epochs))
        return [{"fold": k, "RMSE": 0.5} for k in folds]
    return runner


@pytest.fixture
def calls(monkeypatch):
    monkeypatch.setattr(sweep, "_cohort_from_args", lambda args: object())
    monkeypatch.setattr(sweep, "_local_device", lambda: "cpu")
    monkeypatch.setattr(sweep, "_my_folds", lambda args: [0, 1])
    return []


def test_without_scores_the_runner_gets_the_old_arguments(calls):
    sweep.main_regression(["-K", "4", "-E", "1"], _runner=_stub(calls))
    assert set(calls[0]) == OLD
    assert calls[0]["out_dir"] is None and calls[0]["hidden"] == [110, 110] and calls[0]["latent"] == 10 and calls[0]["combine"] == "gpoe"
    sweep.main_regression(["-K", "4", "-E", "1", "--out-dir", "/tmp/nowhere_fi"], _runner=_stub(calls))
    assert set(calls[1]) == OLD and calls[1]["out_dir"] == Path("/tmp/nowhere_fi") / "HCPimage" / "regression_outputs"


def test_scores_flags_reach_the_runner(calls):
    sweep.main_regression(["-K", "4", "-E", "1", "--scores"], _runner=_stub(calls))
    assert set(calls[0]) == OLD | {"scores", "score_latent", "draws", "draw_seed"}
    assert calls[0]["scores"] is True and calls[0]["score_latent"] == "draw" and calls[0]["draws"] == 1 and calls[0]["draw_seed"] == 0
    sweep.main_regression(["-K", "4", "-E", "1", "--scores", "--draws", "32", "--draw-seed", "7", "--score-latent", "draw"],
                          _runner=_stub(calls))
    assert (calls[1]["score_latent"], calls[1]["draws"], calls[1]["draw_seed"]) == ("draw", 32, 7)
    sweep.main_regression(["-K", "4", "-E", "1", "--scores", "--score-latent", "mean"], _runner=_stub(calls))
    assert (calls[2]["score_latent"], calls[2]["draws"]) == ("mean", 1)


@pytest.mark.parametrize("argv", [["--score-latent", "draw"], ["--draws", "4"], ["--draw-seed", "3"],
                                  ["--scores", "--score-latent", "median"], ["--scores", "--draws", "0"],
                                  ["--scores", "--draws", "65"], ["--scores", "--score-latent", "mean", "--draws", "2"]])
def test_refused_flag_combinations(calls, argv):
    with pytest.raises(SystemExit):
        sweep.main_regression(argv, _runner=_stub(calls))
    assert not calls


def test_runner_signature_keeps_its_defaults():
    import inspect
    p = inspect.signature(sweep.run_regression_folds).parameters
    assert (p["scores"].default, p["score_latent"].default, p["draws"].default, p["draw_seed"].default) == (False, "draw", 1, 0)
