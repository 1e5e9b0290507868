"""The command-line surface of the end-to-end evaluation scores: `sweep endtoend --scores` / `--score-latent`, `sweep
analysis --endtoend-score`, their exclusions, and the CSV / directory layout between the two (a stub runner writes what the
real one does; no GPU)."""
from pathlib import Path

import numpy as np
import pandas as pd
import pytest

from multi_modal_normative_modeling_amd import metrics, sweep


def _stub(calls):
    def runner(cohort, folds, n_splits, epochs, device, **kw):
        calls.append(dict(kw, folds=list(folds), n_splits=n_splits, epochs=epochs))
        return [{"fold": k, "accuracy": 0.5} for k in folds]
    return runner


def test_endtoend_without_scores_calls_the_runner_with_the_old_arguments(monkeypatch):
    calls = []
    monkeypatch.setattr(sweep, "_cohort_from_args", lambda args: object())
    monkeypatch.setattr(sweep, "_local_device", lambda: "cpu")
    monkeypatch.setattr(sweep, "_my_folds", lambda args: [0, 1])
    sweep.main_endtoend(["-K", "4", "-E", "1"], _runner=_stub(calls))
    assert set(calls[0]) == {"modalities", "latent", "classifier_layers", "dropout_rate", "margin", "weightcontrastive", "lr",
                             "hc_label", "hidden", "folds", "n_splits", "epochs"}
    sweep.main_endtoend(["-K", "4", "-E", "1", "--scores", "--score-latent", "draw", "--out-dir", "/tmp/nowhere_e2e"], _runner=_stub(calls))
    assert calls[1]["scores"] is True and calls[1]["score_latent"] == "draw" and calls[1]["procedure"] == "SE-PoE"
    assert calls[1]["out_dir"] == Path("/tmp/nowhere_e2e") / "HCPimage" / "SE-PoE"
    sweep.main_endtoend(["-K", "4", "-E", "1", "--scores"], _runner=_stub(calls))
    assert calls[2]["score_latent"] == "mean" and calls[2]["out_dir"] is None
    with pytest.raises(SystemExit):
        sweep.main_endtoend(["--score-latent", "draw"], _runner=_stub(calls))
    with pytest.raises(SystemExit):
        sweep.main_endtoend(["--scores", "--score-latent", "median"], _runner=_stub(calls))


@pytest.mark.parametrize("extra", [["--score", "latent"], ["--centile-score", "tails"], ["--predictive-score", "msq"],
                                   ["--trajectory-score", "zmean"], ["--loglik-score", "elbo"], ["--roi"], ["--given", "all"],
                                   ["--fit"]])
def test_endtoend_score_is_exclusive(extra, tmp_path, capsys):
    with pytest.raises(SystemExit):
        sweep.main_analysis(["-P", "SE-PoE", "--models-dir", str(tmp_path), "--endtoend-score", "prob"] + extra)
    err = capsys.readouterr().err
    assert "does not go with" in err or "--fit reads the fit tables alone" in err


def test_endtoend_score_error_wording(tmp_path, capsys):
    with pytest.raises(SystemExit):
        sweep.main_analysis(["-P", "SE-PoE", "--models-dir", str(tmp_path), "--endtoend-score", "prob", "--score", "latent"])
    assert "--endtoend-score is a score of its own: it does not go with --score" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        sweep.main_analysis(["-P", "SE-PoE", "--models-dir", str(tmp_path), "--endtoend-score", "prob", "--roi"])
    assert "--endtoend-score is a per-subject score: it does not go with --roi" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        sweep.main_analysis(["-P", "SE-PoE", "--models-dir", str(tmp_path), "--endtoend-score", "odds"])


def test_layout_is_what_the_analysis_reads(tmp_path):
    """Files laid out as run_endtoend_folds(scores=True, out_dir=<models-dir>/<resource>/<procedure>) writes them: _analysis_scores
    finds every fold, takes the three scores from their columns with the sign 'larger = more patient-like', and the patient
    flags from DIA."""
    root = tmp_path / "HCPimage" / "SE-PoE"
    rng = np.random.default_rng(0)
    frames = {}
    for k in (0, 2):
        n = 9 + k
        row = rng.normal(size=(n, 8)).astype(np.float32)
        df = pd.DataFrame({name: row[:, i] for i, name in enumerate(metrics.ENDTOEND_ROW_COLUMNS)})
        df["logit_0"], df["logit_1"] = 0.0, 1.0
        dia = rng.integers(0, 2, size=n)
        df.insert(0, "fold", k)
        df.insert(0, "label", (dia != 1).astype(int))
        df.insert(0, "DIA", dia)
        df.insert(0, "participant_id", np.arange(100 * k, 100 * k + n))
        (root / f"{k:03d}").mkdir(parents=True)
        df.to_csv(root / f"{k:03d}" / "endtoend_SE-PoE.csv", index=False)
        frames[k] = df
    assert set(sweep.ENDTOEND_SCORES) == {"prob", "margin", "contrast"}
    for kind, col in (("prob", "p_disease"), ("margin", "margin"), ("contrast", "contrast")):
        assert f"endtoend_{kind}" in sweep.ANALYSIS_SCORES
        scores, positive, folds, ids = sweep._analysis_scores(root, ["T1w"], "SE-PoE", f"endtoend_{kind}", 4, 1)
        assert folds == [0, 2]
        for s, p, i, k in zip(scores, positive, ids, folds):
            assert np.array_equal(s.numpy(), frames[k][col].to_numpy(dtype=np.float32))
            assert np.array_equal(p.numpy(), frames[k]["label"].to_numpy()) and np.array_equal(i, frames[k]["participant_id"].to_numpy())
    with pytest.raises(FileNotFoundError, match="--scores"):
        sweep._analysis_scores(tmp_path, ["T1w"], "SE-PoE", "endtoend_prob", 4, 1)
