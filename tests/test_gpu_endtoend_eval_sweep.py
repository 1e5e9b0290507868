"""run_endtoend_folds(scores=True): the held-out folds of the end-to-end driver evaluated as one JobSet in one launch, the
per-subject CSVs, and `sweep analysis --endtoend-score` on them; pred_scores / predict_proba of the drop-in class."""
import tempfile
from pathlib import Path

import numpy as np
import pandas as pd
import pytest
import torch

pytestmark = pytest.mark.gpu

import multi_modal_normative_modeling_amd as nm
from multi_modal_normative_modeling_amd import metrics, prep, sweep

DEV = "cuda:0"


def _cohort():
    """The cohort of test_endtoend_sweep_small: a well separated disease group."""
    cohort = prep.synthetic_cohort(n=320, d=116)
    rng = np.random.default_rng(0)
    cohort.dia[:] = 1
    sick = rng.choice(320, size=120, replace=False)
    cohort.dia[sick] = 0
    for m in cohort.x:
        cohort.x[m][sick] += 1.5 * cohort.x[m].std(axis=0)
    return cohort


def test_scores_keep_the_metrics_and_write_the_tables():
    cohort = _cohort()
    kw = dict(latent=16, classifier_layers=(32, 16), dropout_rate=0.0, lr=1e-3)
    with tempfile.TemporaryDirectory() as d:
        old = sweep.run_endtoend_folds(cohort, [1, 4], 5, epochs=20, device=DEV, **kw)
        new = sweep.run_endtoend_folds(cohort, [1, 4], 5, epochs=20, device=DEV, scores=True, out_dir=Path(d) / "HCPimage" / "SE-PoE",
                                       procedure="SE-PoE", **kw)
        for a, b in zip(old, new):
            assert set(b) == set(a) | {"auroc_prob"}
            for k in a:
                if k != "steps_per_s":
                    assert a[k] == b[k], (k, a[k], b[k])
            assert 0.0 <= b["auroc_prob"] <= 1.0
        root = Path(d) / "HCPimage" / "SE-PoE"
        folds = prep.kfold_indices(len(cohort.iid), 5, 42)
        seen = []
        for k in (1, 4):
            df = pd.read_csv(root / f"{k:03d}" / "endtoend_SE-PoE.csv")
            assert list(df.columns[:4]) == ["participant_id", "DIA", "label", "fold"]
            assert list(df.columns[4:12]) == list(metrics.ENDTOEND_ROW_COLUMNS)
            assert list(df.columns[12:]) == ["logit_0", "logit_1"] + [f"dev_{b}_{m}" for b in ("health", "disease") for m in range(3)]
            assert len(df) == len(folds[k][1]) and (df["participant_id"].to_numpy() == cohort.iid[folds[k][1]]).all()
            assert (df["fold"] == k).all() and (df["label"] == (df["DIA"] != 1)).all() and (df["status"] == 0).all()
            assert ((df["p_disease"] >= 0) & (df["p_disease"] <= 1)).all()
            assert ((df["p_disease"] > 0.5) == (df["pred"] == 1)).all() or (df["margin"] == 0).any()
            seen.extend(df["participant_id"].tolist())
        assert len(seen) == len(set(seen))                         # each subject in exactly one fold
        pooled = pd.read_csv(root / "endtoend_SE-PoE.csv")
        assert pooled["participant_id"].tolist() == seen
        base = ["-P", "SE-PoE", "-K", "5", "--models-dir", d]
        t = sweep.main_analysis(base + ["--endtoend-score", "prob", "--bootstrap", "200"])
        assert t.shape[0] == 2 and (root / "group_analysis_endtoend_prob.csv").exists() and (root / "group_analysis_endtoend_prob_bootstrap.csv").exists()
        auc = pd.read_csv(root / "group_analysis_endtoend_prob.csv")["roc_auc"].to_numpy()
        np.testing.assert_allclose(auc, [r["auroc_prob"] for r in new], rtol=0, atol=1e-12)
        sweep.main_analysis(base + ["--endtoend-score", "contrast", "--threshold-rule", "f1max"])
        assert (root / "group_analysis_endtoend_contrast.csv").exists() and (root / "group_analysis_endtoend_contrast_operating_f1max.csv").exists()
        sweep.main_analysis(base + ["--endtoend-score", "margin"])
        assert (root / "group_analysis_endtoend_margin.csv").exists()


def _same_scores(a, b):
    """Two evaluations of the same rows: everything that comes from the latent and the classifier bit for bit; the deviations
    to fp32 summation order where the two-launch route computed them (the general kernel adds a row's four column-group sums
    in arrival order: the bound tests/test_gpu_devpass_multi.py holds out_rowdev to), their difference to that of its terms."""
    for c in a.columns:
        x, y = a[c].to_numpy(), b[c].to_numpy()
        if c == "contrast":
            assert (np.abs(x - y) <= 2e-6 * (a["dev_health"].to_numpy() + a["dev_disease"].to_numpy()) + 1e-9).all(), c
        elif c.startswith("dev_"):
            np.testing.assert_allclose(x, y, rtol=2e-6, atol=1e-9, err_msg=c)
        else:
            assert np.array_equal(x, y), c


def test_pred_scores_and_predict_proba_agree_with_predict():
    torch.manual_seed(4)
    dims, B = [60, 45, 70], 200                       # (one batch: predict() runs its classifier launch over the first 256 rows)
    model = nm.cVAE_multimodal_endtoend(dims, [40, 32], 16, 5, modalities=3, non_linear=True, classifier_layers=[32, 16],
                                        dropout_rate=0.3, num_classes=2)
    model.to(DEV)
    g = torch.Generator().manual_seed(2)
    xes = [torch.randn(B, d, generator=g).to(DEV) for d in dims]
    cs = [torch.rand(B, 5, generator=g).to(DEV)] * 3
    model.train()
    model.forward(xes, cs)                            # (moves the running statistics off their initial values)
    model.eval()
    sd0 = {k: v.clone() for k, v in model.state_dict().items()}
    logits = model.predict(xes, cs)
    df = model.pred_scores(xes, cs)
    proba = model.predict_proba(xes, cs)
    assert list(df.columns[:8]) == list(metrics.ENDTOEND_ROW_COLUMNS) and len(df) == B
    assert list(df.columns[8:]) == ["logit_0", "logit_1"] + [f"dev_{b}_{m}" for b in ("health", "disease") for m in range(3)]
    assert np.array_equal(df[["logit_0", "logit_1"]].to_numpy(), logits.cpu().numpy())
    assert np.array_equal(df["pred"].to_numpy(), torch.argmax(logits, dim=1).cpu().numpy().astype(np.float32))
    assert proba.shape == (B, 2) and torch.equal(proba, torch.softmax(logits, dim=1))
    np.testing.assert_allclose(df["p_disease"].to_numpy(), proba[:, 1].cpu().numpy(), rtol=0, atol=5e-7)
    model.train()                                     # pred_scores is eval mode whatever the module's mode; nothing moves
    df2 = model.pred_scores(xes, cs)
    _same_scores(df2, df)
    draw = model.pred_scores(xes, cs, latent="draw", seed=11)
    assert np.array_equal(draw["logit_1"].to_numpy(), df["logit_1"].to_numpy()) and not np.array_equal(draw["dev_health"].to_numpy(), df["dev_health"].to_numpy())
    _same_scores(model.pred_scores(xes, cs, latent="draw", seed=11), draw)
    sd1 = model.state_dict()
    assert all(torch.equal(sd0[k], sd1[k]) for k in sd0)
