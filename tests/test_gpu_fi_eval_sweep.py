"""run_regression_folds(scores=True): the held-out folds of the regression driver evaluated as one JobSet in one launch, the
per-fold and pooled CSVs, pred_fi / predict_fi of the drop-in class on the same rows, both routes of forward_fi behind the
driver, and the files of a run without scores against the two-launch route."""
import tempfile
from pathlib import Path

import numpy as np
import pandas as pd
import pytest
import torch

pytestmark = pytest.mark.gpu

import multi_modal_normative_modeling_amd as nm
from multi_modal_normative_modeling_amd import metrics, prep, sweep, workload

DEV = "cuda:0"
FOLDS, K, EPOCHS, S, SEED = [0, 3], 5, 3, 4, 5


def _cohort():
    cohort = prep.synthetic_cohort(n=320, d=116)
    cohort.fi[:] = (cohort.fi - cohort.fi.mean()) / cohort.fi.std()
    return cohort


def _trained(cohort):
    """The driver's own training, call for call (run_regression_folds keeps no model): per fold the trained state, the scalers
    and the job's seed."""
    folds = prep.kfold_indices(len(cohort.iid), K, 42)
    cov = np.stack([cohort.age, cohort.gender], axis=1).astype(np.float32)
    jobs, scalers = [], []
    for k in FOLDS:
        tr = folds[k][0]
        sc = [prep.robust_scaler_fit(prep.source_table(cohort, m)[tr]) for m in prep.HCP_MODALITIES]
        xs = [prep.robust_scaler_transform(prep.source_table(cohort, m)[tr], *sc[i]).astype(np.float32) for i, m in enumerate(prep.HCP_MODALITIES)]
        tables = [nm.Table(x, cov[tr], DEV) for x in xs]
        spec = nm.ModelSpec([t.D for t in tables], list(workload.HIDDEN), int(workload.LATENT), 2, True, "regression")
        j = nm.Job(spec, tables, combine="gpoe", lr=1e-4, seed=1000 * k, init_seed=42 + k, loss_cap=8)
        j.reg_lambda = 1.0
        j.set_fi(cohort.fi[tr].astype(np.float32))
        jobs.append(j)
        scalers.append(sc)
    nm.JobSet(jobs).train_regression(EPOCHS * jobs[0].batches_per_epoch)
    torch.cuda.synchronize()
    out = {}
    for k, j, sc in zip(FOLDS, jobs, scalers):
        te = folds[k][1]
        xs = [prep.robust_scaler_transform(prep.source_table(cohort, m)[te], *sc[i]).astype(np.float32) for i, m in enumerate(prep.HCP_MODALITIES)]
        out[k] = (j.spec, j.state_dict(), xs, cov[te], j.seed, te)
    return out


def _without_column(path, name):
    """The file's bytes with one CSV column cut out."""
    lines = Path(path).read_bytes().split(b"\n")
    i = lines[0].split(b",").index(name.encode())
    return b"\n".join(b",".join(c for n, c in enumerate(l.split(b",")) if n != i) for l in lines)


def _frames(d):
    return {k: pd.read_csv(Path(d) / f"regression_fold_{k}.csv") for k in FOLDS}


def test_scores_write_the_tables_and_agree_with_the_drop_in_class(monkeypatch):
    cohort = _cohort()
    trained = _trained(cohort)
    monkeypatch.setenv("NMHIP_FI", "1")
    with tempfile.TemporaryDirectory() as d, tempfile.TemporaryDirectory() as d0:
        res = sweep.run_regression_folds(cohort, FOLDS, K, epochs=EPOCHS, device=DEV, out_dir=d, scores=True, draws=S, draw_seed=SEED)
        monkeypatch.setenv("NMHIP_FI", "0")
        res0 = sweep.run_regression_folds(cohort, FOLDS, K, epochs=EPOCHS, device=DEV, out_dir=d0, scores=True, draws=S, draw_seed=SEED)
        monkeypatch.setenv("NMHIP_FI", "1")            # (the drop-in class below: the pass, as the first run)
        a, b = _frames(d), _frames(d0)
        seen = []
        for k, r, r0 in zip(FOLDS, res, res0):
            df = a[k]
            te = trained[k][5]
            assert list(df.columns) == ["IID", "FI"] + list(metrics.FI_ROW_COLUMNS)
            assert len(df) == len(te) and (df["IID"].to_numpy() == cohort.iid[te]).all() and (df["status"] == 0).all()
            assert np.array_equal(df["FI"].to_numpy(dtype=np.float32), cohort.fi[te].astype(np.float32))
            assert (df["fi_sd"] > 0).all() and (df["fi_min"] <= df["fi_pred"]).all() and (df["fi_pred"] <= df["fi_max"]).all()
            pred = np.load(Path(d) / f"fold_{k}_pred.npy")
            assert pred.shape == (len(te), 1) and np.array_equal(pred[:, 0], df["fi_pred"].to_numpy(dtype=np.float32))
            ref = sweep.evaluate_regression(np.load(Path(d) / f"fold_{k}_true.npy"), pred)
            assert all(r[name] == ref[name] for name in ref)
            # the two routes of forward_fi behind the driver: the files' bytes wherever twin equality holds -- every file of the
            # directory but the score tables, and of those every column but dev (out_rowdev's summation order)
            assert _without_column(Path(d) / f"regression_fold_{k}.csv", "dev") == _without_column(Path(d0) / f"regression_fold_{k}.csv", "dev")
            for c in df.columns:
                if c == "dev":
                    np.testing.assert_allclose(df[c].to_numpy(), b[k][c].to_numpy(), rtol=2e-6, atol=1e-9)
                else:
                    assert np.array_equal(df[c].to_numpy(), b[k][c].to_numpy()), (k, c)
            assert all(r[name] == r0[name] for name in ("RMSE", "MAE", "R2", "MAPE", "pooled_RMSE"))
            # the drop-in class on the same rows, the same keys
            spec, state, xs, cov, _, _ = trained[k]
            model = nm.cVAE_multimodal_regression(spec.input_dims, list(spec.hidden), spec.latent, 2, modalities=3, non_linear=True)
            model.load_state_dict(state)
            model.to(DEV)
            got = model.pred_fi(xs, cov, DEV, "gpoe", latent="draw", n_draws=S, seed=SEED)
            assert list(got.columns) == list(metrics.FI_ROW_COLUMNS)
            for c in ("fi_pred", "fi_sd", "fi_min", "fi_max", "kl"):
                assert np.array_equal(got[c].to_numpy(), df[c].to_numpy(dtype=np.float32)), (k, c)
            one = model.predict_fi(xs, cov, DEV, "gpoe")
            assert one.shape == (len(te), 1) and torch.equal(one, model.predict_fi(xs, cov, DEV, "gpoe"))
            seen.extend(df["IID"].tolist())
        assert sorted(p.name for p in Path(d).iterdir()) == sorted(p.name for p in Path(d0).iterdir())
        for f in Path(d).iterdir():
            if f.name.startswith("regression_"):
                assert _without_column(f, "dev") == _without_column(Path(d0) / f.name, "dev"), f.name
            else:
                assert f.read_bytes() == (Path(d0) / f.name).read_bytes(), f.name
        pooled = pd.read_csv(Path(d) / "regression_pooled.csv")
        assert list(pooled.columns) == ["IID", "FI"] + list(metrics.FI_ROW_COLUMNS) and pooled["IID"].tolist() == seen
        ps = sweep.evaluate_regression(pooled["FI"].to_numpy(dtype=np.float32), pooled["fi_pred"].to_numpy(dtype=np.float32))
        assert res[0]["pooled_RMSE"] == ps["RMSE"] and res[1]["pooled_R2"] == ps["R2"]


def test_without_scores_the_files_are_those_of_the_two_launch_route():
    """A run without scores: every file of its directory, byte for byte, against files written here through
    forward_fi(compact=False) for the driver's evaluation job (its seed, its own draw, no latent exports), the targets and the
    driver's deviation pass on the trained state -- and no score file appears."""
    from multi_modal_normative_modeling_amd import io
    cohort = _cohort()
    trained = _trained(cohort)
    cov_all = np.stack([cohort.age, cohort.gender], axis=1).astype(np.float32)
    with tempfile.TemporaryDirectory() as d, tempfile.TemporaryDirectory() as d2:
        res = sweep.run_regression_folds(cohort, FOLDS, K, epochs=EPOCHS, device=DEV, out_dir=d)
        names = sorted(p.name for p in Path(d).iterdir())
        want = sorted([f"fold_{k}_{w}.npy" for k in FOLDS for w in ("pred", "true")] +
                      [f"deviation_fold_{k}_{m}_roiwise.csv" for k in FOLDS for m in prep.HCP_MODALITIES])
        assert names == want
        assert all(not key.startswith("pooled_") for r in res for key in r)
        for k in FOLDS:
            spec, state, xs, cov, seed, te = trained[k]
            tables = [nm.Table(x, cov, DEV) for x in xs]
            ev = nm.Job(spec, tables, combine="gpoe", state=state, seed=seed + 17, n_tiles_ws=tables[0].n_tiles)
            ev.enable_fi_exports(rows=False, draws=False, loc=True, sqerr=False, rowdev=False, latent=False)
            nm.JobSet([ev]).forward_fi(compact=False)
            torch.cuda.synchronize()
            pred = np.load(Path(d) / f"fold_{k}_pred.npy")
            assert np.array_equal(pred[:, 0], ev.out_fi_pred[: len(te)].cpu().numpy()), k
            np.save(Path(d2) / f"fold_{k}_pred.npy", ev.out_fi_pred[: len(te)].cpu().numpy().reshape(-1, 1))
            np.save(Path(d2) / f"fold_{k}_true.npy", cohort.fi[te].astype(np.float32).reshape(-1, 1))
            fit = nm.Job(spec, tables, combine="gpoe", state=state, seed=seed)      # (the trained job: its state, its seed)
            for i, m in enumerate(prep.HCP_MODALITIES):
                dev, _, iids = sweep.deviation_roiwise(fit, i, cohort, m, DEV, want_matrix=True, covariates=cov_all)
                io.write_roiwise_csv(d2, k, m, iids, dev)
        for name in want:
            assert (Path(d) / name).read_bytes() == (Path(d2) / name).read_bytes(), name
