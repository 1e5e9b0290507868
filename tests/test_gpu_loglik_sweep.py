"""The likelihood pass through the sweep: sweep.test_folds(loglik=S) -- all folds of a table height in one forward_loglik launch
-- with loglik_<P>.csv recomputed from the general kernel's exports by the fp64 restatement (tests/loglik_ref.py); the rerun
byte-identical; the files without the flag untouched; `test --loglik S` and `analysis --loglik-score` on the command line, the
analysis rows equal to metrics.posthoc_metrics on the file's own column and the model-selection table written."""
import filecmp
import tempfile
from pathlib import Path

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import multi_modal_normative_modeling_amd as nm
from multi_modal_normative_modeling_amd import engine, io, metrics, prep, sweep
from tests import loglik_ref as LR
from tests.table_stats_util import trained_cohort

DEV = "cuda:0"
FIVE = ("normalized", "reconstruction", "reconstruction_error", "reconstruction_error_roi", "deviation_as_feature_importance")
COLS = list(metrics.LOGLIK_ROW_COLUMNS)


@pytest.fixture(scope="module")
def trained():
    return trained_cohort(n=120, K=2, device=DEV)


def _files(root):
    return sorted(p.relative_to(root) for p in Path(root).rglob("*") if p.is_file())


def test_loglik_csv_is_the_restatement_of_the_general_kernels_exports(trained):
    import pandas as pd
    cohort, folds, mods, jobs = trained
    K, S, name = len(folds), 4, "SE-gPoE"
    with tempfile.TemporaryDirectory() as da, tempfile.TemporaryDirectory() as db, tempfile.TemporaryDirectory() as dc:
        dirs = lambda d: [Path(d) / f"{k:03d}" for k in range(K)]
        many = sweep.test_folds(jobs, cohort, folds, mods, "gpoe", DEV, out_dirs=dirs(da), loglik=S, loglik_name=name)
        again = sweep.test_folds(jobs, cohort, folds, mods, "gpoe", DEV, out_dirs=dirs(db), loglik=S, loglik_name=name)
        plain = sweep.test_folds(jobs, cohort, folds, mods, "gpoe", DEV, out_dirs=dirs(dc), loglik_name=name)
        fa, fb, fc = _files(da), _files(db), _files(dc)
        # the rerun: the same files, the same bytes; without the flag: the five kinds and no others, the same bytes
        assert fa == fb and sorted(set(fa) - set(fc)) == sorted(Path(f"{k:03d}") / f"loglik_{name}.csv" for k in range(K))
        assert fc == sorted(Path(f"{k:03d}") / m / f"{kind}_{m}.csv" for k in range(K) for m in mods for kind in FIVE)
        for p in fa:
            assert filecmp.cmp(Path(da) / p, Path(db) / p, shallow=False), p
        for p in fc:
            assert filecmp.cmp(Path(da) / p, Path(dc) / p, shallow=False), p
        for k, (tr, te) in enumerate(folds):
            assert "loglik" not in plain[k]
            n = len(te)
            df = pd.read_csv(Path(da) / f"{k:03d}" / f"loglik_{name}.csv", float_precision="round_trip")
            assert list(df.columns) == io.META_COLS + COLS + [f"recon_ll_{m}" for m in mods] and len(df) == n
            assert np.array_equal(df["participant_id"].to_numpy(), cohort.iid[te])
            assert np.array_equal(df[COLS].to_numpy(dtype=np.float32), many[k]["loglik"]["row"])
            # draw s of the evaluation job is the general kernel's draw under key s of the job's own seed
            ev, xs = sweep._fold_eval_job(jobs[k], cohort, tr, te, mods, "gpoe", DEV)
            seeds = engine.draw_seeds(ev.seed, S)
            ev.set_latent_exports(True)
            locs, zs = [], []
            for s in range(S):
                ev.seed = seeds[s]
                ev.touch()
                nm.JobSet([ev]).forward(loss=False)
                torch.cuda.synchronize()
                locs.append([t[:n].cpu().numpy() for t in ev.out_loc])
                zs.append(ev.out_z[:n].cpu().numpy())
            mu, lv = ev.out_mu[:n].cpu().numpy().astype(np.float64), ev.out_logvar[:n].cpu().numpy().astype(np.float64)
            z = np.stack(zs).astype(np.float64)
            eps = (z - mu[None]) * np.exp(-0.5 * lv)[None]
            lvo = [ev.layout.get(ev.params, f"{dp}logvar_out").reshape(-1).cpu().numpy() for _, _, dp in ev.kmods]
            val, bnd = LR.loglik(xs, [np.stack([locs[s][i] for s in range(S)]) for i in range(len(mods))], mu, lv, eps, z, lvo)
            worst = {c: LR.worst_ratio(df[c].to_numpy(), val[c], bnd[c]) for c in COLS}
            worst.update({f"recon_ll_{m}": LR.worst_ratio(df[f"recon_ll_{m}"].to_numpy(), val[f"recon_ll_{i}"], bnd[f"recon_ll_{i}"])
                          for i, m in enumerate(mods)})
            print(f"fold {k}: worst |file - restatement| / bound:", {c: f"{v:.3e}" for c, v in worst.items()})
            assert all(v <= 1.0 for v in worst.values()), worst
            assert (df["ess"] >= 1).all() and (df["ess"] <= S).all()
    # another key gives another table, the same key the same one
    other = sweep.test_folds(jobs, cohort, folds, mods, "gpoe", DEV, loglik=S, loglik_seed=77)
    same = sweep.test_folds(jobs, cohort, folds, mods, "gpoe", DEV, loglik=S, loglik_seed=77)
    for k in range(K):
        assert not np.array_equal(other[k]["loglik"]["row"], many[k]["loglik"]["row"])
        assert np.array_equal(other[k]["loglik"]["row"], same[k]["loglik"]["row"])
        assert np.array_equal(other[k]["loglik"]["row"][:, 4], many[k]["loglik"]["row"][:, 4])     # the analytic KL sees no draw


P, COMMON = "SE-gPoE", ["-K", "2", "-H", "32", "24", "8"]
BASE = Path("HCPimage") / P


@pytest.fixture(scope="module")
def cli():
    """Two folds trained and tested on the command line WITHOUT the flags: (root, the files that wrote, their bytes)."""
    with tempfile.TemporaryDirectory() as d:
        d = Path(d)
        sweep.main(["-P", P, "-E", "2", "--subjects", "300", "--out-dir", str(d), "--save-models", "--no-csv"] + COMMON)
        sweep.main_test(["-P", P, "--subjects", "300", "--models-dir", str(d)] + COMMON)
        before = _files(d)
        yield d, before, {p: (d / p).read_bytes() for p in before}


def test_command_line_loglik_and_its_group_analysis(cli, capsys):
    import pandas as pd
    d, before, stamp = cli
    sweep.main_test(["-P", P, "--subjects", "300", "--models-dir", str(d), "--loglik", "8", "--loglik-seed", "9"] + COMMON)
    printed = capsys.readouterr().out
    assert all(f"fold {k}:" in printed for k in (0, 1)) and "mean elbo" in printed and "median ess" in printed
    new = sorted(set(_files(d)) - set(before))
    assert new == sorted([BASE / f"{k:03d}" / f"loglik_{P}.csv" for k in (0, 1)] + [BASE / f"loglik_{P}.csv"])
    assert all((d / p).read_bytes() == stamp[p] for p in before)       # what `test` wrote without the flag: unchanged
    first = {p: (d / p).read_bytes() for p in new}
    sweep.main_test(["-P", P, "--subjects", "300", "--models-dir", str(d), "--loglik", "8", "--loglik-seed", "9"] + COMMON)
    assert all((d / p).read_bytes() == first[p] for p in new)          # the rerun: byte for byte
    pooled = pd.read_csv(d / BASE / f"loglik_{P}.csv")
    assert len(pooled) == 300 and list(pooled.columns)[:12] == io.META_COLS + COLS
    assert np.isfinite(pooled[COLS].to_numpy()).all() and ((pooled["ess"] >= 1) & (pooled["ess"] <= 8)).all()
    listed = _files(d)
    hc = prep.HC_LABEL.get("HCPimage", 1)
    for kind, column in (("logpx", "log_px"), ("elbo", "elbo")):
        table = sweep.main_analysis(["-P", P, "--models-dir", str(d), "--loglik-score", kind] + COMMON)
        scores, positive, ctl = [], [], []
        for k in (0, 1):
            df = pd.read_csv(d / BASE / f"{k:03d}" / f"loglik_{P}.csv")
            scores.append(torch.as_tensor(-df[column].to_numpy(dtype=np.float64), dtype=torch.float32))
            positive.append(torch.as_tensor(~sweep.healthy(df["DIA"].to_numpy(), hc), dtype=torch.int32))
            ctl.append(df[sweep.healthy(df["DIA"].to_numpy(), hc)][["elbo", "log_px"]].to_numpy(dtype=np.float64).mean(axis=0))
        assert torch.equal(table, metrics.posthoc_metrics(scores, positive).cpu()), kind
        sel = pd.read_csv(d / BASE / "group_analysis_loglik.csv", float_precision="round_trip")
        ctl = np.array(ctl)
        np.testing.assert_allclose(sel[["elbo_mean", "elbo_sd", "log_px_mean", "log_px_sd"]].to_numpy()[0],
                                   [ctl[:, 0].mean(), ctl[:, 0].std(), ctl[:, 1].mean(), ctl[:, 1].std()], rtol=1e-12)
    made = sorted(set(_files(d)) - set(listed))
    assert made == sorted(BASE / f"group_analysis_loglik{t}.csv" for t in ("", "_logpx", "_elbo"))
    # ... through the bootstrap and the threshold rules as any other score
    sweep.main_analysis(["-P", P, "--models-dir", str(d), "--loglik-score", "logpx", "--bootstrap", "100",
                         "--threshold-rule", "f1max"] + COMMON)
    more = sorted(set(_files(d)) - set(listed) - set(made))
    assert more == sorted(BASE / f"group_analysis_loglik_logpx_{tail}.csv" for tail in ("bootstrap", "operating_f1max", "curve"))
