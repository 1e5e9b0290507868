"""The modality-subset pass through the sweep: sweep.test_folds(given=...) -- all folds in one forward_subsets launch per
table height -- against the fold-by-fold form, file by file; the files without `given` untouched; `test --given all` and
`analysis --given all --bootstrap B` on the command line, the full set's rows equal to the plain group analysis."""
import filecmp
import tempfile
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from multi_modal_normative_modeling_amd import io, metrics, prep, sweep
from tests.table_stats_util import trained_cohort

DEV = "cuda:0"


@pytest.fixture(scope="module")
def trained():
    return trained_cohort(n=120, K=2, device=DEV)


def _files(root):
    return sorted(p.relative_to(root) for p in Path(root).rglob("*") if p.is_file())


def test_test_folds_given_equals_the_fold_by_fold_form_file_by_file(trained):
    cohort, folds, mods, jobs = trained
    K = len(folds)
    with tempfile.TemporaryDirectory() as da, tempfile.TemporaryDirectory() as db, tempfile.TemporaryDirectory() as dc:
        dirs = lambda d: [Path(d) / f"{k:03d}" for k in range(K)]
        many = sweep.test_folds(jobs, cohort, folds, mods, "gpoe", DEV, out_dirs=dirs(da), given="loo")
        one = [sweep.test_folds([jobs[k]], cohort, [folds[k]], mods, "gpoe", DEV, out_dirs=[dirs(db)[k]], given="loo")[0]
               for k in range(K)]
        plain = sweep.test_folds(jobs, cohort, folds, mods, "gpoe", DEV, out_dirs=dirs(dc))
        tags = [t for t, _ in sweep.given_subsets("loo", mods)]
        assert tags == [mods[1], mods[0]]
        fa, fb, fc = _files(da), _files(db), _files(dc)
        want = sorted(Path(f"{k:03d}") / m / io.given_filename(m, t) for k in range(K) for m in mods for t in tags)
        assert fa == fb and sorted(set(fa) - set(fc)) == want and set(fc) <= set(fa)
        for p in fa:
            assert filecmp.cmp(Path(da) / p, Path(db) / p, shallow=False), p
        for p in fc:                                                   # without `given`: every file as before
            assert filecmp.cmp(Path(da) / p, Path(dc) / p, shallow=False), p
        for k in range(K):
            assert "given" not in plain[k] and sorted(many[k]["given"]) == sorted(tags)
            for m in mods:
                assert np.array_equal(many[k][m], plain[k][m])
                for t in tags:
                    e = many[k]["given"][t][m]
                    assert np.array_equal(e, one[k]["given"][t][m]) and e.shape == (len(folds[k][1]),)
                    assert np.isfinite(e).all() and e.min() > 0 and not np.array_equal(e, many[k][m])
    # the full set through the subset pass is the plain pass: the same per-subject errors, bit for bit
    full = sweep.test_folds(jobs, cohort, folds, mods, "gpoe", DEV, given="+".join(mods))
    for k in range(K):
        for m in mods:
            got = full[k]["given"]["+".join(mods)][m]
            x_err = plain[k][m]
            # (out_rowdev sums a row in the kernel's order, this one on the host: the bound of tests/test_gpu_devpass_multi.py)
            assert np.allclose(got, x_err, rtol=2e-5, atol=1e-7)


def test_command_line_given_all_and_its_group_analysis(capsys):
    import pandas as pd
    P, common = "SE-gPoE", ["-K", "2", "-H", "32", "24", "8"]
    with tempfile.TemporaryDirectory() as d:
        d = Path(d)
        sweep.main(["-P", P, "-E", "2", "--subjects", "300", "--out-dir", str(d), "--save-models", "--no-csv"] + common)
        sweep.main_test(["-P", P, "--subjects", "300", "--models-dir", str(d)] + common)
        before = _files(d)
        stamp = {p: (d / p).read_bytes() for p in before}
        out = sweep.main_test(["-P", P, "--subjects", "300", "--models-dir", str(d), "--given", "all"] + common)
        mods = list(prep.HCP_MODALITIES)
        base = Path("HCPimage") / P
        tags = [t for t, _ in sweep.given_subsets("all", mods)]
        assert len(tags) == 7
        want = [base / f"{k:03d}" / m / io.given_filename(m, t) for k in (0, 1) for m in mods for t in tags]
        want += [base / m / io.given_filename(m, t) for m in mods for t in tags]
        assert sorted(set(_files(d)) - set(before)) == sorted(want)
        assert all((d / p).read_bytes() == stamp[p] for p in before)   # what `test` wrote without the flag: unchanged
        full = tags[-1]
        for k in (0, 1):
            for m in mods:
                a = (d / base / f"{k:03d}" / m / f"reconstruction_error_{m}.csv").read_text()
                assert a == (d / base / f"{k:03d}" / m / io.given_filename(m, full)).read_text(), (k, m)
        assert len(pd.read_csv(d / base / mods[0] / io.given_filename(mods[0], tags[0]))) == 300 == len(out[mods[0]])

        plain = sweep.main_analysis(["-P", P, "--models-dir", str(d)] + common).numpy()
        listed = _files(d)
        df = sweep.main_analysis(["-P", P, "--models-dir", str(d), "--given", "all", "--bootstrap", "200"] + common)
        new = sorted(set(_files(d)) - set(listed))
        assert new == sorted([base / f"group_analysis_given_{P}.csv", base / f"group_analysis_given_{P}_bootstrap.csv"])
        tab = pd.read_csv(d / base / f"group_analysis_given_{P}.csv", float_precision="round_trip")
        assert list(tab.columns) == ["given", "target", "fold"] + list(metrics.POSTHOC_COLUMNS)
        assert len(tab) == 7 * (len(mods) + 1) * 3 and len(df) == len(tab)
        row = tab[(tab["given"] == full) & (tab["target"] == "mean")]
        assert list(row["fold"]) == ["0", "1", "pooled"]
        for k in (0, 1):                                               # the full set's mean score IS the plain analysis's
            assert float(row["roc_auc"].iloc[k]) == float(plain[k, 0]), k
            assert row.iloc[k][list(metrics.POSTHOC_COLUMNS)].to_numpy(dtype=plain.dtype).tobytes() == plain[k].tobytes(), k
        assert ((tab["roc_auc"] >= 0) & (tab["roc_auc"] <= 1)).all() and tab["roc_auc"].nunique() > 3
        boot = pd.read_csv(d / base / f"group_analysis_given_{P}_bootstrap.csv")
        assert list(boot["given"]) == tags and (boot["n_boot"] == 200).all()
        assert np.all(boot["ci_lo"] <= boot["roc_auc"]) and np.all(boot["roc_auc"] <= boot["ci_hi"])
        pooled_full = float(row["roc_auc"].iloc[2])
        assert abs(float(boot["roc_auc"].iloc[-1]) - pooled_full) <= 1e-6
        vs = boot[boot["given"] != full]
        assert np.isnan(boot["vs_full_delta_auc"].iloc[-1]) and np.isfinite(vs["vs_full_delta_auc"]).all()
        assert np.allclose(vs["vs_full_delta_auc"], vs["roc_auc"] - pooled_full, atol=1e-6)
        assert np.all(vs["vs_full_ci_lo"] <= vs["vs_full_ci_hi"]) and ((vs["vs_full_p_boot"] >= 0) & (vs["vs_full_p_boot"] <= 1)).all()
        text = capsys.readouterr().out
        assert f"given {tags[0]}: pooled AUC " in text and f"against {full}: delta AUC " in text
