"""The latent-space deviation on the device (latent_deviation / separate_latent_deviation, utils_vae.py:155-161, on what
pred_latent returns, cVAE.py:539-545): the encoder-only kernel nm_latent_pass against the general forward kernel bit for bit
at every shape class it admits (one expert included); many models in one launch; the shapes it refuses; the cohort statistics
and z-scores (nm_latent_stats / nm_latent_score) against the reference arithmetic in float64 on the pass's own exports and
against the oracle; the drop-in classes' pred_latent; sweep.latent_folds and the `test --latent` command line."""
import filecmp
import functools
import shutil
import tempfile
from pathlib import Path

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import multi_modal_normative_modeling_amd as nm
from multi_modal_normative_modeling_amd import engine, prep, sweep
from oracle import cvae_ref as R
from tests import latent_ref as LR
from tests.golden_util import Golden
from tests.hip_harness import rel_err
from tests.test_gpu_devpass_multi import _data, _tables

DEV = "cuda:0"


def _job(tables, dims, hidden, Z, c_dim, combine, seed, kind="multimodal", state=None, bypass=True, fill=None):
    """A job with the joint-latent exports on and nothing else; fill: the value the export buffers hold before the launch."""
    spec = nm.ModelSpec(list(dims), list(hidden), Z, c_dim, True, kind)
    job = nm.Job(spec, tables, combine=combine, state=state, seed=seed, init_seed=seed, n_tiles_ws=tables[0].n_tiles,
                 single_bypass=bypass)
    job.enable_exports(loc=False, sqerr=False, rowdev=False, latent=True)
    if fill is not None:
        job.out_mu.fill_(fill)
        job.out_logvar.fill_(fill)
    return job


CASES = [
    # N, D per modality, hidden, Z, c_dim, combine, own covariates per modality, kind, single-expert bypass
    (300, (61, 90, 47), (64, 48), 12, 3, "poe", False, "multimodal", True),     # two full 128-row tiles, a 44-row one, an empty half
    (300, (61, 90, 47), (64, 48), 12, 3, "gpoe", False, "multimodal", True),
    (300, (61, 90, 47), (64, 48), 12, 3, "moe", False, "multimodal", True),
    (300, (61, 90, 47), (64, 48), 12, 3, "mopoe", False, "multimodal", True),
    (129, (40, 40, 40, 120), (112,), 32, 5, "gpoe", False, "multimodal", True), # four experts, both limits, one row in tile 2
    (40, (116, 50), (110, 110), 10, 2, "poe", False, "multimodal", True),       # fewer rows than a tile; Z not a multiple of 4
    (300, (61, 90, 47), (64, 48), 12, 3, "mopoe", True, "multimodal", True),    # every modality its own covariates
    (300, (61,), (64, 48), 12, 3, "poe", False, "multimodal", True),            # one expert, single bypass: heads -> exports
    (40, (61,), (64, 48), 10, 3, "poe", False, "multimodal", True),
    (300, (61,), (64, 48), 12, 3, "poe", False, "single", True),                # ... the cVAE class
    (300, (61,), (64, 48), 12, 3, "poe", False, "multimodal", False),           # ... bypass off (mmJSD): product with the prior
    (40, (61,), (64, 48), 10, 3, "gpoe", False, "multimodal", False),
]


@pytest.mark.parametrize("N,dims,hidden,Z,c_dim,combine,own_cov,kind,bypass", CASES)
def test_latent_pass_equals_general_forward_bit_for_bit(N, dims, hidden, Z, c_dim, combine, own_cov, kind, bypass):
    xs, cs = _data(N, dims, c_dim, seed=21, own_cov=own_cov)
    tables = _tables(xs, cs)
    gen = _job(tables, dims, hidden, Z, c_dim, combine, seed=11, kind=kind, bypass=bypass)
    nm.JobSet([gen]).forward()                                        # the general kernel with the latent exports
    cmp_ = _job(tables, dims, hidden, Z, c_dim, combine, seed=11, kind=kind, bypass=bypass, fill=7.0)
    js = nm.JobSet([cmp_])
    assert js.latent_ok()
    js.latent(compact=True)
    torch.cuda.synchronize()
    for what, a, b in (("out_mu", gen.out_mu, cmp_.out_mu), ("out_logvar", gen.out_logvar, cmp_.out_logvar)):
        a, b = a.cpu(), b.cpu()
        assert torch.equal(a[:N], b[:N]), (what, float((a[:N] - b[:N]).abs().max()))
        assert float(b[:N].abs().max()) > 0 and float(b[:N].abs().min()) > 0, what
        assert b.shape[0] > N and float(b[N:].abs().max()) == 0.0, what          # rows past the table: zeros, not the 7.0


def test_twenty_models_in_one_launch_equal_each_alone():
    N, dims, hidden, Z, cd = 300, (61, 90, 47), (64, 48), 12, 3
    xs, cs = _data(N, dims, cd, seed=8)
    tables = _tables(xs, cs)
    one = _tables([xs[0]], [cs[0]])
    def make(j):        # every fourth model has one expert: both paths of the kernel in one launch
        if j % 4 == 3:
            return _job(one, dims[:1], hidden, Z, cd, "poe", seed=100 + j)
        return _job(tables, dims, hidden, Z, cd, ("gpoe", "poe", "moe")[j % 4], seed=100 + j)
    jobs = [make(j) for j in range(20)]
    js = nm.JobSet(jobs)
    assert js.latent_ok()
    js.latent(compact=True)
    torch.cuda.synchronize()
    for j in range(20):
        alone = make(j)
        nm.JobSet([alone]).latent(compact=True)
        torch.cuda.synchronize()
        assert torch.equal(alone.out_mu, jobs[j].out_mu) and torch.equal(alone.out_logvar, jobs[j].out_logvar), j
        assert float(jobs[j].out_mu[:N].abs().max()) > 0


@pytest.mark.parametrize("why", ["general-shape path", "NMHIP_LATENT=0", "dmvae"])
def test_fallbacks_run_on_the_general_kernel(why, monkeypatch):
    N, dims, cd = 300, (61, 90, 47), 3
    hidden, kind = ((300, 300), "multimodal") if why == "general-shape path" else ((64, 48), "dmvae" if why == "dmvae" else "multimodal")
    xs, cs = _data(N, dims, cd, seed=13)
    if kind == "dmvae":                                              # (covariate-free networks: tables without the block)
        xs, cs = [torch.sigmoid(x) for x in xs], [torch.zeros(N, 0)] * 3
    job = _job(_tables(xs, cs), dims, hidden, 12, cd, "poe", seed=6, kind=kind)
    if why == "NMHIP_LATENT=0":
        assert nm.JobSet([job]).latent_ok()
        monkeypatch.setenv("NMHIP_LATENT", "0")
    js = nm.JobSet([job])
    assert not js.latent_ok() and not js.latent_pick()
    seen = []
    real = nm.JobSet._issue
    monkeypatch.setattr(nm.JobSet, "_issue", lambda self, entry, *a: (seen.append(entry), real(self, entry, *a))[1])
    js.latent()
    torch.cuda.synchronize()
    assert seen and "nm_latent_pass" not in seen
    assert float(job.out_mu[:N].abs().max()) > 0 and float(job.out_logvar[:N].abs().max()) > 0
    with pytest.raises(ValueError):
        js.latent(compact=True)


@functools.lru_cache(maxsize=None)
def _golden_run(name):
    """The golden's weights on a 300-row train table (seed 31) and a 300-row test table (seed 5): the pass's exports, the
    device statistics and scores -- computed once, shared by the tests below, never modified."""
    g = Golden(name)
    N = 300
    P = {k: v for k, v in g.weights("w0").items()}
    data = {s: _data(N, g.dims, g.c_dim, seed=s) for s in (31, 5)}
    jobs = {s: _job(_tables(*data[s]), g.dims, g.hidden, g.Z, g.c_dim, g.combine, seed=0, state=P) for s in (31, 5)}
    js = nm.JobSet([jobs[31], jobs[5]])
    assert js.latent_ok()
    js.latent(compact=True)
    mean, var = nm.JobSet([jobs[31]]).latent_stats()
    zsep, score = nm.JobSet([jobs[5]]).latent_scores(mean, var)
    torch.cuda.synchronize()
    return {"g": g, "N": N, "P": P, "data": data, "jobs": jobs, "mean": mean, "var": var, "zsep": zsep[0], "score": score[0],
            "mu_tr": jobs[31].out_mu[:N].cpu().numpy(), "mu_te": jobs[5].out_mu[:N].cpu().numpy(),
            "lv_te": jobs[5].out_logvar[:N].cpu().numpy()}


def _ulps(got, want):
    want = np.asarray(want, np.float32)
    return np.abs(got.astype(np.float64) - want.astype(np.float64)) / np.spacing(np.abs(want)).astype(np.float64)


def test_stats_and_scores_equal_the_reference_arithmetic_on_the_exports():
    r = _golden_run("mm3_gpoe")
    mean, var = r["mean"].cpu().numpy()[0], r["var"].cpu().numpy()[0]
    mu64 = r["mu_tr"].astype(np.float64)
    u_mean, u_var = _ulps(mean, np.mean(mu64, axis=0).astype(np.float32)), _ulps(var, np.var(mu64, axis=0).astype(np.float32))
    print(f"stats: mean off by {u_mean.max():.2f} ulp, var by {u_var.max():.2f} ulp (bound 2); min var {var.min():.3e}")
    assert u_mean.max() <= 2 and u_var.max() <= 2
    zs_ref, sc_ref = LR.scores_given_stats(mean, var, r["mu_te"], r["lv_te"])
    zs, sc = r["zsep"].cpu().numpy(), r["score"].cpu().numpy()
    print(f"zsep: max |got - ref| {np.abs(zs - zs_ref).max():.3e} (max |z| {np.abs(zs_ref).max():.3f}); "
          f"score: max rel {np.abs(sc / sc_ref - 1).max():.3e}")
    np.testing.assert_allclose(zs, zs_ref, rtol=1e-6, atol=1e-7)
    np.testing.assert_allclose(sc, sc_ref, rtol=4e-6, atol=0)
    # the same through the two reference helpers themselves, from the exported arrays
    np.testing.assert_allclose(zs, LR.separate_latent_deviation(mu64, r["mu_te"].astype(np.float64), np.exp(r["lv_te"].astype(np.float64))),
                               rtol=1e-5, atol=1e-6)


def test_stats_and_scores_are_deterministic_and_sets_are_independent():
    r = _golden_run("mm3_gpoe")
    a, b = r["jobs"][31], r["jobs"][5]
    N = r["N"]
    sets = [a.out_mu[:N], b.out_mu[:N], a.out_mu[:131], b.out_mu[7:8]]            # (131: one full chunk and three rows; one row)
    m1, v1 = engine.latent_stats(sets)
    m2, v2 = engine.latent_stats(sets)
    assert torch.equal(m1, m2) and torch.equal(v1, v2)
    assert torch.equal(m1[:1], r["mean"]) and torch.equal(v1[:1], r["var"])
    for k, s in enumerate(sets):
        mk, vk = engine.latent_stats([s])
        assert torch.equal(mk[0], m1[k]) and torch.equal(vk[0], v1[k]), k
    assert float(v1[3].abs().max()) == 0.0 and torch.equal(m1[3], b.out_mu[7])    # one row: its own mean, zero variance
    lvs = [b.out_logvar[:N], a.out_logvar[:N], b.out_logvar[:131], a.out_logvar[7:8]]
    mus = [b.out_mu[:N], a.out_mu[:N], b.out_mu[:131], a.out_mu[7:8]]
    z1, s1 = engine.latent_scores(mus, lvs, m1, v1)
    z2, s2 = engine.latent_scores(mus, lvs, m1, v1)
    for k in range(4):
        assert torch.equal(z1[k], z2[k]) and torch.equal(s1[k], s2[k]), k
        zk, sk = engine.latent_scores([mus[k]], [lvs[k]], m1[k:k + 1], v1[k:k + 1])
        assert torch.equal(zk[0], z1[k]) and torch.equal(sk[0], s1[k]), k
    assert torch.equal(z1[0], r["zsep"]) and torch.equal(s1[0], r["score"])
    # an empty cohort has no statistics
    me, ve = engine.latent_stats([a.out_mu[:0], a.out_mu[:N]])
    assert torch.isnan(me[0]).all() and torch.isnan(ve[0]).all() and torch.equal(me[1], r["mean"][0])


def _oracle_latent(r, mode):
    g = r["g"]
    rs = R.Spec(g.dims, g.hidden, g.Z, g.c_dim)
    R.set_operand_rounding(mode)
    try:
        out = {}
        for s in (31, 5):
            xs, cs = r["data"][s]
            with torch.no_grad():
                f = R.forward_multimodal(r["P"], rs, xs, [c.long() for c in cs], g.combine, torch.zeros(r["N"], g.Z))
            out[s] = (f["mu"].numpy().astype(np.float64), f["logvar"].numpy().astype(np.float64))
    finally:
        R.set_operand_rounding("fp32")
    return out


def _check_against_oracle(name, zs, sc, r):
    ref = {}
    for mode in ("fp32", "bf16"):
        o = _oracle_latent(r, mode)
        ref[mode] = (LR.separate_latent_deviation(o[31][0], o[5][0], np.exp(o[5][1])),
                     LR.latent_deviation(o[31][0], o[5][0], np.exp(o[5][1])))
    for what, got, k in (("z", zs, 0), ("score", sc, 1)):
        noise = float(np.abs(ref["bf16"][k] - ref["fp32"][k]).max())
        d16, d32 = float(np.abs(got - ref["bf16"][k]).max()), float(np.abs(got - ref["fp32"][k]).max())
        print(f"{name} {what}: |got - bf16| {d16:.3e}  |got - fp32| {d32:.3e}  noise {noise:.3e}  max |ref| {np.abs(ref['fp32'][k]).max():.3e}")
        assert d16 <= 1.5 * noise + 1e-5, (what, d16, noise)
        assert d32 <= 3.0 * noise + 1e-5, (what, d32, noise)


@pytest.mark.parametrize("name", ["mm3_gpoe", "mm4_uca_gpoe", "mm1_small"])
def test_latent_deviation_matches_the_oracle(name):
    r = _golden_run(name)
    _check_against_oracle(name, r["zsep"].cpu().numpy().astype(np.float64), r["score"].cpu().numpy().astype(np.float64), r)


def test_exported_mu_against_the_golden_pred_latent():
    """single_small holds the reference's pred_latent (after one Adam step, weights w1): the encoder-only kernel's export
    within the bound tests/test_gpu_api_sweep.py sets for cVAE.pred_latent."""
    g = Golden("single_small")
    x, c = g.t("x0"), g.t("c")
    job = _job([nm.Table(x, c, DEV)], g.dims, g.hidden, g.Z, g.c_dim, "poe", seed=0, kind="single", state=g.weights("w1"))
    nm.JobSet([job]).latent(compact=True)
    torch.cuda.synchronize()
    n = x.shape[0]
    assert rel_err(job.out_mu[:n].cpu(), torch.from_numpy(g.z["pred_latent"])) < 2e-2
    assert rel_err(job.out_logvar[:n].exp().cpu(), torch.from_numpy(g.z["pred_latent_var"])) < 2e-2


def test_pred_latent_of_the_drop_in_class_takes_the_encoder_only_kernel(monkeypatch):
    import pandas as pd
    r = _golden_run("mm3_gpoe")
    g = r["g"]
    model = nm.cVAE_multimodal(list(g.dims), list(g.hidden), g.Z, g.c_dim, modalities=g.M, non_linear=True)
    model.to(DEV)
    model.load_state_dict(r["P"])
    seen = []
    real = nm.JobSet._issue
    monkeypatch.setattr(nm.JobSet, "_issue", lambda self, entry, *a: (seen.append(entry), real(self, entry, *a))[1])
    out = {}
    for s in (31, 5):
        xs, cs = r["data"][s]
        out[s] = model.pred_latent([pd.DataFrame(x.numpy()) for x in xs], cs[0].long().numpy(), DEV, g.combine)
        assert out[s][0].shape == (r["N"], g.Z) and out[s][1].shape == (r["N"], g.Z)
    assert seen == ["nm_latent_pass", "nm_latent_pass"]
    # the arrays are the pass's own exports (same weights, same tables), the variance its exponential
    assert np.array_equal(out[5][0], r["mu_te"]) and np.array_equal(out[31][0], r["mu_tr"])
    np.testing.assert_allclose(out[5][1], np.exp(r["lv_te"]), rtol=2e-6)
    zs = model.separate_latent_deviation(out[31], out[5])
    sc = model.latent_deviation(out[31], out[5])
    assert zs.shape == (r["N"], g.Z) and sc.shape == (r["N"],)
    _check_against_oracle("pred_latent", zs.astype(np.float64), sc.astype(np.float64), r)
    # DataFrames in: pass + statistics + scores on the device in one call; (var -> log -> exp costs an ulp or two)
    frames = {s: ([pd.DataFrame(x.numpy()) for x in r["data"][s][0]], r["data"][s][1][0].long().numpy(), g.combine) for s in (31, 5)}
    sc2 = model.latent_deviation(frames[31], frames[5])
    assert np.array_equal(sc2, r["score"].cpu().numpy())
    np.testing.assert_allclose(sc, sc2, rtol=1e-5)
    # the other multimodal classes have the method too; a following forward_multimodal still works
    assert hasattr(nm.mmJSD, "pred_latent") and hasattr(nm.cVAE_multimodal_regression, "pred_latent")
    xs, cs = r["data"][5]
    fwd = model.forward_multimodal([x[:64].to(DEV) for x in xs], [cs[0][:64].long().to(DEV)] * g.M, g.combine)
    assert fwd["mu_multimodal"].shape == (64, g.Z)


def _trained_folds(K=3, n=300, d=40):
    cohort = prep.synthetic_cohort(n=n, d=d)
    folds = prep.kfold_indices(n, K, 42)
    mods = list(prep.HCP_MODALITIES)
    spec = nm.ModelSpec([d] * 3, [32, 24], 8, 29)
    jobs = []
    for k, (tr, _) in enumerate(folds):
        xs, cov = prep.fold_train_tables(cohort, mods, tr)
        job = nm.Job(spec, [nm.Table(x, cov, DEV) for x in xs], combine="gpoe", seed=1000 * k, init_seed=50 + k)
        nm.JobSet([job]).train(3)
        jobs.append(job)
    return cohort, folds, mods, jobs


def test_latent_folds_equals_the_fold_by_fold_form_and_its_csvs_read_back():
    import pandas as pd
    cohort, folds, mods, jobs = _trained_folds()
    K = len(folds)
    with tempfile.TemporaryDirectory() as da:
        many = sweep.latent_folds(jobs, cohort, folds, mods, "gpoe", DEV, out_dirs=[Path(da) / f"{k:03d}" for k in range(K)], name="SE-gPoE")
        assert len(many) == K
        for k, (tr, te) in enumerate(folds):
            one = sweep.latent_folds([jobs[k]], cohort, [folds[k]], mods, "gpoe", DEV)[0]
            for key in ("mu", "var", "z", "score"):
                assert np.array_equal(one[key], many[k][key]), (k, key)
            assert many[k]["mu"].shape == (len(te), 8) and many[k]["score"].shape == (len(te),)
            assert np.isfinite(many[k]["z"]).all() and float(np.abs(many[k]["z"]).max()) > 0
            # the score is the row mean of |z|; z follows from mu / var and the train cohort's statistics
            np.testing.assert_allclose(many[k]["score"], np.abs(many[k]["z"]).mean(1), rtol=1e-5)
            lat = pd.read_csv(Path(da) / f"{k:03d}" / "latent_SE-gPoE.csv")
            dev = pd.read_csv(Path(da) / f"{k:03d}" / "latent_deviation_SE-gPoE.csv")
            meta = ["participant_id", "DIA", "AGE", "PTGENDER"]
            assert list(lat.columns) == meta + [f"mu_{i}" for i in range(8)] + [f"var_{i}" for i in range(8)]
            assert list(dev.columns) == meta + ["Latent deviation"] + [f"z_{i}" for i in range(8)]
            assert np.array_equal(lat["participant_id"].to_numpy(), cohort.iid[te]) and np.array_equal(dev["DIA"].to_numpy(), cohort.dia[te])
            assert np.array_equal(lat.iloc[:, 4:12].to_numpy(dtype=np.float32), many[k]["mu"])
            assert np.array_equal(lat.iloc[:, 12:].to_numpy(dtype=np.float32), many[k]["var"])
            assert np.array_equal(dev["Latent deviation"].to_numpy(dtype=np.float32), many[k]["score"])
            assert np.array_equal(dev.iloc[:, 5:].to_numpy(dtype=np.float32), many[k]["z"])


def test_test_command_line_with_and_without_latent():
    """`sweep test` writes exactly the files it wrote before unless --latent is given; with it, the two latent tables per
    fold and for all folds together on top, and `analysis --score latent` scores the `Latent deviation` column."""
    import pandas as pd
    with tempfile.TemporaryDirectory() as d:
        a, b = Path(d) / "a", Path(d) / "b"
        sweep.main(["-P", "SE-gPoE", "-E", "2", "-K", "2", "-H", "32", "24", "8", "--subjects", "300", "--out-dir", str(a),
                    "--save-models", "--no-csv"])
        shutil.copytree(a, b)
        common = ["-P", "SE-gPoE", "-K", "2", "-H", "32", "24", "8", "--subjects", "300"]
        ea = sweep.main_test(common + ["--models-dir", str(a)])
        eb = sweep.main_test(common + ["--models-dir", str(b), "--latent"])
        assert all(np.array_equal(ea[m], eb[m]) for m in ea)
        fa = sorted(p.relative_to(a) for p in a.rglob("*") if p.is_file())
        fb = sorted(p.relative_to(b) for p in b.rglob("*") if p.is_file())
        assert not any("latent" in p.name for p in fa)
        extra = sorted(set(fb) - set(fa))
        base = Path("HCPimage") / "SE-gPoE"
        assert extra == sorted([base / f"{k:03d}" / f"{kind}_SE-gPoE.csv" for k in (0, 1) for kind in ("latent", "latent_deviation")]
                               + [base / f"{kind}_SE-gPoE.csv" for kind in ("latent", "latent_deviation")])
        for p in fa:
            if p.suffix == ".csv":                                       # (the .pt files were copied, not written by `test`)
                assert filecmp.cmp(a / p, b / p, shallow=False), p
        allf = pd.read_csv(b / base / "latent_deviation_SE-gPoE.csv")
        assert allf.shape == (300, 5 + 8) and np.isfinite(allf["Latent deviation"].to_numpy()).all()
        assert pd.read_csv(b / base / "latent_SE-gPoE.csv").shape == (300, 4 + 16)
        tab = sweep.main_analysis(["-P", "SE-gPoE", "-K", "2", "--models-dir", str(b), "--score", "latent"]).numpy()
        assert tab.shape == (2, 8) and (b / base / "group_analysis_latent.csv").exists() and not (b / base / "group_analysis.csv").exists()
        from oracle import metrics_ref as MR
        f1 = pd.read_csv(b / base / "001" / "latent_deviation_SE-gPoE.csv")
        ref = MR.posthoc_metrics(f1["Latent deviation"].to_numpy().astype(np.float32), (f1["DIA"].to_numpy() != 1).astype(np.int32))
        assert abs(tab[1, 0] - ref[0]) < 1e-9 and np.array_equal(tab[1, 2:5], np.asarray(ref[2:5]))
