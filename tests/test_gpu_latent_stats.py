"""nm_latent_stats / nm_latent_score (csrc/nm_metrics.hip) on synthetic device tensors against float64 numpy: cohorts that
cross a round boundary of the chunk merge (more than 256 // Z chunks of 128 rows), widths that leave threads idle, Z = 1 and
the maximum Z = 64, data with a large common offset, an empty cohort between full ones, pitch > Z with NaN in the padding,
score sets beyond one pass of the thread block.  Bounds (tests/fusion_ref.py): the statistics are formed in fp64 and rounded
once -- 1 ulp of np.mean / np.var of the widened input; zsep 4 eps32 |ref|; score (Z + 4) eps32 ref."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from multi_modal_normative_modeling_amd import _lib, engine
from tests import fusion_ref as F
from tests import latent_ref as LR

DEV = "cuda:0"
CANARY = -12345.678
EPS = F.EPS32


def _stream():
    return torch.cuda.current_stream().cuda_stream


@pytest.mark.parametrize("Z", sorted({z for _, z in F.LATENT_CASES}))
def test_stats_every_cohort_in_one_launch_and_alone(Z):
    """Every case of this width, each with the three kinds of data, as cohorts of one launch (an empty one between the first
    two), then one by one: within 1 ulp of float64 numpy, the same bits both ways and run to run."""
    sets = [F.latent_inputs(n, z, kind) for n, z in F.LATENT_CASES if z == Z for kind in F.LATENT_KINDS]
    sets.insert(1, np.zeros((0, Z), np.float32))
    dev = [torch.from_numpy(s).to(DEV) for s in sets]
    mean, var = engine.latent_stats(dev)
    mean2, var2 = engine.latent_stats(dev)
    assert torch.equal(mean[2:], mean2[2:]) and torch.equal(var[2:], var2[2:]) and torch.equal(mean[0], mean2[0])
    mean, var = mean.cpu().numpy(), var.cpu().numpy()
    worst = [0.0, 0.0]
    for k, s in enumerate(sets):
        if s.shape[0] == 0:
            assert np.isnan(mean[k]).all() and np.isnan(var[k]).all()                  # an empty cohort has no statistics
            continue
        s64 = s.astype(np.float64)
        u_m, u_v = F.ulps32(mean[k], s64.mean(0)).max(), F.ulps32(var[k], s64.var(0)).max()
        worst = [max(worst[0], u_m), max(worst[1], u_v)]
        assert u_m <= 1.0 and u_v <= 1.0, (k, s.shape, u_m, u_v)
        if s.shape[0] == 1:
            assert np.array_equal(mean[k], s[0]) and not var[k].any()                  # one row: itself, exactly zero variance
        mk, vk = engine.latent_stats([dev[k]])
        assert np.array_equal(mk.cpu().numpy()[0].view(np.uint32), mean[k].view(np.uint32)), (k, s.shape)
        assert np.array_equal(vk.cpu().numpy()[0].view(np.uint32), var[k].view(np.uint32)), (k, s.shape)
    print(f"nm_latent_stats Z={Z}: {len(sets)} cohorts, worst mean {worst[0]:.2f} ulp, var {worst[1]:.2f} ulp (bound 1)")


def _pitched(a, pitch, fill=np.nan):
    """a [rows, Z] as the first Z columns of a [rows, pitch] device buffer whose other columns hold `fill`."""
    buf = torch.full((a.shape[0], pitch), fill, dtype=torch.float32)
    buf[:, :a.shape[1]] = torch.from_numpy(a)
    return buf.to(DEV)


@pytest.mark.parametrize("pitch", [9, 64])
def test_pitch_beyond_z_reads_no_padding_and_writes_none(pitch):
    """Z = 6 on a view of a wider buffer (pitch Z + 3 and 64) whose padding holds NaN: the same bits as the dense call (one
    cohort crosses a round boundary), zsep written into the same pitch with the padding untouched."""
    Z = 6
    sets = [F.latent_inputs(5377, Z, "offset1e4"), F.latent_inputs(300, Z, "normal", seed=1)]
    lvs = [np.random.default_rng(3 + k).uniform(-20, 5, s.shape).astype(np.float32) for k, s in enumerate(sets)]
    rows = sum(s.shape[0] for s in sets)
    offs = torch.tensor([0, sets[0].shape[0], rows], dtype=torch.int32, device=DEV)
    mu_p, lv_p = _pitched(np.concatenate(sets), pitch), _pitched(np.concatenate(lvs), pitch)
    lib = _lib.load()
    stats = torch.full((2, 2 * Z + 1), CANARY, dtype=torch.float32, device=DEV)        # (a slack element behind each output)
    _lib.check(lib.nm_latent_stats(mu_p.data_ptr(), offs.data_ptr(), 2, Z, pitch, stats[0].data_ptr(), stats[1].data_ptr(), _stream()),
               "nm_latent_stats")
    dev = [torch.from_numpy(s).to(DEV) for s in sets]
    mean, var = engine.latent_stats(dev)
    assert torch.equal(stats[0, :2 * Z].view(2, Z), mean) and torch.equal(stats[1, :2 * Z].view(2, Z), var)
    assert float(stats[0, -1]) == np.float32(CANARY) and float(stats[1, -1]) == np.float32(CANARY)
    for k, s in enumerate(sets):
        s64 = s.astype(np.float64)
        assert F.ulps32(mean[k].cpu().numpy(), s64.mean(0)).max() <= 1.0 and F.ulps32(var[k].cpu().numpy(), s64.var(0)).max() <= 1.0
    # the scores of each set against the OTHER cohort's statistics
    mean_x, var_x = mean.flip(0).contiguous(), var.flip(0).contiguous()
    zsep = torch.full((rows, pitch), CANARY, dtype=torch.float32, device=DEV)
    score = torch.full((rows + 1,), CANARY, dtype=torch.float32, device=DEV)
    _lib.check(lib.nm_latent_score(mu_p.data_ptr(), lv_p.data_ptr(), offs.data_ptr(), 2, Z, pitch, mean_x.data_ptr(), var_x.data_ptr(),
                                   zsep.data_ptr(), score.data_ptr(), _stream()), "nm_latent_score")
    z_d, s_d = engine.latent_scores(dev, [torch.from_numpy(l).to(DEV) for l in lvs], mean_x, var_x)
    assert torch.equal(zsep[:, :Z], torch.cat(z_d)) and torch.equal(score[:rows], torch.cat(s_d))
    assert bool((zsep[:, Z:] == np.float32(CANARY)).all()) and float(score[-1]) == np.float32(CANARY)
    assert bool(torch.isfinite(zsep[:, :Z]).all()) and bool(torch.isfinite(score[:rows]).all())


@pytest.mark.parametrize("n,Z", F.SCORE_CASES)
def test_scores_against_another_cohorts_statistics(n, Z):
    rng = np.random.default_rng(100 * n + Z)
    cohort = (0.3 + 1.2 * rng.standard_normal((400, Z))).astype(np.float64)
    mean, var = cohort.mean(0).astype(np.float32), cohort.var(0).astype(np.float32)
    mu = rng.standard_normal((n, Z)).astype(np.float32)
    lv = rng.uniform(-20.0, 5.0, (n, Z)).astype(np.float32)
    d_mu, d_lv = torch.from_numpy(mu).to(DEV), torch.from_numpy(lv).to(DEV)
    d_mean, d_var = torch.from_numpy(mean[None]).to(DEV), torch.from_numpy(var[None]).to(DEV)
    zs, sc = engine.latent_scores([d_mu], [d_lv], d_mean, d_var)
    zs, sc = zs[0].cpu().numpy(), sc[0].cpu().numpy()
    z_ref, s_ref = LR.scores_given_stats(mean, var, mu, lv)
    r_z = float(np.max(np.abs(zs - z_ref) / (EPS * np.abs(z_ref))))
    r_s = float(np.max(np.abs(sc - s_ref) / (EPS * s_ref)))
    print(f"nm_latent_score n={n} Z={Z}: zsep off by {r_z:.2f} eps32 |ref| (bound 4), score by {r_s:.2f} eps32 ref (bound {Z + 4})")
    assert r_z <= 4.0 and r_s <= Z + 4
    # one output at a time: the bits of the run that asked for both
    lib = _lib.load()
    offs = torch.tensor([0, n], dtype=torch.int32, device=DEV)
    only_z = torch.full((n * Z + 1,), CANARY, dtype=torch.float32, device=DEV)
    only_s = torch.full((n + 1,), CANARY, dtype=torch.float32, device=DEV)
    for z_out, s_out in ((only_z, None), (None, only_s)):
        _lib.check(lib.nm_latent_score(d_mu.data_ptr(), d_lv.data_ptr(), offs.data_ptr(), 1, Z, Z, d_mean.data_ptr(), d_var.data_ptr(),
                                       z_out.data_ptr() if z_out is not None else None,
                                       s_out.data_ptr() if s_out is not None else None, _stream()), "nm_latent_score")
    assert np.array_equal(only_z.cpu().numpy()[:-1].reshape(n, Z).view(np.uint32), zs.view(np.uint32))
    assert np.array_equal(only_s.cpu().numpy()[:-1].view(np.uint32), sc.view(np.uint32))
    assert float(only_z[-1]) == np.float32(CANARY) and float(only_s[-1]) == np.float32(CANARY)
