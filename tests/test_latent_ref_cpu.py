"""tests/latent_ref.py -- the restatement of latent_deviation / separate_latent_deviation (utils_vae.py:155-161) the GPU
tests measure the device kernels against -- held to the literal numpy expressions, plus two sanity properties."""
import numpy as np

from tests import latent_ref as LR


def _arrays(seed, n_train=211, n=97, Z=10):
    g = np.random.default_rng(seed)
    return g.normal(0.3, 1.2, (n_train, Z)), g.normal(0.0, 1.5, (n, Z)), np.exp(g.normal(-1.0, 0.5, (n, Z)))


def test_helpers_equal_the_literal_expressions():
    for seed, Z in ((0, 10), (1, 1), (2, 32)):
        mt, ms, vs = _arrays(seed, Z=Z)
        var = np.var(mt, axis=0)
        want_sep = (ms - np.mean(mt, axis=0)) / np.sqrt(var + vs)
        want = np.sum(np.abs(ms - np.mean(mt, axis=0)) / np.sqrt(var + vs), axis=1) / ms.shape[1]
        assert np.array_equal(LR.separate_latent_deviation(mt, ms, vs), want_sep)
        assert np.array_equal(LR.latent_deviation(mt, ms, vs), want)
        assert want.shape == (ms.shape[0],) and want_sep.shape == ms.shape
        # the score is the row mean of |z|
        np.testing.assert_allclose(want, np.abs(want_sep).mean(1), rtol=1e-13)
        # ... and the form with the statistics handed in agrees with both
        zs, sc = LR.scores_given_stats(np.mean(mt, axis=0), var, ms, np.log(vs))
        np.testing.assert_allclose(zs, want_sep, rtol=1e-12, atol=1e-14)
        np.testing.assert_allclose(sc, want, rtol=1e-12)


def test_population_variance_is_what_the_reference_takes():
    mt, ms, vs = _arrays(3)
    z = LR.separate_latent_deviation(mt, ms, vs)
    ddof1 = (ms - mt.mean(0)) / np.sqrt(np.var(mt, axis=0, ddof=1) + vs)
    assert np.abs(z - ddof1).max() > 1e-6                         # (the two differ: np.var's default, ddof 0, is the one)


def test_cohort_scored_against_itself_has_zero_column_mean_numerator():
    """A cohort against itself: sum over subjects of (mu - mean) is zero per column, so with one common posterior variance
    the column means of z vanish."""
    mt, _, _ = _arrays(4)
    z = LR.separate_latent_deviation(mt, mt, np.full_like(mt, 0.37))
    assert np.abs(z.mean(0)).max() < 1e-13


def test_permuting_the_train_rows_changes_nothing_beyond_summation_noise():
    mt, ms, vs = _arrays(5)
    perm = np.random.default_rng(9).permutation(mt.shape[0])
    np.testing.assert_allclose(LR.separate_latent_deviation(mt[perm], ms, vs), LR.separate_latent_deviation(mt, ms, vs),
                               rtol=1e-12, atol=1e-14)
    np.testing.assert_allclose(LR.latent_deviation(mt[perm], ms, vs), LR.latent_deviation(mt, ms, vs), rtol=1e-12)
