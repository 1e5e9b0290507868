"""CPU restatement of the reference's two latent-deviation helpers (utils_vae.py:155-161), in float64: the yardstick of the
device kernels nm_latent_stats / nm_latent_score.  mu_train [N_train, Z], mu_sample / var_sample [N, Z]."""
import numpy as np


def latent_deviation(mu_train, mu_sample, var_sample):
    """utils_vae.py:155-157: per subject, the mean over the latent dimensions of |z-score|."""
    var = np.var(mu_train, axis=0)
    return np.sum(np.abs(mu_sample - np.mean(mu_train, axis=0)) / np.sqrt(var + var_sample), axis=1) / mu_sample.shape[1]


def separate_latent_deviation(mu_train, mu_sample, var_sample):
    """utils_vae.py:159-161: the z-score per latent dimension."""
    var = np.var(mu_train, axis=0)
    return (mu_sample - np.mean(mu_train, axis=0)) / np.sqrt(var + var_sample)


def scores_given_stats(mean, var, mu_sample, logvar_sample):
    """The two helpers with the cohort statistics handed in (what nm_latent_score computes from): float64 throughout."""
    mean, var = np.asarray(mean, np.float64), np.asarray(var, np.float64)
    mu, lv = np.asarray(mu_sample, np.float64), np.asarray(logvar_sample, np.float64)
    zsep = (mu - mean) / np.sqrt(var + np.exp(lv))
    return zsep, np.sum(np.abs(mu - mean) / np.sqrt(var + np.exp(lv)), axis=1) / mu.shape[1]
