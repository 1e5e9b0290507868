"""The likelihood pass restated in fp64 numpy (the definition in include/nmhip.h, nm_devpass_iw), with the error bound of
every returned value for an fp32 evaluation of the same definition.

    log w_s = sum_m [ll_const_m - 0.5 sum_d (x_d - x_hat_s,d)^2 / exp(logvar_out_d)] - 0.5 sum_k (z_s,k^2 - eps_s,k^2 - lv_k)
    log_px  = logsumexp_s(log w_s) - log S        elbo = mean_s log w_s        ess = (sum w)^2 / sum w^2
    kl_mc   = -mean_s a_s                          kl = 0.5 sum_k (mu_k^2 + exp(lv_k) - 1 - lv_k)
    recon_ll = mean_s sum_m ll_m,s                 logw_max / logw_min

Bounds (all from the definition, none from what a kernel returns):
    one log-weight   a recursive fp32 sum of n = (sum of the wanted D) + Z + M terms, each formed by at most four rounded
                     operations: b_s = (n + 8) 2^-23 sum_i |t_i|, from the fp64 terms, per row and draw
    log_px, elbo, logw_max, logw_min   1-Lipschitz in the sup-norm of the log-weights: max_s b_s + 2^-17 (1 + |value|)
                     (the second term: S <= 1024 additions of values in (0, 1] and a few-ulp expf / logf)
    ess              relative: expm1(4 max_s b_s) + 2^-16
    kl, kl_mc, recon_ll, recon_ll_m    the recursive-sum bound over their own terms
"""
import numpy as np

COLUMNS = ("log_px", "elbo", "ess", "kl_mc", "kl", "recon_ll", "logw_max", "logw_min")
LOG_2PI = float(np.log(2.0 * np.pi))
U = 2.0 ** -23


def ll_const(logvar_out):
    """-0.5 sum_d (logvar_out_d + log 2 pi) in fp64."""
    return float(-0.5 * (np.asarray(logvar_out, np.float64).reshape(-1) + LOG_2PI).sum())


def _sum_bound(n, abs_sum):
    return (n + 8) * U * abs_sum


def loglik(x, x_hat, mu, lv, eps, z, logvar_out, decoders=None):
    """x[m] [N, D_m]; x_hat[m] [S, N, D_m]; mu, lv [N, Z]; eps, z [S, N, Z]; logvar_out[m] [D_m]; decoders: the indices that
    enter the weight (default: all).  -> (values, bounds): dicts of [N] float64 arrays under COLUMNS and 'recon_ll_<m>' per
    wanted decoder, plus values['logw'] [S, N] and bounds['logw'] [S, N]."""
    M = len(x)
    dec = list(range(M)) if decoders is None else sorted(int(m) for m in decoders)
    mu, lv = np.asarray(mu, np.float64), np.asarray(lv, np.float64)
    eps, z = np.asarray(eps, np.float64), np.asarray(z, np.float64)
    S, N, Z = z.shape
    # latent terms, per k
    ta = -0.5 * (z * z - eps * eps - lv[None])                     # [S, N, Z]
    a = ta.sum(axis=2)
    abs_a = np.abs(ta).sum(axis=2)
    rec = np.zeros((S, N))
    abs_rec = np.zeros((S, N))
    ll_m, abs_m, n_m = {}, {}, {}
    for m in dec:
        xm = np.asarray(x[m], np.float64)
        xh = np.asarray(x_hat[m], np.float64)
        lvo = np.asarray(logvar_out[m], np.float64).reshape(-1)
        t = -0.5 * (xm[None] - xh) ** 2 / np.exp(lvo)[None, None]    # [S, N, D]
        c = ll_const(lvo)
        ll_m[m] = c + t.sum(axis=2)
        abs_m[m] = abs(c) + np.abs(t).sum(axis=2)
        n_m[m] = t.shape[2] + 1
        rec += ll_m[m]
        abs_rec += abs_m[m]
    logw = rec + a
    n = sum(n_m.values()) + Z
    b = _sum_bound(n, abs_rec + abs_a)                             # [S, N]
    bmax = b.max(axis=0)
    mxw = logw.max(axis=0)
    w = np.exp(logw - mxw[None])
    s1, s2 = w.sum(axis=0), (w * w).sum(axis=0)
    tk = 0.5 * (mu * mu + np.exp(lv) - 1.0 - lv)                   # [N, Z]
    val = {
        "log_px": mxw + np.log(s1) - np.log(S),
        "elbo": logw.mean(axis=0),
        "ess": s1 * s1 / s2,
        "kl_mc": -a.mean(axis=0),
        "kl": tk.sum(axis=1),
        "recon_ll": rec.mean(axis=0),
        "logw_max": mxw,
        "logw_min": logw.min(axis=0),
        "logw": logw,
    }
    lip = lambda v: bmax + 2.0 ** -17 * (1.0 + np.abs(v))
    bnd = {
        "log_px": lip(val["log_px"]), "elbo": lip(val["elbo"]), "logw_max": lip(val["logw_max"]), "logw_min": lip(val["logw_min"]),
        "ess": (np.expm1(4.0 * bmax) + 2.0 ** -16) * val["ess"],
        "kl_mc": _sum_bound(Z, abs_a).max(axis=0),
        "kl": _sum_bound(Z, np.abs(tk).sum(axis=1)),
        "recon_ll": _sum_bound(n - Z, abs_rec).max(axis=0),
        "logw": b,
    }
    for m in dec:
        val[f"recon_ll_{m}"] = ll_m[m].mean(axis=0)
        bnd[f"recon_ll_{m}"] = _sum_bound(n_m[m], abs_m[m]).max(axis=0)
    return val, bnd


def worst_ratio(got, val, bnd):
    """max over rows of |got - value| / bound."""
    return float((np.abs(np.asarray(got, np.float64) - val) / bnd).max())
