"""The yardstick of nm_column_regress (own code, numpy + scipy, float64): per column of a table the fit
target ~ const + column + covariates over the included rows -- the columns of metrics.COLUMN_REGRESS_COLUMNS, by the
definitions of include/nmhip.h:

    the design       Z = (1, x - mean(x), cov - mean(cov)) over the included rows, P = 2 + q columns; slopes are those of the
                     raw design, const = b0 - m.b, var_const = g' C g with g = (1, -m)
    ols              b = solve(Z'Z, Z'y); s^2 = RSS / (n - P); C = s^2 (Z'Z)^-1; p = I_x(df / 2, 1 / 2) at x = df / (df + t^2), by scipy's betainc
    logit            Newton from zero: step = solve(H, Z'(y - p)), H = Z' diag(p (1 - p)) Z; converged when every |step| <= TOL,
                     at most MAX_ITER steps; C = H^-1 at the final parameters; p = erfc(|z| / sqrt 2)
    positive definite   every Cholesky pivot d_j > PIVOT * A_jj
    n_iter           the Newton steps (0 for ols);  -1: a logit that did not converge or lost positive definiteness after its
                     first step;  -2: invalid input (a non-finite value in an included row, n <= P, a constant column, a singular
                     design, for logit a target outside {0, 1} or one class only);  the six statistics are NaN in both cases

`table` fits all columns at once (stacked matrices); `ols_raw` is the textbook fit on the raw normal equations, kept to show
what centring is for; `latent_pvalues` is the reference's DataFrame (utils_vae.py:163-174) from `table`."""
import numpy as np
from scipy import special

COLUMNS = ("const", "coef", "se_const", "se_coef", "p_const", "p_coef", "n_obs", "n_iter")
MAX_ITER = 35
TOL = 1e-8
PIVOT = 1e-12


def student_t_two_sided(t, df):
    """P(|T_df| >= |t|) = I_x(df / 2, 1 / 2) at x = df / (df + t^2).  For t^2 < 1 (p above 0.3) the complement 1 - I_{1-x}(1 / 2, df / 2) with
    1 - x = t^2 / (df + t^2) formed directly: x itself rounds near 1 and would cost a small t its digits (at t = 1e-4, 4e-10 of p)."""
    t = np.asarray(t, dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        t2 = t * t
        return np.where(t2 < 1.0, 1.0 - special.betainc(0.5, 0.5 * df, t2 / (df + t2)), special.betainc(0.5 * df, 0.5, df / (df + t2)))


def pivots_ok(A):
    """[K] booleans: every pivot of the Cholesky factorisation of A[k] exceeds PIVOT times its diagonal entry."""
    K, P, _ = A.shape
    L = np.zeros_like(A)
    ok = np.ones(K, dtype=bool)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        for j in range(P):
            d = A[:, j, j] - (L[:, j, :j] ** 2).sum(1)
            ok &= d > PIVOT * A[:, j, j]
            l = np.sqrt(d)
            L[:, j, j] = l
            for i in range(j + 1, P):
                L[:, i, j] = (A[:, j, i] - (L[:, i, :j] * L[:, j, :j]).sum(1)) / l
    return ok


def table(x, target, cov=None, include=None, kind="ols"):
    """[D, 8] float64 (COLUMNS) of one set: x [rows, D], target [rows], cov [rows, q] or None, include [rows] or None."""
    assert kind in ("ols", "logit")
    x = np.asarray(x, dtype=np.float64)
    rows, D = x.shape
    keep = np.ones(rows, dtype=bool) if include is None else np.asarray(include).reshape(-1) != 0
    xi = x[keep]
    y = np.asarray(target, dtype=np.float64).reshape(-1)[keep]
    c = np.zeros((rows, 0)) if cov is None else np.asarray(cov, dtype=np.float64).reshape(rows, -1)
    c = c[keep]
    n, q = xi.shape[0], c.shape[1]
    P = 2 + q
    out = np.full((D, 8), np.nan)
    out[:, 6], out[:, 7] = n, -2
    bad_set = not (np.isfinite(y).all() and np.isfinite(c).all()) or n <= P
    if kind == "logit" and not bad_set:
        bad_set = not np.isin(y, (0.0, 1.0)).all() or y.sum() == 0 or y.sum() == n
    if bad_set:
        return out
    with np.errstate(invalid="ignore"):
        cols = np.flatnonzero(np.isfinite(xi).all(0) & (xi.min(0) < xi.max(0)))
    if cols.size == 0:
        return out
    K = cols.size
    m = np.concatenate([np.zeros((K, 1)), xi[:, cols].mean(0)[:, None], np.repeat(c.mean(0)[None, :], K, 0)], 1)   # [K, P]
    Z = np.empty((K, n, P))
    Z[:, :, 0] = 1.0
    Z[:, :, 1] = (xi[:, cols] - m[:, 1]).T
    Z[:, :, 2:] = (c - c.mean(0))[None, :, :]
    beta = np.zeros((K, P))
    cov_b = np.full((K, P, P), np.nan)
    n_iter = np.zeros(K, dtype=np.int64)
    state = np.zeros(K, dtype=np.int64)            # 0 iterating, 1 converged: the Hessian is due, 2 done, 3 failed, 4 invalid
    if kind == "ols":
        A = np.einsum("knp,knq->kpq", Z, Z)
        g = np.einsum("knp,n->kp", Z, y)
        ok = pivots_ok(A)
        state[~ok] = 4
        beta[ok] = np.linalg.solve(A[ok], g[ok][:, :, None])[:, :, 0]
        rss = ((y[None, :] - np.einsum("knp,kp->kn", Z, beta)) ** 2).sum(1)
        with np.errstate(invalid="ignore", divide="ignore"):
            cov_b[ok] = np.linalg.inv(A[ok]) * (rss[ok] / (n - P))[:, None, None]
        state[ok] = 2
    else:
        while np.any(state <= 1):
            with np.errstate(over="ignore", invalid="ignore"):
                p = 1.0 / (1.0 + np.exp(-np.einsum("knp,kp->kn", Z, beta)))
                H = np.einsum("knp,kn,knq->kpq", Z, p * (1.0 - p), Z)
                g = np.einsum("knp,kn->kp", Z, y[None, :] - p)
            pd = pivots_ok(H)
            live = state <= 1
            lost = live & ~pd
            state[lost] = np.where(n_iter[lost] == 0, 4, 3)
            last = live & pd & (state == 1)
            cov_b[last] = np.linalg.inv(H[last])
            step_ = live & pd & (state == 0)
            state[last] = 2
            if np.any(step_):
                step = np.linalg.solve(H[step_], g[step_][:, :, None])[:, :, 0]
                beta[step_] += step
                n_iter[step_] += 1
                big = np.abs(step).max(1)
                with np.errstate(invalid="ignore"):
                    state[step_] = np.where(big <= TOL, 1, np.where((n_iter[step_] >= MAX_ITER) | np.isnan(big), 3, 0))
    done = state == 2
    gvec = np.concatenate([np.ones((K, 1)), -m[:, 1:]], 1)
    const = np.einsum("kp,kp->k", gvec, beta)
    with np.errstate(invalid="ignore", divide="ignore"):
        se0 = np.sqrt(np.einsum("kp,kpq,kq->k", gvec, cov_b, gvec))
        se1 = np.sqrt(cov_b[:, 1, 1])
        if kind == "ols":
            p0, p1 = student_t_two_sided(const / se0, n - P), student_t_two_sided(beta[:, 1] / se1, n - P)
        else:
            p0 = special.erfc(np.abs(const / se0) / np.sqrt(2.0))
            p1 = special.erfc(np.abs(beta[:, 1] / se1) / np.sqrt(2.0))
    res = np.stack([const, beta[:, 1], se0, se1, p0, p1], 1)
    res[~done] = np.nan
    out[cols, :6] = res
    out[cols, 7] = np.where(done, n_iter, np.where(state == 3, -1, -2))
    return out


def ols_raw(x, y):
    """(const, coef, se_const, se_coef) of y ~ const + x from the raw normal equations (no centring), float64."""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    Z = np.stack([np.ones_like(x), x], 1)
    A = Z.T @ Z
    b = np.linalg.solve(A, Z.T @ y)
    rss = ((y - Z @ b) ** 2).sum()
    C = np.linalg.inv(A) * (rss / (len(x) - 2))
    return b[0], b[1], np.sqrt(C[0, 0]), np.sqrt(C[1, 1])


def latent_pvalues(latent, target, type):
    import pandas as pd
    tab = table(np.asarray(latent, dtype=np.float32), np.asarray(target, dtype=np.float32),
                kind="ols" if type == "continuous" else "logit")
    pval_df = pd.DataFrame({"labels": ["const", "latent"]})
    for i in range(tab.shape[0]):
        pval_df["latent {0}".format(i)] = [float(tab[i, 4]), float(tab[i, 5])]
    return pval_df


def close(got, ref, tol=1e-9):
    """The closeness rule: n_obs, the status codes and NaN patterns exactly, a Logit's n_iter within 1 and inside 1..MAX_ITER,
    an estimate within tol x max(|ref|, its se), se and p within tol relative.  Returns the worst ratio error / bound over
    the table (<= 1 passes; inf where a pattern or an integer differs)."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    if got.shape != ref.shape or not np.array_equal(np.isnan(got), np.isnan(ref)):
        return np.inf
    if not np.array_equal(got[..., 6], ref[..., 6]) or not np.array_equal(got[..., 7] < 0, ref[..., 7] < 0):
        return np.inf
    bad = ref[..., 7] < 0
    gi, ri = got[..., 7], ref[..., 7]
    if not np.array_equal(gi[bad], ri[bad]) or np.any(np.abs(gi[~bad] - ri[~bad]) > 1) or np.any(gi != np.rint(gi)):
        return np.inf
    if np.any((ri[~bad] > 0) & ((gi[~bad] < 1) | (gi[~bad] > MAX_ITER))) or np.any((ri[~bad] == 0) & (gi[~bad] != 0)):
        return np.inf
    g, r = got[~bad], ref[~bad]
    if g.size == 0:
        return 0.0
    worst = 0.0
    with np.errstate(invalid="ignore", divide="ignore"):
        for est, se in ((0, 2), (1, 3)):
            err = np.abs(g[:, est] - r[:, est])
            worst = max(worst, float(np.where(err == 0, 0.0, err / (tol * np.maximum(np.abs(r[:, est]), r[:, se]))).max()))
        for k in (2, 3, 4, 5):
            err = np.abs(g[:, k] - r[:, k])
            worst = max(worst, float(np.where(err == 0, 0.0, err / (tol * np.abs(r[:, k]))).max()))
    return worst if worst == worst else np.inf


def make_case(rng, rows, D, q, kind):
    """A synthetic set (fp32): columns of different scales and offsets, q covariates, and a target that depends on the first
    columns and the covariates with effects small enough that |z| stays far below 30: (x, target, cov or None)."""
    x = rng.normal(size=(rows, D)) * rng.uniform(0.5, 3.0, D) + rng.uniform(-5.0, 5.0, D)
    cov = rng.normal(size=(rows, q)) + np.arange(q)
    lin = 0.5 * (x[:, 0] - x[:, 0].mean()) / x[:, 0].std() - 0.3 * (x[:, D // 2] - x[:, D // 2].mean()) / (x[:, D // 2].std() + 1e-30)
    lin = lin + cov @ (0.2 * np.ones(q)) if q else lin
    if kind == "ols":
        y = 1.5 + lin + rng.normal(size=rows)
    else:
        y = (rng.random(rows) < 1.0 / (1.0 + np.exp(-(0.2 + lin)))).astype(np.float64)
        if rows >= 2 and (y.sum() == 0 or y.sum() == rows):      # both classes present, whatever the draw
            y[0], y[1] = 0.0, 1.0
    return x.astype(np.float32), y.astype(np.float32), (cov.astype(np.float32) if q else None)
