"""The modality-subset pass restated with the oracle's own pieces (oracle/cvae_ref.py): every expert's encoder once, then per
subset the fusion of that subset's experts, the latent draw and every decoder.

Per row r and subset s with experts A_s: E = A_s & present[r] (present None: every expert).  The joint posterior is
R.combine_latent over the experts of E alone -- its sums run over E, its M is |E|, the gPoE softmax sees the logits of E only
(the weights sum to 1) -- without the single-expert bypass: the model has several experts, also where one is left.
z = mu_E + eps[r] exp(logvar_E / 2) with the SAME eps for every subset.  A row with E empty has no posterior: NaN."""
import torch

from oracle import cvae_ref as R


def mask_of(subset):
    m = 0
    for i in subset:
        m |= 1 << int(i)
    return m


def all_subsets(M):
    """Every non-empty subset of M experts, by ascending mask."""
    return [tuple(i for i in range(M) if (mask >> i) & 1) for mask in range(1, 1 << M)]


def encode(P, spec, xes, cs):
    enc = [R.encoder_fwd(P, spec, m, xes[m], cs[m]) for m in range(spec.M)]
    mus = torch.stack([e[0] for e in enc])
    logvars = torch.stack([e[1] for e in enc])
    return mus, logvars


def fuse(P, spec, mus, variances, combine, E):
    """The joint (mu, variance) of the experts in the list E over all rows of mus / variances [M, N, Z]."""
    E = list(E)
    alphas = [P[f"alpha_m_list.{m}"] for m in range(spec.M)]
    return R.combine_latent(mus[E], variances[E], combine, [alphas[m] for m in E], single_bypass=False)


def forward_subsets(P, spec, xes, cs, combine, eps, subsets, present=None):
    """Per subset {"locs": [loc_m], "mu", "var", "z"}.  present: None or one integer per row, bit m = expert m observed."""
    N = xes[0].shape[0]
    mus, logvars = encode(P, spec, xes, cs)
    variances = torch.exp(logvars)
    pres = torch.full((N,), (1 << spec.M) - 1, dtype=torch.long) if present is None else torch.as_tensor(present).long()
    out = []
    for sub in subsets:
        eff = pres & mask_of(sub)
        mu = torch.full((N, spec.latent), float("nan"))
        var = torch.full((N, spec.latent), float("nan"))
        for e in sorted(set(eff.tolist())):
            if e == 0:
                continue
            rows = (eff == e).nonzero().flatten()
            E = [i for i in range(spec.M) if (e >> i) & 1]
            if rows.numel() == N:                                   # (no gather: the tensors of the full pass themselves)
                mu, var = fuse(P, spec, mus, variances, combine, E)
            else:
                mu_e, var_e = fuse(P, spec, mus[:, rows], variances[:, rows], combine, E)
                mu[rows], var[rows] = mu_e.detach(), var_e.detach()
        logvar = torch.log(var)
        z = R.reparameterise(mu, logvar, eps)
        zd = torch.nan_to_num(z, nan=0.0)
        locs = []
        for m in range(spec.M):
            loc = R.decoder_fwd(P, spec, m, zd, cs[m])[0].detach().clone()
            loc[eff == 0] = float("nan")
            locs.append(loc)
        out.append({"locs": locs, "mu": mu.detach(), "var": var.detach(), "z": z.detach()})
    return out


def exports(xes, res, present=None):
    """(out_loc, out_sqerr, out_rowdev) per modality of one subset's result: squared residuals and their row means, NaN on
    the rows whose present bits lack the modality (x is a placeholder there)."""
    out = []
    for m, loc in enumerate(res["locs"]):
        sq = (xes[m] - loc) ** 2
        if present is not None:
            miss = ((torch.as_tensor(present).long() >> m) & 1) == 0
            sq[miss] = float("nan")
        out.append((loc, sq, sq.sum(1) / sq.shape[1]))
    return out
