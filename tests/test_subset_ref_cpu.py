"""tests/subset_ref.py -- the reference the GPU tests of the modality-subset pass compare against -- held to the oracle it
restates: the full subset IS R.forward_multimodal, a moe singleton is that expert's own posterior, a gPoE subset's weights
sum to 1, a subset's result does not depend on what else the list holds, and presence bits select the experts per row."""
import pytest
import torch

from oracle import cvae_ref as R
from tests import subset_ref as S

COMBINERS = ("poe", "gpoe", "moe", "mopoe")
SHAPES = {3: ((13, 9, 11), (16, 12), 6, 3), 4: ((7, 9, 5, 12), (16,), 5, 2)}


def _case(M, seed=0, N=23):
    dims, hidden, Z, c_dim = SHAPES[M]
    spec = R.Spec(list(dims), list(hidden), Z, c_dim)
    P = R.init_params(spec, seed=seed + 3)
    g = torch.Generator().manual_seed(seed)
    for m in range(M):                                   # distinct gPoE logits: equal ones would hide a wrong softmax
        P[f"alpha_m_list.{m}"] = torch.randn(P[f"alpha_m_list.{m}"].shape, generator=g)
    xs = [torch.randn(N, d, generator=g) for d in dims]
    c = torch.zeros(N, c_dim)
    c[torch.arange(N), torch.randint(0, c_dim, (N,), generator=g)] = 1
    eps = torch.randn(N, Z, generator=g)
    return spec, P, xs, [c.long()] * M, eps


@pytest.mark.parametrize("M", [3, 4])
@pytest.mark.parametrize("combine", COMBINERS)
def test_full_subset_is_forward_multimodal(M, combine):
    spec, P, xs, cs, eps = _case(M)
    want = R.forward_multimodal(P, spec, xs, cs, combine, eps)
    got = S.forward_subsets(P, spec, xs, cs, combine, eps, [tuple(range(M))])[0]
    for m in range(M):
        assert torch.equal(got["locs"][m], want["locs"][m].detach()), m
    assert torch.equal(got["mu"], want["mu"].detach()) and torch.equal(got["z"], want["z"].detach())


@pytest.mark.parametrize("M", [3, 4])
def test_moe_singleton_is_the_experts_own_posterior(M):
    spec, P, xs, cs, eps = _case(M, seed=1)
    mus, logvars = S.encode(P, spec, xs, cs)
    res = S.forward_subsets(P, spec, xs, cs, "moe", eps, [(m,) for m in range(M)])
    for m in range(M):
        assert torch.equal(res[m]["mu"], mus[m].detach()), m
        assert torch.equal(res[m]["var"], torch.exp(logvars[m]).detach()), m


@pytest.mark.parametrize("M", [3, 4])
def test_gpoe_weights_of_a_subset_sum_to_one(M):
    """With every expert at unit variance the gPoE precision is the sum of the weights: 1 for every subset -- and the joint
    mean the weighted mean of the subset's own softmax, not of the full model's."""
    spec, P, xs, cs, eps = _case(M, seed=2)
    N, Z = 5, spec.latent
    mus = torch.randn(M, N, Z, generator=torch.Generator().manual_seed(4))
    ones = torch.ones(M, N, Z)
    for E in S.all_subsets(M):
        mu, var = S.fuse(P, spec, mus, ones, "gpoe", E)
        assert torch.allclose(var, torch.ones(N, Z), rtol=0, atol=2e-7), E
        a = torch.softmax(torch.stack([P[f"alpha_m_list.{m}"].reshape(()) for m in E]), 0)
        assert abs(float(a.sum()) - 1.0) < 1e-6
        assert torch.allclose(mu, (mus[list(E)] * a.reshape(-1, 1, 1)).sum(0), rtol=1e-5, atol=1e-6), E


@pytest.mark.parametrize("combine", COMBINERS)
def test_a_subsets_result_does_not_depend_on_the_list(combine):
    spec, P, xs, cs, eps = _case(3, seed=5)
    subs = S.all_subsets(3)
    together = S.forward_subsets(P, spec, xs, cs, combine, eps, subs)
    back = S.forward_subsets(P, spec, xs, cs, combine, eps, subs[::-1])[::-1]
    for s, sub in enumerate(subs):
        alone = S.forward_subsets(P, spec, xs, cs, combine, eps, [sub])[0]
        for m in range(3):
            assert torch.equal(alone["locs"][m], together[s]["locs"][m]), (sub, m)
            assert torch.equal(back[s]["locs"][m], together[s]["locs"][m]), (sub, m)
    # and the subsets differ from each other (the same draw, other posteriors)
    assert not torch.equal(together[0]["locs"][0], together[-1]["locs"][0])


@pytest.mark.parametrize("combine", COMBINERS)
def test_presence_bits_select_the_experts_row_by_row(combine):
    """Rows with present = p under the full subset equal the same rows under subset p; rows with no expert are NaN; the
    squared error of an unobserved modality is NaN while its reconstruction is finite."""
    M = 3
    spec, P, xs, cs, eps = _case(M, seed=6, N=40)
    present = torch.arange(40) % 8
    full = S.forward_subsets(P, spec, xs, cs, combine, eps, [(0, 1, 2)], present=present)[0]
    ex = S.exports(xs, full, present)
    for p in range(1, 8):
        rows = (present == p).nonzero().flatten()
        sub = tuple(i for i in range(M) if (p >> i) & 1)
        want = S.forward_subsets(P, spec, xs, cs, combine, eps, [sub])[0]
        for m in range(M):
            assert torch.allclose(full["locs"][m][rows], want["locs"][m][rows], rtol=1e-6, atol=1e-6), (p, m)
            assert bool(torch.isfinite(ex[m][0][rows]).all())
            assert bool(torch.isnan(ex[m][1][rows]).all()) == (((p >> m) & 1) == 0), (p, m)
            assert bool(torch.isnan(ex[m][2][rows]).all()) == (((p >> m) & 1) == 0), (p, m)
    none = (present == 0).nonzero().flatten()
    for m in range(M):
        assert bool(torch.isnan(ex[m][0][none]).all()) and bool(torch.isnan(ex[m][1][none]).all())
