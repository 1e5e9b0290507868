"""gPoE on a one-expert model without an alpha parameter, bypass off (the shape of the twin fuzz's latent case s4): the
descriptor carries the product of experts (Job.kernel_combine), so no kernel reads the float in front of the parameter
buffer, and every pass gives the bytes of the same job asked for as 'poe'."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import multi_modal_normative_modeling_amd as nm
from multi_modal_normative_modeling_amd import _lib
from tests.twin_cases import assert_same

DEV = "cuda:0"


@pytest.fixture(scope="module")
def pair():
    g = torch.Generator().manual_seed(4)
    N, D, Z, C = 129, 420, 15, 16
    spec = nm.ModelSpec([D], [31, 15], Z, C, False, "single")
    c = torch.zeros(N, C)
    c[torch.arange(N), torch.randint(0, C, (N,), generator=g)] = 1
    tables = [nm.Table(torch.randn(N, D, generator=g) * 1.2, c, DEV)]
    P = nm.ParamLayout(spec).init_reference_rule(7)
    mk = lambda combine: nm.Job(spec, tables, combine=combine, state=P, seed=3, single_bypass=False, n_tiles_ws=tables[0].n_tiles)
    return mk, N


def test_descriptor_carries_the_product_of_experts(pair):
    mk, _ = pair
    d = mk("gpoe").struct()
    assert d.mod[0].alpha == -1 and d.combine == _lib.NM_COMBINE["poe"] and d.single_bypass == 0


def test_every_pass_gives_the_bytes_of_poe(pair):
    mk, N = pair
    out = {}
    for combine in ("gpoe", "poe"):
        a = mk(combine)
        a.enable_exports(loc=True, sqerr=True, rowdev=True, latent=True)
        nm.JobSet([a]).forward()                                      # the general kernel
        b = mk(combine)
        b.enable_exports(loc=False, sqerr=False, rowdev=False, latent=True)
        nm.JobSet([b]).latent(compact=True)                           # the encoder-only kernel
        c = mk(combine)
        c.enable_exports(loc=True, sqerr=True, rowdev=True, latent=False)
        c.enable_predictive_exports(3)
        nm.JobSet([c]).forward_draws()
        d = mk(combine)
        d.enable_likelihood_exports(3, per_modality=True)
        nm.JobSet([d]).forward_loglik()
        torch.cuda.synchronize()
        out[combine] = {"loc": a.out_loc[0].cpu(), "z": a.out_z.cpu(), "mu": a.out_mu.cpu(), "lat_mu": b.out_mu.cpu(),
                        "lat_lv": b.out_logvar.cpu(), "pred_mean": c.pred_mean[0].cpu(), "pred_var": c.pred_var[0].cpu(),
                        "iw_row": d.iw_row.cpu(), "iw_recon_ll": d.iw_recon_ll[0].cpu()}
        for k, t in out[combine].items():
            assert bool(torch.isfinite(t).all()) and float(t[:N].abs().max()) > 0, (combine, k)
        assert torch.equal(out[combine]["mu"][:N], out[combine]["lat_mu"][:N])
    assert_same(out["poe"], out["gpoe"], "gpoe against poe")
