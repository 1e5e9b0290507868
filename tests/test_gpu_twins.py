"""Seeded fuzz of every bit-identical kernel twin over its whole admitted domain (the draw: tests/twin_cases.py, held to its
contract by tests/test_twin_cases_cpu.py).  Each compact form runs next to the generic kernel it must equal, from the same
initial state on the same tables, and the results are compared WITHOUT tolerance:
  plain          train(plain=True) against plain=False: parameters, both Adam moments, bf16 shadow images, loss rows
  split          grads / train(split=True) against one workgroup per model: gradients, then the same as above
  devpass        forward(loss=False) on nm_devpass / nm_devpass_multi against nm_forward: out_loc and out_sqerr of every
  devpass_multi  modality (out_rowdev at rtol 2e-6, atol 1e-9: fp32 summation order, the bound of tests/test_gpu_devpass*.py);
                 rows past the table's end come back as zeros from buffers that held 7.0
  latent         latent(compact=True) on nm_latent_pass against nm_forward with the latent exports: out_mu, out_logvar
The reference is another launch, a case a model of a few thousand parameters and at most 6 steps.  tests/fuzz_many.py --twin
runs the same comparison over more seeds."""
import ctypes as C
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

import multi_modal_normative_modeling_amd as nm
from multi_modal_normative_modeling_amd import _lib
from tests import twin_cases as T
from tests.twin_cases import assert_same

DEV = "cuda:0"
LOSS_CAP = 8


def _onehot(gen, B, c_dim):
    c = torch.zeros(B, c_dim)
    c[torch.arange(B), torch.randint(0, c_dim - 2, (B,), generator=gen)] = 1
    c[torch.arange(B), c_dim - 2 + torch.randint(0, 2, (B,), generator=gen)] = 1
    return c


class Built:
    """The data of one case, built once and shared by both forms: tables, injected draws, reference-rule weights."""

    def __init__(self, cs):
        gen = torch.Generator().manual_seed(cs.data_seed)
        self.cs = cs
        self.spec = nm.ModelSpec(list(cs.dims), list(cs.hidden), cs.Z, cs.c_dim, cs.non_linear, cs.kind)
        self.P = nm.ParamLayout(self.spec).init_reference_rule(cs.init_seed)
        xs = [torch.randn(cs.N, d, generator=gen) * 1.2 for d in cs.dims]
        c0 = _onehot(gen, cs.N, cs.c_dim)
        covs = [c0] * cs.M if cs.shared_cov else [c0] + [_onehot(gen, cs.N, cs.c_dim) for _ in range(cs.M - 1)]
        self.tables = [nm.Table(x, c, DEV) for x, c in zip(xs, covs)]
        self.n_tiles = self.tables[0].n_tiles
        n_eps = 3 if cs.twin in T.TRAINING else self.n_tiles          # (training: a ring shorter than the steps taken)
        self.eps = torch.randn(n_eps, 256, cs.Z, generator=gen) if cs.inject else None

    def job(self, exports=None, fill=None):
        """exports: None (a training job), "mod" (out_loc / out_sqerr / out_rowdev) or "latent"; fill: what the export
        buffers hold before the launch."""
        cs = self.cs
        job = nm.Job(self.spec, self.tables, combine=cs.combine, state=self.P, lr=cs.lr, betas=cs.betas, adam_eps=cs.adam_eps,
                     kl_weight=cs.kl_weight, ll_weight=cs.ll_weight, seed=cs.job_seed, loss_cap=LOSS_CAP,
                     single_bypass=cs.single_bypass, n_tiles_ws=1 if exports is None else self.n_tiles)
        job.set_eps(self.eps)                                       # (None: the in-kernel draw, keyed by (seed, step, row, z))
        if cs.lr_table is not None:
            job.set_lr_table(cs.lr_table)
        if exports is not None:
            job.enable_exports(loc=exports == "mod", sqerr=exports == "mod", rowdev=exports == "mod", latent=exports == "latent")
            bufs = [job.out_mu, job.out_logvar] if exports == "latent" else job.out_loc + job.out_sqerr + job.out_rowdev
            if fill is not None:
                for t in bufs:
                    t.fill_(fill)
        return job


@functools.lru_cache(maxsize=8)
def built(cs):
    return Built(cs)


def _entries(js):
    """Record the C entry points the set's launches go through."""
    seen, real = [], js._issue
    js._issue = lambda entry, *a: (seen.append(entry), real(entry, *a))[1]
    return seen


def snapshot(job, n_rows):
    torch.cuda.synchronize()
    return {"params": job.params.cpu().clone(), "adam_m": job.adam_m.cpu().clone(), "adam_v": job.adam_v.cpu().clone(),
            "wsh": job._wsh.cpu().clone(), "loss_log": job.loss_log[:n_rows].cpu().clone()}


def _trained(snap, start, what):
    rows = snap["loss_log"]
    assert bool(torch.isfinite(rows).all()) and bool((rows[:, 0] != 0).all()), (what, rows[:, 0])      # (column 0: the step's total)
    assert not torch.equal(snap["params"], start), what             # (it trained)


def train_plain(jobs, launches, plain):
    js = nm.JobSet(jobs)
    for n in launches:
        js.train(n, plain=plain, split=False, rowsplit=1)
        assert js.last_launch["plain"] == plain and js.last_launch["entry"] == "nm_launch"
        assert bool(js.last_launch["flags"] & _lib.NM_F_PLAIN) == plain
    js.check_split_errors(block=True)


def train_split(jobs, launches, split):
    js = nm.JobSet(jobs)
    for n in launches:
        if split:
            js.train(n, split=True)
            assert js.last_launch["entry"] == "split" and not js.last_launch["plain"]
        else:
            js.train(n, split=False, rowsplit=1, plain=False)
            assert js.last_launch["entry"] == "nm_launch" and not js.last_launch["plain"]
    js.check_split_errors(block=True)


def run_plain(cs):
    b = built(cs)
    a, g = b.job(), b.job()
    assert a.plain_ok() and _lib.load().nm_plain_ok(C.byref(a.struct())) == 0
    start = a.params.cpu().clone()
    train_plain([a], cs.steps, True)
    train_plain([g], cs.steps, False)
    sa, sg = snapshot(a, sum(cs.steps)), snapshot(g, sum(cs.steps))
    assert_same(sg, sa, cs.id)
    _trained(sa, start, cs.id)


def run_split(cs):
    b = built(cs)
    a, g = b.job(), b.job()
    start = a.params.cpu().clone()
    res = []
    for job, split in ((g, False), (a, True)):
        js = nm.JobSet([job])
        assert js.split_parts() == cs.M
        js.grads(0, export=False, split=split)
        assert js.last_launch["entry"] == ("split" if split else "nm_launch")
        js.check_split_errors(block=True)
        torch.cuda.synchronize()
        res.append({"grads": job.grads.cpu().clone(), "loss_log": job.loss_log[:1].cpu().clone()})
    assert_same(res[0], res[1], cs.id + " gradients")
    assert float(res[1]["grads"].abs().max()) > 0 and float(res[1]["loss_log"][0, 0]) != 0
    train_split([a], cs.steps, True)
    train_split([g], cs.steps, False)
    sa, sg = snapshot(a, sum(cs.steps)), snapshot(g, sum(cs.steps))
    assert_same(sg, sa, cs.id)
    _trained(sa, start, cs.id)


def run_devpass(cs):
    b = built(cs)
    N, multi = cs.N, cs.twin == "devpass_multi"
    gen, cmp_ = b.job("mod"), b.job("mod", fill=7.0)
    js = nm.JobSet([gen])
    seen = _entries(js)
    js.forward()                                                    # the general kernel
    assert seen == ["nm_launch"]
    js = nm.JobSet([cmp_])
    lib_ok = _lib.load().nm_devpass_multi_ok if multi else _lib.load().nm_devpass_ok
    assert js.devpass_ok() != multi and js.devpass_multi_ok() == multi and lib_ok(C.byref(cmp_.struct())) == 0
    seen = _entries(js)
    js.forward(loss=False, compact=True)
    assert seen == ["nm_devpass_multi" if multi else "nm_devpass"]
    torch.cuda.synchronize()
    exact = lambda j: {f"{k}[{m}]": t[m].cpu() for k, t in (("out_loc", j.out_loc), ("out_sqerr", j.out_sqerr)) for m in range(cs.M)}
    assert_same(exact(gen), exact(cmp_), cs.id)
    for m in range(cs.M):
        rd_g, rd_c = gen.out_rowdev[m].cpu(), cmp_.out_rowdev[m].cpu()
        assert torch.allclose(rd_g[:N], rd_c[:N], rtol=2e-6, atol=1e-9), (cs.id, m, "out_rowdev", float((rd_g[:N] - rd_c[:N]).abs().max()))
        for what, t in (("out_loc", cmp_.out_loc[m]), ("out_sqerr", cmp_.out_sqerr[m]), ("out_rowdev", cmp_.out_rowdev[m])):
            t = t.cpu()
            assert float(t[:N].abs().max()) > 0, (cs.id, m, what)
            if t.shape[0] > N:                                       # rows past the table: zeros, not the 7.0
                assert float(t[N:].abs().max()) == 0.0, (cs.id, m, what, int((t[N:] != 0).sum()))


def run_latent(cs):
    b = built(cs)
    N = cs.N
    gen, cmp_ = b.job("latent"), b.job("latent", fill=7.0)
    js = nm.JobSet([gen])
    seen = _entries(js)
    js.forward()                                                    # the general kernel with the latent exports
    assert seen == ["nm_launch"]
    js = nm.JobSet([cmp_])
    assert js.latent_ok() and _lib.load().nm_latent_pass_ok(C.byref(cmp_.struct())) == 0
    seen = _entries(js)
    js.latent(compact=True)
    assert seen == ["nm_latent_pass"]
    torch.cuda.synchronize()
    live = lambda j: {"out_mu": j.out_mu[:N].cpu(), "out_logvar": j.out_logvar[:N].cpu()}
    assert_same(live(gen), live(cmp_), cs.id)
    for what, t in (("out_mu", cmp_.out_mu.cpu()), ("out_logvar", cmp_.out_logvar.cpu())):
        assert float(t[:N].abs().max()) > 0, (cs.id, what)
        assert t.shape[0] >= N and float(t[N:].abs().max() if t.shape[0] > N else 0.0) == 0.0, (cs.id, what)


RUN = {"plain": run_plain, "split": run_split, "devpass": run_devpass, "devpass_multi": run_devpass, "latent": run_latent}


def run(cs):
    RUN[cs.twin](cs)


_ids = lambda cs: cs.name


@pytest.mark.parametrize("cs", T.cases("plain"), ids=_ids)
def test_plain_equals_generic(cs):
    run(cs)


@pytest.mark.parametrize("cs", T.cases("split"), ids=_ids)
def test_split_equals_single_workgroup(cs):
    run(cs)


@pytest.mark.parametrize("cs", T.cases("devpass"), ids=_ids)
def test_devpass_equals_general_forward(cs):
    run(cs)


@pytest.mark.parametrize("cs", T.cases("devpass_multi"), ids=_ids)
def test_devpass_multi_equals_general_forward(cs):
    run(cs)


@pytest.mark.parametrize("cs", T.cases("latent"), ids=_ids)
def test_latent_pass_equals_general_forward(cs):
    run(cs)


def _set_of_six(cases, train):
    """Six jobs of different shapes in ONE launch of the compact form, each against the same job launched alone."""
    assert len(cases) == 6 and len({(c.dims, c.hidden, c.Z) for c in cases}) == 6
    launches = (2, 3)                                               # (jobs of one set take the same steps)
    together = [built(c).job() for c in cases]
    train(together, launches, True)
    for c, jt in zip(cases, together):
        alone = built(c).job()
        start = alone.params.cpu().clone()
        train([alone], launches, True)
        st = snapshot(jt, sum(launches))
        assert_same(snapshot(alone, sum(launches)), st, f"{c.id} in a set of six")
        _trained(st, start, c.id)


def test_plain_set_of_six_shapes_equals_each_alone():
    """Seeds 0..5 of the plain draw -- M = 1, 2, 3, 4, 1, 2: JobSet and nm_launch take a set whose models differ in their number
    of modalities on this form (one workgroup per job, every job reads its own descriptor; only the split and the
    equal-count row-split launches ask for one M) -- with their own shapes, tables, knobs and learning-rate tables."""
    cases = [T.draw("plain", s) for s in range(6)]
    assert len({c.M for c in cases}) == 4
    _set_of_six(cases, train_plain)


def test_split_set_of_six_shapes_equals_each_alone():
    """Six two-modality models of the split draw (split_parts() wants one M per set): 6 x 2 workgroups, padded to 16."""
    cases = [c for c in (T.draw("split", s) for s in T.SEEDS["split"]) if c.M == 2][:6]
    _set_of_six(cases, train_split)
