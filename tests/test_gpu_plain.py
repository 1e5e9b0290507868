"""The step kernel's plain-training instantiation (NM_F_PLAIN, nm_step_kernel<false, 0, true>) against the generic one, its
oracle: the same jobs trained twice from the same initial state, plain=True and plain=False, must agree BIT FOR BIT --
parameters, both Adam moments, the bf16 shadow images and every loss row.  No tolerance: the plain kernel folds launch
constants and scalar bookkeeping, the arithmetic is the generic kernel's operation by operation.

Shapes: the smallest that reach every branch the plain code touches (see CASES)."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

import multi_modal_normative_modeling_amd as nm
from multi_modal_normative_modeling_amd import _lib
from tests.hip_harness import DEV


def _onehot(gen, B, c_dim):
    c = torch.zeros(B, c_dim)
    c[torch.arange(B), torch.randint(0, c_dim - 2, (B,), generator=gen)] = 1
    c[torch.arange(B), c_dim - 2 + torch.randint(0, 2, (B,), generator=gen)] = 1
    return c


class Case:
    """Seeded data of one model shape: tables (shared by every job of the case), draws, reference-rule weights."""

    def __init__(self, dims, hidden, Z, c_dim, n_rows, combine, inject, seed=0):
        gen = torch.Generator().manual_seed(seed)
        self.spec = nm.ModelSpec(list(dims), list(hidden), Z, c_dim, True)
        self.P = nm.ParamLayout(self.spec).init_reference_rule(seed)
        self.combine = combine
        xs = [torch.randn(n_rows, d, generator=gen) * 1.2 for d in dims]
        c = _onehot(gen, n_rows, c_dim)
        self.eps = torch.randn(3, 256, Z, generator=gen) if inject else None
        self.tables = [nm.Table(x, c, DEV) for x in xs]

    def job(self, seed=11):
        j = nm.Job(self.spec, self.tables, combine=self.combine, state=self.P, seed=seed, loss_cap=8)
        j.set_eps(self.eps)                               # (None: the in-kernel draw, keyed by (seed, step, row, z))
        return j


# name: (dims, hidden, Z, c_dim, rows, combine, injected eps, steps)
D3 = (70, 17, 33)
CASES = {
    # full and partial output chunks (70 = 64 + 6), a full and a ragged batch (256 + 44 rows), edge n tiles (24 = 16 + 8), a
    # weight-gradient pass of exactly one k tile with its filler tile (Z + C + 1 = 16), odd pair counts, the epoch wrap (step 2)
    "a_gpoe_draw": (D3, [24, 18], 10, 5, 300, "gpoe", False, 5),
    "b_poe_z8_eps": (D3, [24, 18], 8, 5, 300, "poe", True, 5),              # the four-column latent path, injected eps
    "c_single_h1": ((130,), [20], 10, 5, 256, "gpoe", False, 3),            # single-expert bypass, L = 1, a last chunk of 2 columns
    "d_mopoe_l3": (D3, [40, 24, 17], 10, 5, 300, "mopoe", False, 3),        # L = 3, the other combiners
    "d_moe_l3": (D3, [40, 24, 17], 10, 5, 300, "moe", False, 3),
    "e_metric": ((379, 379, 379), [110, 110], 10, 29, 256, "gpoe", False, 2),   # the benchmark's shape, once
}
_cases = {}


def case(name):
    if name not in _cases:
        dims, hidden, Z, c_dim, rows, combine, inject, _ = CASES[name]
        _cases[name] = Case(dims, hidden, Z, c_dim, rows, combine, inject)
    return _cases[name]


def snapshot(job):
    torch.cuda.synchronize()
    return {"params": job.params.cpu().clone(), "adam_m": job.adam_m.cpu().clone(), "adam_v": job.adam_v.cpu().clone(),
            "wsh": job._wsh.cpu().clone(), "loss_log": job.loss_log.cpu().clone()}


def assert_same(a, b, what):
    for k in a:
        assert torch.equal(a[k], b[k]), (what, k, int((a[k] != b[k]).sum()))


def train(jobs, n_steps, plain, launches=1):
    js = nm.JobSet(jobs)
    for _ in range(launches):
        js.train(n_steps, plain=plain, split=False, rowsplit=1)
        assert js.last_launch["plain"] == plain and js.last_launch["entry"] == "nm_launch"
        assert bool(js.last_launch["flags"] & _lib.NM_F_PLAIN) == plain
    js.check_split_errors(block=True)
    return js


@pytest.mark.parametrize("name", list(CASES))
def test_plain_equals_generic_bit_for_bit(name):
    cs, n = case(name), CASES[name][-1]
    a, b = cs.job(), cs.job()
    assert a.plain_ok() and _lib.load().nm_plain_ok(C.byref(a.struct())) == 0
    train([a], n, True)
    train([b], n, False)
    sa, sb = snapshot(a), snapshot(b)
    assert_same(sa, sb, name)
    rows = sa["loss_log"][:n]
    assert bool(torch.isfinite(rows).all()) and bool((rows[:, 0] != 0).all())      # (column 0: the step's total)
    assert not torch.equal(sa["params"], cs.job().params.cpu())   # (it trained)


def test_plain_second_launch_continues_the_first():
    """Two launches of 2 + 3 steps (the second starts mid-epoch on the ragged batch) against the generic kernel."""
    cs = case("a_gpoe_draw")
    a, b = cs.job(), cs.job()
    ja, jb = nm.JobSet([a]), nm.JobSet([b])
    for n in (2, 3):
        ja.train(n, plain=True, split=False, rowsplit=1)
        jb.train(n, plain=False, split=False, rowsplit=1)
    ja.check_split_errors(block=True)
    assert_same(snapshot(a), snapshot(b), "2 + 3 steps")


def test_plain_set_of_eight_equals_each_alone():
    """8 models of case (a) with their own draws in ONE plain launch: each equals the same model trained alone."""
    cs = case("a_gpoe_draw")
    jobs = [cs.job(seed=100 + i) for i in range(8)]
    js = train(jobs, 5, True)
    assert js.last_launch["plain"]
    alone = [cs.job(seed=100 + i) for i in (0, 3, 7)]
    for j in alone:
        train([j], 5, True)
    for i, j in zip((0, 3, 7), alone):
        assert_same(snapshot(jobs[i]), snapshot(j), f"job {i}")
    assert not torch.equal(jobs[0].params.cpu(), jobs[1].params.cpu())


def _regression_job():
    g = torch.Generator().manual_seed(5)
    dims, rows = [70, 17, 33], 256
    xes = [torch.randn(rows, d, generator=g) for d in dims]
    c = torch.rand(rows, 2, generator=g)
    spec = nm.ModelSpec(dims, [24, 18], 10, 2, True, "regression")
    job = nm.Job(spec, [nm.Table(x, c, DEV) for x in xes], combine="gpoe", seed=3, loss_cap=8)
    job.set_fi(torch.randn(rows, generator=g) * 0.5 + 1.0)
    return job


def test_kernel_guard_for_c_abi_callers():
    """A C-ABI caller that sets NM_F_PLAIN on a job nm_plain_ok refuses (a regression model): the kernel sets the job's error
    word and leaves before touching anything; JobSet surfaces it as NmError."""
    lib = _lib.load()
    job = _regression_job()
    js = nm.JobSet([job])
    assert not job.plain_ok() and lib.nm_plain_ok(C.byref(job.struct())) == 1 and not js.plain_pick()
    ptr = js._upload(1)
    torch.cuda.synchronize()
    before = snapshot(job)
    st = torch.cuda.current_stream().cuda_stream
    flags = _lib.NM_F_BACKWARD | _lib.NM_F_ADAM | _lib.NM_F_PLAIN
    assert lib.nm_launch(ptr, 1, 0, 2, 1, flags, st) == 0
    js._split_pending = True
    js._pending_kinds.add("plain")
    torch.cuda.synchronize()
    err = torch.zeros(1, dtype=torch.int32, device=DEV)
    assert lib.nm_split_errors(ptr, 1, err.data_ptr(), 0, st) == 0
    torch.cuda.synchronize()
    assert int(err.item()) == _lib.NM_SYNC_ERR_PLAIN
    with pytest.raises(nm.NmError, match="refused by the kernel"):
        js.check_split_errors(block=True)
    assert_same(before, snapshot(job), "refused job")
    js.check_split_errors(block=True)                     # read and cleared
    # the flag is ignored where it does not apply: a gradient launch with it is the generic kernel's, nothing refused
    assert lib.nm_launch(ptr, 1, 0, 1, 1, _lib.NM_F_BACKWARD | _lib.NM_F_GRADS | _lib.NM_F_PLAIN, st) == 0
    js._split_pending = True
    js.check_split_errors(block=True)
    with pytest.raises(ValueError, match="plain=True"):
        js.train(1, plain=True, split=False, rowsplit=1)


def test_pick(monkeypatch):
    """The automatic pick: every job eligible -> the plain kernel; one ineligible job (export buffers set) or NMHIP_PLAIN=0
    -> the generic one; launches that are not plain training (gradients, forward) never carry the flag."""
    monkeypatch.delenv("NMHIP_PLAIN", raising=False)
    cs = case("a_gpoe_draw")
    jobs = [cs.job(seed=i) for i in range(2)]
    js = nm.JobSet(jobs)
    js.train(1, split=False, rowsplit=1)
    assert js.last_launch["plain"] and js.last_launch["flags"] & _lib.NM_F_PLAIN
    js.grads(split=False, rowsplit=1)
    assert not js.last_launch["plain"] and not js.last_launch["flags"] & _lib.NM_F_PLAIN
    monkeypatch.setenv("NMHIP_PLAIN", "0")
    js.train(1, split=False, rowsplit=1)
    assert not js.last_launch["plain"]
    monkeypatch.delenv("NMHIP_PLAIN")
    js.train(1, split=False, rowsplit=1)
    assert js.last_launch["plain"]
    jobs[1].enable_exports()
    assert not jobs[1].plain_ok() and _lib.load().nm_plain_ok(C.byref(jobs[1].struct())) == 1
    js.train(1, split=False, rowsplit=1)
    assert not js.last_launch["plain"] and not js.last_launch["flags"] & _lib.NM_F_PLAIN
    js.check_split_errors(block=True)
    js.assert_finite()
    # ... and the mixed history (plain and generic launches interleaved) equals the generic kernel throughout
    ref = cs.job(seed=0)
    rs = nm.JobSet([ref])
    for _ in range(4):
        rs.train(1, plain=False, split=False, rowsplit=1)
    a, b = snapshot(jobs[0]), snapshot(ref)
    for k in ("params", "adam_m", "adam_v", "wsh"):
        assert torch.equal(a[k], b[k]), k
