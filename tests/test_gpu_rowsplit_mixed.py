"""The mixed row-split launch (nm_launch_rowsplit_mixed): models that differ in their number of modalities -- the reference's
grid is 5 folds x {SM-T1w_sMRI, SM-T2w_sMRI, SM-fMRI, UCA-gPoE}, 15 one-modality and 5 four-modality models
(commands_list_deviation.sh:13-23) -- as ONE launch whose groups come from a per-job map.

Every comparison is bit for bit: the row-split arithmetic of a parameter (the k partials summed in slice order, Adam) does
not depend on which other groups share the launch, on the helpers, or on where in the set a model stands.  The single-model
row-split launch itself is held to the oracle and the reference's goldens by tests/test_gpu_rowsplit.py; nothing here is
compared with a tolerance."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

import multi_modal_normative_modeling_amd as nm
from multi_modal_normative_modeling_amd import _lib, prep, sweep
from tests.golden_util import Golden
from tests.hip_harness import DEV

NAMES = ["mm1_small", "mm3_gpoe", "mm4_uca_gpoe", "mm2_z64"]           # 1, 3, 4 and 2 modalities
TRAIN = _lib.NM_F_BACKWARD | _lib.NM_F_ADAM
N_STEPS = 7


@pytest.fixture(scope="module", autouse=True)
def mixed_lib():
    """Without the entry point nothing below may launch: a mixed set must never reach nm_launch_rowsplit, whose one M for
    the whole launch maps its workgroups wrongly."""
    lib = _lib.load()
    assert hasattr(lib, "nm_launch_rowsplit_mixed"), "libnmhip.so has no nm_launch_rowsplit_mixed"
    assert hasattr(lib, "nm_rowsplit_groups"), "libnmhip.so has no nm_rowsplit_groups"
    return lib


class Shape:
    """A golden case's shapes and weights on a seeded n_rows table (several batches, ragged tail); the jobs of one shape
    share its tables and differ in the seed of the in-kernel draw."""

    def __init__(self, name, n_rows=600, seed=5):
        g = Golden(name)
        gen = torch.Generator().manual_seed(seed)
        xs = [torch.randn(n_rows, d, generator=gen) for d in g.dims]
        c = torch.zeros(n_rows, g.c_dim)
        c[torch.arange(n_rows), torch.randint(0, g.c_dim, (n_rows,), generator=gen)] = 1
        self.spec = nm.ModelSpec(g.dims, g.hidden, g.Z, g.c_dim)
        self.tables = [nm.Table(x, c, DEV) for x in xs]
        self.combine, self.state, self.M = g.combine, g.weights("w0"), g.M

    def job(self, seed):
        j = nm.Job(self.spec, self.tables, combine=self.combine, state=self.state)
        j.seed = seed
        j.set_eps(None)                                       # in-kernel draw, keyed by (seed, step, row, z)
        return j


@pytest.fixture(scope="module")
def shapes(mixed_lib):
    return {n: Shape(n) for n in NAMES}


# the mixed set: two of each shape, distinct seeds -- (shape, seed) in set order; 20 groups -> 24 slots
SET = [(n, 10 * i + r) for r in range(2) for i, n in enumerate(NAMES)]
PERM = [5, 0, 7, 2, 4, 1, 6, 3]


def _jobs(shapes, order=None):
    items = SET if order is None else [SET[i] for i in order]
    return [shapes[n].job(seed) for n, seed in items]


def _snap(job, n=N_STEPS):
    torch.cuda.synchronize()
    return (job.params.cpu().clone(), job.adam_m.cpu().clone(), job.adam_v.cpu().clone(), job.loss_log[:n].cpu().clone())


def _same(a, b, what):
    for x, y, t in zip(a, b, ("params", "adam_m", "adam_v", "loss_log")):
        assert torch.equal(x, y), (what, t, float((x - y).abs().max()))


def _sync(js):
    js.check_split_errors(block=True)
    torch.cuda.synchronize()


_ALONE = {}


def _alone(shapes, k, n_steps=N_STEPS):
    """Every model of SET trained alone with rowsplit=k (once per k)."""
    if (k, n_steps) not in _ALONE:
        res = []
        for n, seed in SET:
            j = shapes[n].job(seed)
            js = nm.JobSet([j])
            js.train(n_steps, rowsplit=k)
            _sync(js)
            res.append(_snap(j, n_steps))
        _ALONE[(k, n_steps)] = res
    return _ALONE[(k, n_steps)]


@pytest.mark.parametrize("k", [2, 4])
def test_each_model_gets_what_it_gets_alone(mixed_lib, shapes, k):
    """7 steps over 600-row tables in one mixed launch: parameters, both moments and the loss rows of every model equal the
    same model trained alone with rowsplit=k; whatever the helpers, and in a permuted job order."""
    alone = _alone(shapes, k)
    assert not torch.equal(alone[0][0], alone[4][0])          # (the seeds do tell the two models of a shape apart)
    for helpers in (None, 0, 3):
        jobs = _jobs(shapes)
        js = nm.JobSet(jobs)
        assert js.rowsplit_k() == 1 and js.rowsplit_k(mixed=True) == 4
        js.train(N_STEPS, rowsplit=k, helpers=helpers)
        _sync(js)
        js.assert_finite()
        for i, j in enumerate(jobs):
            _same(_snap(j), alone[i], (k, helpers, i, SET[i]))
    jobs = _jobs(shapes, PERM)
    js = nm.JobSet(jobs)
    js.train(N_STEPS, rowsplit=k)
    _sync(js)
    for pos, i in enumerate(PERM):
        _same(_snap(jobs[pos]), alone[i], (k, "permuted", pos, SET[i]))


@pytest.mark.parametrize("k", [2, 4])
def test_one_launch_equals_stepwise_and_run_again(mixed_lib, shapes, k):
    res = []
    for mode in ("fused", "stepwise", "fused"):
        jobs = _jobs(shapes)
        js = nm.JobSet(jobs)
        if mode == "stepwise":
            for _ in range(N_STEPS):
                js.train(1, rowsplit=k)
        else:
            js.train(N_STEPS, rowsplit=k)
        _sync(js)
        res.append([_snap(j) for j in jobs])
    for i in range(len(SET)):
        _same(res[0][i], res[1][i], (k, "stepwise", i))
        _same(res[0][i], res[2][i], (k, "second run", i))


UNWRITTEN = 12345.0


@pytest.mark.parametrize("k", [2, 4])
def test_gradients_through_the_mixed_launch(mixed_lib, shapes, k):
    """js.grads(0, rowsplit=k) on the mixed set == every model's own grads(0, rowsplit=k), tensor by tensor and in the loss
    row.  The gradient buffers start at a marker: what a launch does not write (the flat buffer's padding; alpha of a
    one-modality model, which has no gPoE weighting) is unwritten in both, everything else is written in both."""
    jobs = _jobs(shapes)
    for j in jobs:
        j.grads.fill_(UNWRITTEN)
    js = nm.JobSet(jobs)
    js.grads(0, export=False, rowsplit=k)
    _sync(js)
    for i, (n, seed) in enumerate(SET):
        one = shapes[n].job(seed)
        one.grads.fill_(UNWRITTEN)
        s1 = nm.JobSet([one])
        s1.grads(0, export=False, rowsplit=k)
        _sync(s1)
        got, want = jobs[i].grads_dict(), one.grads_dict()
        assert got.keys() == want.keys() and len(want) > 0
        for key, w in want.items():
            assert bool(torch.isfinite(w).all()), (k, i, key)
            assert torch.equal(got[key], w), (k, i, SET[i], key)
            assert "alpha" in key or not bool((w == UNWRITTEN).any()), (k, i, key)
        assert torch.equal(jobs[i].loss_log[0].cpu(), one.loss_log[0].cpu()), (k, i, SET[i])
        assert torch.equal(jobs[i].params.cpu(), one.params.cpu())               # (no update)


def test_the_grid_at_size(mixed_lib):
    """15 models of D = [379] and 5 of D = [379, 379, 379, 1137], H = [110, 110], Z = 10, 600-row tables: 35 groups ->
    40 x 4 = 160 workgroups (+ 2 helpers per group), 3 steps in one launch; one SM and one UCA model equal their
    alone-runs."""
    gen = torch.Generator().manual_seed(21)
    n_rows, c_dim = 600, 29
    c = torch.zeros(n_rows, c_dim)
    c[torch.arange(n_rows), torch.randint(0, c_dim - 2, (n_rows,), generator=gen)] = 1
    c[torch.arange(n_rows), c_dim - 2 + torch.randint(0, 2, (n_rows,), generator=gen)] = 1
    made = {}
    for tag, dims in (("sm", [379]), ("uca", [379, 379, 379, 1137])):
        spec = nm.ModelSpec(dims, [110, 110], 10, c_dim, True)
        made[tag] = (spec, [nm.Table(torch.randn(n_rows, d, generator=gen) * 1.2, c, DEV) for d in dims],
                     nm.ParamLayout(spec).init_reference_rule(3 + len(dims)))

    def job(tag, seed):
        spec, tables, P = made[tag]
        j = nm.Job(spec, tables, combine="gpoe", state=P)
        j.seed = seed
        j.set_eps(None)
        return j

    items = [("sm", i) for i in range(15)] + [("uca", 100 + i) for i in range(5)]
    jobs = [job(t, s) for t, s in items]
    js = nm.JobSet(jobs)
    assert js.rowsplit_k() == 1
    assert js.rowsplit_k(mixed=True) == 4 and js.rowsplit_helpers(4) == 2
    js.train(3, rowsplit=4)
    js.check_split_errors(block=True)
    js.assert_finite()
    for i in (6, 17):
        one = job(*items[i])
        s1 = nm.JobSet([one])
        s1.train(3, rowsplit=4)
        _sync(s1)
        _same(_snap(jobs[i], 3), _snap(one, 3), ("grid", i, items[i]))
    assert not torch.equal(jobs[6].params.cpu(), jobs[7].params.cpu())
    assert not torch.equal(jobs[17].params.cpu(), jobs[18].params.cpu())


def _direct(mixed_lib, jobs, k, counts=None, M=None, helpers=0, n_steps=N_STEPS):
    """A row-split launch through the C entry points themselves; returns (status, the set)."""
    js = nm.JobSet(jobs)
    for j in jobs:
        j._ensure_rowsplit(k)
    ptr = js._upload(k)
    st = torch.cuda.current_stream().cuda_stream
    if M is not None:
        return mixed_lib.nm_launch_rowsplit(ptr, len(jobs), M, k, helpers, 0, n_steps, TRAIN, 0, st), js
    arr = (C.c_int * len(counts))(*counts)
    return mixed_lib.nm_launch_rowsplit_mixed(ptr, len(counts), arr, k, helpers, 0, n_steps, TRAIN, 0, st), js


def _error_words(mixed_lib, js, n):
    out = torch.full((n,), -1, dtype=torch.int32, device=DEV)
    st = torch.cuda.current_stream().cuda_stream
    assert mixed_lib.nm_split_errors(js._dev.data_ptr(), n, out.data_ptr(), 1, st) == 0
    torch.cuda.synchronize()
    return out.tolist()


@pytest.mark.parametrize("k", [2, 4])
def test_uniform_set_through_the_mixed_entry(mixed_lib, shapes, k):
    """job_M_host = [3, 3, 3] == nm_launch_rowsplit(..., M = 3, ...), bit for bit."""
    res = []
    for how in ("mixed", "uniform"):
        jobs = [shapes["mm3_gpoe"].job(s) for s in (1, 2, 3)]
        status, js = _direct(mixed_lib, jobs, k, counts=[3, 3, 3]) if how == "mixed" else _direct(mixed_lib, jobs, k, M=3)
        assert status == 0, (how, status)
        assert _error_words(mixed_lib, js, 3) == [0, 0, 0]
        res.append([_snap(j) for j in jobs])
    for i in range(3):
        _same(res[0][i], res[1][i], (k, i))
    assert not torch.equal(res[0][0][0], res[0][1][0])


def test_residency_refusals(mixed_lib):
    """130 groups at k = 2 (136 slots: beyond any map, and 272 workgroups beyond the chip) and 120 groups at k = 4 (480
    workgroups) come back NM_E_RESIDENCY before anything is launched."""
    small = {n: Shape(n, n_rows=19) for n in ("mm1_small", "mm4_uca_gpoe")}
    jobs = [small["mm4_uca_gpoe"].job(i) for i in range(30)] + [small["mm1_small"].job(100 + i) for i in range(10)]
    before = [j.params.clone() for j in jobs]
    counts = [4] * 30 + [1] * 10
    assert sum(counts) == 130
    status, js = _direct(mixed_lib, jobs, 2, counts=counts, n_steps=1)
    assert status == _lib.NM_E_RESIDENCY
    assert js.rowsplit_k(mixed=True) == 1
    status, _ = _direct(mixed_lib, jobs[:30], 4, counts=counts[:30], n_steps=1)
    assert status == _lib.NM_E_RESIDENCY
    torch.cuda.synchronize()
    assert all(torch.equal(j.params, b) for j, b in zip(jobs, before))


@pytest.mark.parametrize("listed", [2, 4])
def test_job_listed_with_a_wrong_modality_count_is_refused(mixed_lib, shapes, listed):
    """A 3-modality job listed with 2 (fewer groups than it has parts) or 4 (a group too many): every workgroup the map
    gives that job leaves before its first hand-off -- no time-out -- with NM_SYNC_ERR_SHAPE in the job's error word; its
    parameters stay as they were, the other jobs of the launch train and equal their alone-runs."""
    k = 4
    alone = _alone(shapes, k)
    pick = [0, 1, 3]                                          # mm1_small, mm3_gpoe, mm2_z64
    jobs = [shapes[SET[i][0]].job(SET[i][1]) for i in pick]
    before = (jobs[1].params.cpu().clone(), jobs[1].adam_m.cpu().clone(), jobs[1].adam_v.cpu().clone())
    status, js = _direct(mixed_lib, jobs, k, counts=[1, listed, 2])
    assert status == 0                                        # (the kernel cannot fail the stream)
    if listed == 2:
        assert _error_words(mixed_lib, js, 3) == [0, _lib.NM_SYNC_ERR_SHAPE, 0]
    else:                                                     # the host path: the words surface as NmError
        js._split_pending = True
        js._pending_kinds.add("rowsplit")
        with pytest.raises(_lib.NmError, match=r"job\(s\) \[1\]"):
            js.check_split_errors(block=True)
    torch.cuda.synchronize()
    for got, was in zip((jobs[1].params, jobs[1].adam_m, jobs[1].adam_v), before):
        assert torch.equal(got.cpu(), was)
    _same(_snap(jobs[0]), alone[0], (listed, "job 0"))
    _same(_snap(jobs[2]), alone[3], (listed, "job 2"))


def test_sweep_one_launch(mixed_lib):
    """run_cells on SM-T1w_sMRI, SM-fMRI and UCA-gPoE cells (folds 0 and 1): one launch and shape group after shape group
    give the same metric rows in every column but the rate; a model family that cannot run row-split refuses one_launch=True."""
    cohort = prep.synthetic_cohort(n=320, d=379)
    cells = [c for c in sweep.plan_cells(["SM-T1w_sMRI", "SM-fMRI", "UCA-gPoE"], 5) if c.fold in (0, 1)]
    assert len(cells) == 6
    one = sweep.run_cells(cohort, cells, 5, epochs=4, device=DEV, one_launch=True)
    grouped = sweep.run_cells(cohort, cells, 5, epochs=4, device=DEV, one_launch=False)
    auto = sweep.run_cells(cohort, cells, 5, epochs=4, device=DEV)
    rate = list(sweep.METRIC_COLUMNS).index("steps_per_s")
    keep = [i for i in range(sweep.N_METRICS) if i != rate]
    assert one.shape == grouped.shape == (6, sweep.N_METRICS)
    assert bool(torch.isfinite(one).all())
    assert torch.equal(one[:, keep], grouped[:, keep])
    assert torch.equal(auto[:, keep], grouped[:, keep])
    # (-Model mvtCAE on SE cells, as tests/test_gpu_api_sweep.py trains it: not a model the row-split kernel holds)
    zoo = [c for c in sweep.plan_cells(["SE-PoE"], 5) if c.fold in (0, 1)]
    with pytest.raises(ValueError, match="one_launch=True"):
        sweep.run_cells(cohort, zoo, 5, epochs=4, device=DEV, one_launch=True, model="mvtCAE")
    assert sweep.run_cells(cohort, zoo, 5, epochs=2, device=DEV, model="mvtCAE").shape == (2, sweep.N_METRICS)
