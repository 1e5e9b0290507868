"""nm_auc_bootstrap on the device against the yardstick tests/auc_bootstrap_ref.py.  roc_auc, ci_lo, ci_hi, the counts, p_boot,
delta_auc and every A2* of boot_out must be the yardstick's bits / integers; boot_mean and boot_se are held to the relative
bound 4 n_boot 2^-52 (fp64 summation of n_boot integers in any order) -- the largest ratio to it is printed.  Outputs, boot_out
and the workspace start out poisoned.  Shapes are the smallest at which the kernels take another path: sizes around the
wave (64) and the sort's powers of two, n_boot around NM_BOOT_CHUNK, the LDS ceiling at n = 8192, the close pass's LDS ceiling
at n_boot = NM_BOOT_MAX."""
import numpy as np
import pytest
import torch

from multi_modal_normative_modeling_amd import _lib, metrics
from multi_modal_normative_modeling_amd.engine import _stream_ptr
from tests import auc_bootstrap_ref as R
from tests.table_stats_util import same_bits as _same_bits

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
POISON, POISON_INT, SEED = 777.0, 0x5A5A5A5A, 20240611
CH = _lib.NM_BOOT_CHUNK


def _set(n_pos, n_neg, seed, quantum=0.25, shift=0.6):
    """Scores quantised to `quantum` (ties are common), the positives shifted up, the classes interleaved."""
    rng = np.random.default_rng(seed)
    lab = np.zeros(n_pos + n_neg, dtype=np.int32)
    lab[rng.permutation(n_pos + n_neg)[:n_pos]] = 1
    s = rng.standard_normal(n_pos + n_neg) + shift * lab
    return (np.round(s / quantum) * quantum).astype(np.float32), lab


def _launch(sets, n_boot, ci=0.95, seed=SEED, streams=None, pairs=None, max_set=None):
    """The C entry point on poisoned buffers: (out [n_sets, 8], pairs_out [n_pairs, 8] or None, boot_out [n_sets, n_boot])."""
    sizes = [len(s) for s, _ in sets]
    flat_s = np.concatenate([np.asarray(s, dtype=np.float32) for s, _ in sets] + [np.zeros(1, dtype=np.float32)])
    flat_l = np.concatenate([np.asarray(l, dtype=np.int32) for _, l in sets] + [np.zeros(1, dtype=np.int32)])
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    s, l, o = (torch.as_tensor(v).to(DEV) for v in (flat_s, flat_l, off))
    st = torch.as_tensor(np.asarray(streams, dtype=np.int32)).to(DEV) if streams is not None else None
    n_sets, n_pairs = len(sets), (0 if pairs is None else len(pairs))
    pr = torch.as_tensor(np.asarray(pairs, dtype=np.int32).reshape(-1, 2)).to(DEV) if n_pairs else None
    max_set = max_set if max_set is not None else max(max(sizes), 1)
    lo, hi = metrics.boot_indices(n_boot, ci)
    lib = _lib.load()
    need = int(lib.nm_auc_bootstrap_workspace(n_sets, max_set, n_boot, n_pairs))
    assert need > 0
    ws = torch.full((need,), 0xA5, dtype=torch.uint8, device=DEV)
    out = torch.full((n_sets, 8), POISON, dtype=torch.float64, device=DEV)
    pout = torch.full((max(n_pairs, 1), 8), POISON, dtype=torch.float64, device=DEV)
    boot = torch.full((n_sets, n_boot), POISON_INT, dtype=torch.int32, device=DEV)
    _lib.check(lib.nm_auc_bootstrap(s.data_ptr(), l.data_ptr(), o.data_ptr(), st.data_ptr() if st is not None else None, n_sets, max_set,
                                    n_boot, lo, hi, seed, pr.data_ptr() if pr is not None else None, n_pairs, ws.data_ptr(), need,
                                    out.data_ptr(), pout.data_ptr() if n_pairs else None, boot.data_ptr(), _stream_ptr(DEV)),
               "nm_auc_bootstrap")
    torch.cuda.synchronize()
    if not n_pairs:
        assert bool((pout == POISON).all())                            # (nothing of it is touched without pairs)
    return out.cpu().numpy(), (pout.cpu().numpy() if n_pairs else None), boot.cpu().numpy()


def _expect(sets, n_boot, ci=0.95, seed=SEED, streams=None, pairs=None, max_set=None):
    """The same three arrays from the yardstick."""
    lo, hi = R.boot_indices(n_boot, ci)
    streams = list(range(len(sets))) if streams is None else list(streams)
    max_set = max_set if max_set is not None else max(max(len(s) for s, _ in sets), 1)
    rows, boots = [], []
    for (s, l), k in zip(sets, streams):
        row, bt = R.set_row(s, l, n_boot, lo, hi, seed, k, max_set=max_set, return_boot=True)
        rows.append(row)
        boots.append(bt)
    prs = None
    if pairs is not None and len(pairs):
        prs = np.stack([R.pair_row((*sets[a], streams[a]), (*sets[c], streams[c]), n_boot, lo, hi, seed, max_set=max_set) for a, c in pairs])
    return np.stack(rows), prs, np.stack(boots)


def _compare(got, ref, n_boot, what):
    """Bits for every column but the two moments, integers for boot_out; the moments within 4 n_boot 2^-52; the largest ratio."""
    (out, pout, boot), (rout, rpout, rboot) = got, ref
    assert np.array_equal(boot, rboot), what
    assert not (out == POISON).any() and not (boot == POISON_INT).any(), what
    worst = 0.0
    for name, g, r in (("sets", out, rout), ("pairs", pout, rpout)):
        if r is None:
            assert g is None
            continue
        assert not (g == POISON).any(), (what, name)
        exact = [0, 1, 2, 5, 6, 7]
        assert _same_bits(g[:, exact], r[:, exact]), (what, name, g[:, exact], r[:, exact])
        for j in (3, 4):
            assert np.array_equal(np.isnan(g[:, j]), np.isnan(r[:, j])), (what, name, j)
            ok = ~np.isnan(r[:, j])
            err, mag = np.abs(g[ok, j] - r[ok, j]), np.abs(r[ok, j])
            assert np.all(err <= R.moment_bound(n_boot) * mag), (what, name, j, g[ok, j], r[ok, j])
            nz = mag > 0
            if nz.any():
                worst = max(worst, float((err[nz] / (R.moment_bound(n_boot) * mag[nz])).max()))
    print(f"[auc_bootstrap] {what}: boot_mean / boot_se within {worst:.3g} of the bound 4 n_boot 2^-52"
          + (" (exactly the yardstick's)" if worst == 0.0 else ""))
    return worst


def _base_sets():
    shapes = [(1, 1), (1, 32), (63, 1), (31, 32), (32, 32), (33, 32), (90, 81), (127, 128), (128, 128), (129, 128), (532, 532)]
    sets = [_set(p, q, 100 + i) for i, (p, q) in enumerate(shapes)]
    equal = (np.full(40, 1.25, dtype=np.float32), _set(17, 23, 7)[1])
    return sets + [equal]


@pytest.fixture(scope="module")
def base():
    """One launch over the sizes: n = 2, 33 with one positive, 64 with one negative, 63 / 64 / 65, 171, 255 / 256 / 257, 1064 and
    an all-equal set; 130 resamples (three chunks, the last one short); pairs among them.  Shared, never changed."""
    sets = _base_sets()
    n_boot = 2 * CH + 2
    got = _launch(sets, n_boot)
    ref = _expect(sets, n_boot)
    return sets, n_boot, got, ref


def test_sizes_around_the_wave_and_the_sort_with_ties(base):
    sets, n_boot, got, ref = base
    _compare(got, ref, n_boot, "sizes 2..1064")
    out, _, boot = got
    assert [int(v) for v in out[:, 6] + out[:, 7]] == [2, 33, 64, 63, 64, 65, 171, 255, 256, 257, 1064, 40]
    assert np.all(boot[-1] == 17 * 23) and out[-1, 0] == 0.5 and out[-1, 1] == out[-1, 2] == out[-1, 3] == 0.5 and out[-1, 4] == 0.0
    assert np.all(out[:, 1] <= out[:, 2]) and np.all(out[:, 5] == n_boot)
    post = metrics.posthoc_metrics([torch.as_tensor(s) for s, _ in sets], [torch.as_tensor(l) for _, l in sets]).cpu().numpy()
    diff = np.abs(post[:, 0] - out[:, 0])
    print(f"[auc_bootstrap] roc_auc against nm_posthoc_metrics: largest difference {diff.max():.3g}")
    assert np.all(diff <= 1e-12)
    assert np.array_equal(post[:, 6:], out[:, 6:])


def test_signed_zeros_and_infinities():
    s = np.array([-0.0, 0.0, np.inf, np.inf, -np.inf, 1.0, 0.0, -0.0, -1.0, np.inf, -np.inf, 0.0], dtype=np.float32)
    l = np.array([1, 0, 1, 0, 0, 1, 1, 0, 0, 1, 1, 0], dtype=np.int32)
    sets = [(s, l), (s[::-1].copy(), l[::-1].copy()), _set(9, 8, 3)]
    got, ref = _launch(sets, 70), _expect(sets, 70)
    _compare(got, ref, 70, "-0 / +0 / inf / -inf")
    by_hand = sum(2 * (a > b) + (a == b) for a in s[l == 1].astype(np.float64) for b in s[l == 0].astype(np.float64))
    assert got[0][0, 0] == by_hand / (2 * 6 * 6)


def test_invalid_sets_get_nan_rows_and_leave_their_neighbours_alone():
    good = [_set(20, 13, 1), _set(7, 30, 2), _set(33, 32, 3)]
    nan = _set(10, 10, 4)
    nan[0][5] = np.nan
    one_class = (_set(10, 10, 5)[0], np.ones(20, dtype=np.int32))
    empty = (np.zeros(0, dtype=np.float32), np.zeros(0, dtype=np.int32))
    too_long = _set(40, 41, 6)                                         # 81 > max_set = 65
    sets = [nan, good[0], one_class, empty, good[1], too_long, good[2], empty]
    streams = [10, 0, 11, 12, 1, 13, 2, 14]
    pairs = [(1, 1), (0, 1), (1, 0), (3, 3), (5, 5)]
    got = _launch(sets, 70, streams=streams, pairs=pairs, max_set=65)
    ref = _expect(sets, 70, streams=streams, pairs=pairs, max_set=65)
    _compare(got, ref, 70, "invalid sets")
    out, pout, boot = got
    for k in (0, 2, 3, 5, 7):
        assert np.all(np.isnan(out[k])) and np.all(boot[k] == -1), k
    assert np.all(np.isnan(pout[1:])) and not np.isnan(pout[0]).any()
    alone = _launch(good, 70, streams=[0, 1, 2], max_set=65)
    assert out[[1, 4, 6]].tobytes() == alone[0].tobytes() and boot[[1, 4, 6]].tobytes() == alone[2].tobytes()


@pytest.mark.parametrize("n_boot", [1, CH - 1, CH, CH + 1, 2 * CH + 1, 300])
def test_resample_counts_around_the_chunk(n_boot):
    sets = [_set(20, 13, 1), _set(20, 13, 2), _set(1, 5, 3)]
    sets[1] = (sets[1][0], sets[0][1])                                 # (the labels of set 0: a pair)
    kw = dict(streams=[4, 4, 9], pairs=[(0, 1), (2, 2)])
    got, ref = _launch(sets, n_boot, **kw), _expect(sets, n_boot, **kw)
    _compare(got, ref, n_boot, f"n_boot = {n_boot}")
    if n_boot == 1:
        assert metrics.boot_indices(1, 0.95) == (0, 0)
        assert np.all(np.isnan(got[0][:, 4])) and np.all(np.isnan(got[1][:, 4])) and not np.isnan(got[0][:, :4]).any()


def test_the_largest_set_with_as_many_groups_as_scores():
    rng = np.random.default_rng(8)
    s = rng.permutation(8192).astype(np.float32) * 0.5 - 1000.0        # distinct: G = 8192
    l = np.zeros(8192, dtype=np.int32)
    l[np.argsort(s + 2000.0 * rng.standard_normal(8192))[4096:]] = 1   # the upper half of a noisy ranking
    assert len(np.unique(s)) == 8192 and int(l.sum()) == 4096
    sets = [(s, l), _set(5, 6, 1)]
    got, ref = _launch(sets, CH + 1), _expect(sets, CH + 1)
    _compare(got, ref, CH + 1, "n = 8192, 4096 / 4096")
    assert got[0][0, 6] == got[0][0, 7] == 4096


def test_the_largest_set_with_one_negative():
    s, l = _set(8191, 1, 12)
    got, ref = _launch([(s, l)], 20), _expect([(s, l)], 20)
    _compare(got, ref, 20, "n = 8192, 8191 / 1")
    assert got[0][0, 6] == 8191 and got[0][0, 7] == 1


def test_the_most_resamples():
    a, c = _set(6, 7, 21), _set(6, 7, 22)
    sets = [a, (c[0], a[1])]
    kw = dict(streams=[3, 3], pairs=[(0, 1)])
    n_boot = _lib.NM_BOOT_MAX
    got, ref = _launch(sets, n_boot, **kw), _expect(sets, n_boot, **kw)
    _compare(got, ref, n_boot, f"n_boot = {n_boot}")


def test_a_sets_row_does_not_depend_on_its_place(base):
    sets, n_boot, got, _ = base
    perm = [7, 2, 11, 0, 5, 10, 1, 9, 3, 8, 6, 4]
    moved = _launch([sets[k] for k in perm], n_boot, streams=perm)
    assert moved[0].tobytes() == got[0][perm].tobytes() and moved[2].tobytes() == got[2][perm].tobytes()
    explicit = _launch(sets, n_boot, streams=list(range(len(sets))))
    assert explicit[0].tobytes() == got[0].tobytes() and explicit[2].tobytes() == got[2].tobytes()


def test_two_calls_give_the_same_bytes_and_another_seed_other_resamples(base):
    sets, n_boot, got, _ = base
    again = _launch(sets, n_boot)
    assert again[0].tobytes() == got[0].tobytes() and again[2].tobytes() == got[2].tobytes()
    other = _launch(sets, n_boot, seed=SEED + 1)
    assert not np.array_equal(other[2][:-1], got[2][:-1])
    assert other[0][:, 0].tobytes() == got[0][:, 0].tobytes()           # (the observed AUC knows no seed)
    assert np.array_equal(other[2][-1], got[2][-1])                     # (the all-equal set: every resample the same)


def test_pairs():
    a, c, other = _set(30, 41, 31), _set(30, 41, 32), _set(30, 41, 33)
    c = (c[0], a[1])                                                    # the labels of a: the same subjects
    swapped = a[1].copy()
    i, j = np.flatnonzero(swapped == 1)[0], np.flatnonzero(swapped == 0)[0]
    swapped[i], swapped[j] = 0, 1                                       # one differing positive, one differing negative: n_pos stays
    nan = (c[0].copy(), a[1])
    nan[0][0] = np.nan
    sets = [a, c, (other[0], a[1]), (c[0], swapped), nan, _set(29, 41, 34)]
    streams = [5, 5, 6, 5, 5, 5]
    pairs = [(0, 1), (1, 0), (0, 0), (0, 2), (0, 3), (0, 4), (4, 0), (0, 5)]
    n_boot = 150
    got = _launch(sets, n_boot, streams=streams, pairs=pairs)
    ref = _expect(sets, n_boot, streams=streams, pairs=pairs)
    _compare(got, ref, n_boot, "pairs")
    pout = got[1]
    assert not np.isnan(pout[:3]).any() and np.all(np.isnan(pout[3:]))
    assert pout[0, 0] == -pout[1, 0] and pout[0, 6] == pout[1, 7] and pout[0, 1] == -pout[1, 2] and pout[0, 5] == pout[1, 5]
    assert tuple(pout[2]) == (0.0, 0.0, 0.0, 0.0, 0.0, 1.0, n_boot, n_boot)
    none = _launch(sets, n_boot, streams=streams, pairs=None)          # n_pairs = 0 with pairs = NULL
    assert none[1] is None and none[0].tobytes() == got[0].tobytes() and none[2].tobytes() == got[2].tobytes()


def test_many_full_size_sets_with_the_distribution_in_the_workspace():
    """Twenty sets of 1064 through metrics.auc_bootstrap without return_boot: the A2* live in the workspace alone."""
    sets = [_set(532, 532, 200 + k, quantum=1.0 / 16) for k in range(20)]
    n_boot = 2 * CH + 2
    out = metrics.auc_bootstrap([torch.as_tensor(s) for s, _ in sets], [torch.as_tensor(l) for _, l in sets], n_boot=n_boot, seed=SEED)
    ref = _expect(sets, n_boot)
    _compare((out.cpu().numpy(), None, ref[2]), ref, n_boot, "20 sets of 1064")


def test_the_python_entry_points(base):
    sets, n_boot, got, _ = base
    sc, lb = [torch.as_tensor(s) for s, _ in sets], [torch.as_tensor(l) for _, l in sets]
    out = metrics.auc_bootstrap(sc, lb, n_boot=n_boot, seed=SEED)
    assert isinstance(out, torch.Tensor) and out.cpu().numpy().tobytes() == got[0].tobytes()
    out, pout, boot = metrics.auc_bootstrap(sc, lb, n_boot=n_boot, seed=SEED, pairs=[(4, 4)], return_boot=True)
    assert boot.dtype == torch.int32 and boot.cpu().numpy().tobytes() == got[2].tobytes()
    assert tuple(pout.shape) == (1, 8) and float(pout[0, 5]) == 1.0
    out, pout = metrics.auc_bootstrap(sc, lb, n_boot=n_boot, seed=SEED, pairs=[])
    assert tuple(pout.shape) == (0, 8)
    a, c = _set(30, 41, 31), _set(30, 41, 32)
    lo, hi = R.boot_indices(200, 0.9)
    res = metrics.auc_compare(a[0], c[0], a[1], n_boot=200, ci=0.9, seed=3)
    ref = R.pair_row((a[0], a[1], 0), (c[0], a[1], 0), 200, lo, hi, seed=3)
    assert tuple(res) == metrics.AUC_COMPARE_COLUMNS
    for j, name in enumerate(metrics.AUC_COMPARE_COLUMNS):
        if j in (3, 4):
            assert abs(res[name] - ref[j]) <= R.moment_bound(200) * abs(ref[j]), name
        else:
            assert res[name] == ref[j], name
