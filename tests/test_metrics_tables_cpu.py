"""The host path of the table statistics without a device: metrics._set_table's bytes (and its three wrappers') against each of the three ctypes structs
filled by hand, field by field, and the split rule of metrics._row_words.  Host tensors stand in for device ones.  Three sets per
table: no rows (null pointers, pitch = the width), one row (pitch = the width whatever the stride), five rows of a [:, :D] view of
a wider buffer (pitch = its row stride)."""
import numpy as np
import pytest
import torch

from multi_modal_normative_modeling_amd import _lib, metrics

D = 7


def _views():
    """(the three tables, their expected pitches): 0 rows, 1 row of a buffer of pitch 11, 5 rows of a buffer of pitch 12."""
    wide, one = torch.zeros(5, 12), torch.zeros(3, 11)
    views = [wide[:0, :D], one[2:3, :D], wide[:, :D]]
    assert [v.stride(0) for v in views] == [12, 11, 12]
    return views, [D, D, 12]


def _by_hand(struct, views, pitches):
    table = (struct * len(views))()
    for e, v, p in zip(table, views, pitches):
        e.x = v.data_ptr() if v.shape[0] else None
        e.rows = v.shape[0]
        e.pitch = p
    return table


def test_roi_set_bytes():
    views, pitches = _views()
    grp = [torch.zeros(len(v), dtype=torch.int32) for v in views]
    want = _by_hand(_lib.NmRoiSet, views, pitches)
    want[1].group, want[2].group = grp[1].data_ptr(), grp[2].data_ptr()
    got = metrics._set_table(_lib.NmRoiSet, views, group=grp)
    assert bytes(got) == bytes(want) and len(bytes(got)) == 3 * 24
    assert got[0].x is None and got[0].group is None and got[1].x == views[1].data_ptr()
    assert bytes(metrics._roi_table(views, grp)) == bytes(want)


def test_reg_set_bytes():
    views, pitches = _views()
    n_cov = 2
    tgt = [torch.zeros(len(v)) for v in views]
    cov = [torch.zeros(len(v), n_cov) for v in views]
    inc = [torch.ones(0, dtype=torch.int32), None, torch.ones(5, dtype=torch.int32)]
    want = _by_hand(_lib.NmRegSet, views, pitches)
    for k, e in enumerate(want):
        e.cov_pitch, e.pad = n_cov, 0
        if views[k].shape[0]:
            e.target, e.cov = tgt[k].data_ptr(), cov[k].data_ptr()
    want[2].include = inc[2].data_ptr()
    got = metrics._set_table(_lib.NmRegSet, views, target=tgt, cov=cov, include=inc, cov_pitch=n_cov)
    assert bytes(got) == bytes(want) and len(bytes(got)) == 3 * 48
    assert got[1].include is None and got[2].include == inc[2].data_ptr() and [e.cov_pitch for e in got] == [2, 2, 2]
    # without covariates and include words: null pointers, cov_pitch 0
    bare = _by_hand(_lib.NmRegSet, views, pitches)
    bare[1].target, bare[2].target = tgt[1].data_ptr(), tgt[2].data_ptr()
    assert bytes(metrics._set_table(_lib.NmRegSet, views, target=tgt, cov=None, include=None, cov_pitch=0)) == bytes(bare)
    # the wrapper the callers use: the same bytes, and covariates are not looked at when there are none (n_cov = 0)
    assert bytes(metrics._reg_table(views, tgt, cov, inc, n_cov)) == bytes(want)
    assert bytes(metrics._reg_table(views, tgt, cov, [None] * 3, 0)) == bytes(bare)


def test_norm_set_bytes():
    views, pitches = _views()
    grp = [torch.zeros(len(v), dtype=torch.int32) for v in views]
    loc = torch.zeros(5, 16)
    subs = [loc[:0, :D], loc[4:5, :D], loc[:, :D]]                    # (pitch 16 where the table's is 12)
    zs = [torch.zeros(len(v), D) for v in views]
    want = _by_hand(_lib.NmNormSet, views, pitches)
    for k, (e, off) in enumerate(zip(want, (0, 0, 1))):
        e.row_off, e.pad = off, 0
        if views[k].shape[0]:
            e.group, e.sub, e.z = grp[k].data_ptr(), subs[k].data_ptr(), zs[k].data_ptr()
    want[0].sub_pitch, want[1].sub_pitch, want[2].sub_pitch = 0, D, 16
    want[0].z_pitch, want[1].z_pitch, want[2].z_pitch = 0, D, D
    got = metrics._set_table(_lib.NmNormSet, views, group=grp, sub=subs, sub_pitch=subs, z=zs, z_pitch=zs)
    assert bytes(got) == bytes(want) and len(bytes(got)) == 3 * 56
    assert [e.row_off for e in got] == [0, 0, 1] and got[2].sub_pitch == 16 != got[2].pitch == 12
    # the table alone (nm_mahalanobis): x, rows, pitch and row_off, everything else zero
    bare = _by_hand(_lib.NmNormSet, views, pitches)
    bare[2].row_off = 1
    assert bytes(metrics._set_table(_lib.NmNormSet, views)) == bytes(bare)
    assert bytes(metrics._set_table(_lib.NmNormSet, views, group=None, sub=None, sub_pitch=None)) == bytes(bare)
    # the wrapper the callers use: subs give sub and sub_pitch, zs give z and z_pitch
    assert bytes(metrics._norm_table(views, grp, subs, zs)) == bytes(want) and bytes(metrics._norm_table(views)) == bytes(bare)


@pytest.mark.parametrize("dtype, src", [(torch.int32, np.int64), (torch.float32, np.float64)])
def test_row_words_are_views_of_one_buffer(dtype, src):
    seqs = [np.zeros(0, dtype=src), np.array([3], dtype=src), np.arange(5, dtype=src) - 2]
    out = metrics._row_words(seqs, "cpu", dtype)
    assert [tuple(t.shape) for t in out] == [(0,), (1,), (5,)] and all(t.dtype == dtype for t in out)
    assert out[1].tolist() == [3] and out[2].tolist() == [-2, -1, 0, 1, 2]
    base = out[1].untyped_storage().data_ptr()
    assert all(t.untyped_storage().data_ptr() == base for t in out) and out[1].untyped_storage().nbytes() == 6 * 4
    assert [t.storage_offset() for t in out] == [0, 0, 1]


def test_row_words_keep_a_none_and_normalise_include_words():
    inc = [np.array([0, 2, -1, 0, 7]), None, torch.tensor([5.0]), np.zeros(0)]
    out = metrics._row_words(inc, "cpu", torch.int32, nonzero=True)
    assert out[1] is None and out[0].tolist() == [0, 1, 1, 0, 1] and out[2].tolist() == [1] and out[3].numel() == 0
    assert all(t.dtype == torch.int32 for t in out if t is not None)
    assert out[0].untyped_storage().data_ptr() == out[2].untyped_storage().data_ptr() and out[2].storage_offset() == 5
    assert metrics._row_words([None, None], "cpu", torch.int32, nonzero=True) == [None, None]
