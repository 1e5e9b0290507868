"""tests/pack_ref.py held to itself: its sizes are nm_xb_elems', its bf16 conversion is torch's, Table.packed_rows'
un-permutation restated on the reference image returns x | c | 1 | 0, and the comparison the GPU tests use
(pack_ref.compare_packed) flags every way a pack kernel is likely to be wrong."""
import numpy as np
import pytest
import torch

from multi_modal_normative_modeling_amd import _lib
from tests import pack_ref as R

CASES = [(N, D, C) for N in R.PACK_N for D, C in R.PACK_DC]


@pytest.fixture(scope="module")
def lib():
    if not _lib.LIB_PATH.exists():
        import __graft_entry__ as ge
        ge.build()
    return _lib.load()


def test_sizes_agree_with_nm_xb_elems(lib):
    for N, D, C in CASES + [(8192, 1137, 29), (1, 1, 0)]:
        g = R.geometry(N, D, C)
        assert g["rows_alloc"] % 256 == 0 and g["rows_alloc"] >= max(N, 1) and g["rows_alloc"] - N < 256 + (N == 0)
        assert g["Kx"] % 32 == 0 and 0 <= g["Kx"] - (D + C + 1) < 32
        assert g["x_pitch"] % 4 == 0 and 0 <= g["x_pitch"] - D < 4 and g["Cz"] % 8 == 0 and 0 <= g["Cz"] - (C + 1) < 8
        assert lib.nm_xb_elems(g["rows_alloc"], g["Kx"]) == R.xb_elems(g["rows_alloc"], g["Kx"]) == g["rows_alloc"] * g["nch"] * 72
        if (N, D, C) in CASES:
            x, c = R.pack_case(N, D, C)
            xb, xf, cz = R.pack_ref(x, c)
            assert xb.shape == (g["rows_alloc"] * g["nch"] * 72,) and xb.dtype == np.uint16
            assert xf.shape == (g["rows_alloc"], g["x_pitch"]) and xf.dtype == np.float32
            assert cz.shape == (g["rows_alloc"], g["Cz"]) and cz.dtype == np.uint16
    assert [R.geometry(1, D, C)["Kx"] for D, C in R.PACK_DC] == [32, 64, 64, 96, 96, 96, 96, 96, 32, 64, 160]
    assert [R.geometry(1, D, C)["nch"] for D, C in R.PACK_DC] == [1, 1, 1, 2, 2, 2, 2, 2, 1, 1, 3]


def test_bf16_conversion_is_round_to_nearest_even():
    assert np.array_equal(R.bf16_rne(R.PLANTED), R.PLANTED_BF16)
    rng = np.random.default_rng(0)
    bits = rng.integers(0, 2 ** 32, size=200000, dtype=np.uint64).astype(np.uint32)
    edge = np.array([0x3F808000, 0x3F818000, 0x3F807FFF, 0x3F808001, 0x7F7FFFFF, 0x7F800000, 0xFF800000, 0x00000001, 0x80000000,
                     0x00008000, 0x00018000, 0x007FFFFF], dtype=np.uint32)
    a = np.concatenate([bits, edge]).view(np.float32)
    a = a[~np.isnan(a)]
    ref = torch.from_numpy(a.copy()).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    assert np.array_equal(R.bf16_rne(a), ref)
    assert (R.bf16_rne(R.PLANTED) != R.bf16_trunc(R.PLANTED)).any()      # the planted values tell the two conversions apart


@pytest.mark.parametrize("N,D,C", CASES)
def test_unpermuted_image_is_the_operand_rows(N, D, C):
    x, c = R.pack_case(N, D, C)
    g = R.geometry(N, D, C)
    xb, xf, cz = R.pack_ref(x, c)
    rows = R.rows_of_image(xb, g["rows_alloc"], g["Kx"])
    want = np.zeros((g["rows_alloc"], g["Kx"]), dtype=np.float32)
    want[:N, :D], want[:N, D:D + C], want[:N, D + C] = x, c, 1.0
    want = torch.from_numpy(want).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    assert np.array_equal(rows, want)
    # the same through torch, exactly as Table.packed_rows does it
    t = torch.from_numpy(xb.view(np.int16).copy()).view(g["rows_alloc"] // 256, g["nch"], 256, 72)[..., :64]
    t = t.permute(0, 2, 1, 3).reshape(g["rows_alloc"], g["nch"] * 64)[:, :g["Kx"]]
    assert np.array_equal(t.numpy().view(np.uint16), want)
    # element by element from the documented formula, on a sample of coordinates
    img = xb.reshape(g["rows_alloc"] // 256, g["nch"], 256, 72)
    rng = np.random.default_rng(N + D)
    for _ in range(200):
        t_, k_, r_, j_ = (int(rng.integers(0, s)) for s in img.shape)
        row, col = 256 * t_ + r_, 64 * k_ + j_
        exp = want[row, col] if (j_ < 64 and row < N and col < g["Kx"]) else 0
        assert img[t_, k_, r_, j_] == exp, (t_, k_, r_, j_)
    # what is not data is zero: pad columns, dead rows, the columns past the ones column
    assert not img[..., 64:].any() and not rows[N:].any() and not rows[:, D + C + 1:].any()
    assert (rows[:N, D + C] == 0x3F80).all()
    assert not xf[N:].any() and not xf[:, D:].any() and np.array_equal(xf[:N, :D].view(np.uint32), x.view(np.uint32))
    assert not cz[N:].any() and not cz[:, C + 1:].any() and (cz[:N, C] == 0x3F80).all()
    assert R.compare_packed(xb, xf, cz, x, c) == []


@pytest.mark.parametrize("N,D,C", [(257, 35, 29), (513, 130, 5), (1, 2, 29), (256, 32, 0), (255, 64, 29)])
def test_the_comparison_flags_each_mutation(N, D, C):
    x, c = R.pack_case(N, D, C)
    g = R.geometry(N, D, C)
    xb, xf, cz = R.pack_ref(x, c)
    tiles, nch = g["rows_alloc"] // 256, g["nch"]

    def flagged(xb_=xb, xf_=xf, cz_=cz):
        return R.compare_packed(xb_, xf_, cz_, x, c)

    assert flagged() == []
    img = xb.reshape(tiles, nch, 256, 72)
    if nch > 1:                                                         # [tile][256][chunk][72] instead of [tile][chunk][256][72]
        assert flagged(xb_=np.ascontiguousarray(img.transpose(0, 2, 1, 3)).reshape(-1))
    rows = R.operand_rows(x, c)                                         # rows in one piece, [rows_alloc][nch * 64 + pad]: no chunks at all
    if N > 1:
        assert flagged(xb_=np.concatenate([rows.reshape(-1), np.zeros(xb.size - rows.size, np.uint16)]))
    m = img.copy(); m[tiles - 1, nch - 1, (N - 1) % 256, 71] = 0x3F80      # one nonzero pad column
    assert flagged(xb_=m.reshape(-1))
    m = img.copy(); m[0, 0, 0, 64] = 0x7FC0                               # a NaN left in a pad column
    assert flagged(xb_=m.reshape(-1))
    if N < g["rows_alloc"]:                                             # one nonzero dead row element, in each buffer
        m = img.copy(); m[tiles - 1, 0, N % 256, 0] = 0x0001
        assert flagged(xb_=m.reshape(-1))
        m = xf.copy(); m[N, 0] = np.float32(1e-40)
        assert flagged(xf_=m)
        m = cz.copy(); m[g["rows_alloc"] - 1, C] = 0x3F80
        assert flagged(cz_=m)
    for at in (D + C - 1, D + C + 1):                                   # the ones column off by one
        if 0 <= at < nch * 64:
            w = R.operand_rows(x, c, ones_at=at)
            if at < D + C:
                w[:N, D + C] = 0
            assert flagged(xb_=R.image_of_rows(w))
    m = cz.copy(); m[:N, C], m[:N, C + 1] = 0, 0x3F80
    assert flagged(cz_=m)
    assert flagged(xb_=R.image_of_rows(R.operand_rows(x, c, convert=R.bf16_trunc)))      # truncation instead of rounding
    if C > 0:
        live = np.concatenate([c, np.ones((N, 1), np.float32)], 1)
        assert flagged(cz_=R.bf16_trunc(np.pad(live, ((0, g["rows_alloc"] - N), (0, g["Cz"] - C - 1)))))
    m = xf.copy().view(np.uint32); m[0, 0] ^= 1                           # one bit of the fp32 copy; a lost sign of zero
    assert flagged(xf_=m.view(np.float32))
    for zr, zc in np.argwhere(np.signbit(x) & (x == 0))[:1]:
        m = xf.copy(); m[zr, zc] = 0.0
        assert flagged(xf_=m)
    assert flagged(xb_=xb[:-72]) and flagged(xf_=xf.astype(np.float64))  # a wrong size or type is a difference too
