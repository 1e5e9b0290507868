"""A plain restatement of the packed table layout, written from the documentation of engine.Table and of
nm_modality_t.xb / nm_pack_table in include/nmhip.h -- numpy only, no device, no library call.

  rows_alloc = max(1, ceil(N / 256)) * 256        Kx = roundup32(D + C + 1)        nch = ceil(Kx / 64)
  x_pitch = roundup4(D)                            Cz = roundup8(C + 1)

  xb    [rows_alloc / 256][nch][256][72] bf16   element (tile, chunk, row, j): column 64 chunk + j of  x | c | 1 | 0  of
                                                row 256 tile + row when j < 64 and that row is below N, else zero
  x_f32 [rows_alloc][x_pitch] fp32              x, zero beyond D and beyond N
  cz    [rows_alloc][Cz] bf16                   c | 1 | 0, zero rows beyond N

fp32 -> bf16 is round-to-nearest-even, done here on the bit patterns.  The GPU tests (tests/test_gpu_pack.py) hold both
pack kernels to this image bit for bit; tests/test_pack_ref_cpu.py holds this file to itself."""
import math

import numpy as np

TILE, CHUNK, PITCH = 256, 64, 72


def geometry(N, D, C):
    rows_alloc = max(1, math.ceil(N / TILE)) * TILE
    Kx = (D + C + 1 + 31) // 32 * 32
    return dict(N=N, D=D, C=C, rows_alloc=rows_alloc, Kx=Kx, nch=(Kx + CHUNK - 1) // CHUNK, x_pitch=(D + 3) // 4 * 4,
                Cz=(C + 1 + 7) // 8 * 8)


def xb_elems(rows_alloc, Kx):
    """What nm_xb_elems documents: the elements the image of a [rows_alloc, Kx] table holds."""
    return rows_alloc * ((Kx + CHUNK - 1) // CHUNK) * PITCH


def bf16_rne(a):
    """fp32 array -> bf16 bit patterns (uint16), round to nearest, ties to even; a NaN stays a (quiet) NaN."""
    u = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)
    nan = (u & 0x7FFFFFFF) > 0x7F800000
    return np.where(nan, ((u >> 16) | 0x40).astype(np.uint16), r)


def bf16_trunc(a):
    """The wrong conversion: the upper half of the fp32 pattern (a mutation for the self-test)."""
    return (np.ascontiguousarray(a, dtype=np.float32).view(np.uint32) >> 16).astype(np.uint16)


def operand_rows(x, c, ones_at=None, convert=bf16_rne):
    """x | c | 1 | 0 as bf16 patterns [rows_alloc, nch * 64]; rows >= N are zero."""
    N, D = x.shape
    C = c.shape[1]
    g = geometry(N, D, C)
    full = np.zeros((g["rows_alloc"], g["nch"] * CHUNK), dtype=np.float32)
    full[:N, :D] = x
    full[:N, D:D + C] = c
    full[:N, D + C if ones_at is None else ones_at] = 1.0
    return convert(full)


def image_of_rows(rows_u16):
    """[rows_alloc, nch * 64] patterns -> the flat [tile][chunk][256][72] image, 8 zero pad columns per row."""
    rows_alloc, width = rows_u16.shape
    tiles, nch = rows_alloc // TILE, width // CHUNK
    img = np.zeros((tiles, nch, TILE, PITCH), dtype=np.uint16)
    for t in range(tiles):
        for k in range(nch):
            img[t, k, :, :CHUNK] = rows_u16[t * TILE:(t + 1) * TILE, k * CHUNK:(k + 1) * CHUNK]
    return img.reshape(-1)


def rows_of_image(xb, rows_alloc, Kx):
    """Table.packed_rows' un-permutation, restated: the flat image back to [rows_alloc, Kx] patterns."""
    nch = (Kx + CHUNK - 1) // CHUNK
    img = np.asarray(xb).reshape(rows_alloc // TILE, nch, TILE, PITCH)
    out = np.zeros((rows_alloc, nch * CHUNK), dtype=np.uint16)
    for t in range(rows_alloc // TILE):
        for k in range(nch):
            out[t * TILE:(t + 1) * TILE, k * CHUNK:(k + 1) * CHUNK] = img[t, k, :, :CHUNK]
    return out[:, :Kx]


def pack_ref(x, c):
    """(xb uint16 [rows_alloc * nch * 72], x_f32 float32 [rows_alloc, x_pitch], cz uint16 [rows_alloc, Cz])."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    c = np.ascontiguousarray(c, dtype=np.float32)
    N, D = x.shape
    C = c.shape[1]
    g = geometry(N, D, C)
    xb = image_of_rows(operand_rows(x, c))
    xf = np.zeros((g["rows_alloc"], g["x_pitch"]), dtype=np.float32)
    xf[:N, :D] = x
    czf = np.zeros((g["rows_alloc"], g["Cz"]), dtype=np.float32)
    czf[:N, :C] = c
    czf[:N, C] = 1.0
    return xb, xf, bf16_rne(czf)


def mismatches(got, ref, what, shape=None, limit=4):
    """Compare two arrays through their bit patterns; a list of readable differences (empty = identical).  `shape`
    names the axes of a flat buffer (the xb image: (tiles, nch, 256, 72)) so a difference reads as a coordinate."""
    got, ref = np.ascontiguousarray(got), np.ascontiguousarray(ref)
    if got.dtype.itemsize != ref.dtype.itemsize or got.size != ref.size:
        return [f"{what}: {got.size} x {got.dtype} against {ref.size} x {ref.dtype}"]
    bits = {2: np.uint16, 4: np.uint32, 8: np.uint64}[ref.dtype.itemsize]
    gi, ri = got.reshape(-1).view(bits), ref.reshape(-1).view(bits)
    bad = np.flatnonzero(gi != ri)
    if bad.size == 0:
        return []
    shape = tuple(shape) if shape is not None else ref.shape
    out = [f"{what}: {bad.size} of {ri.size} elements differ"]
    for i in bad[:limit]:
        out.append(f"{what}{tuple(int(v) for v in np.unravel_index(i, shape))}: got 0x{int(gi[i]):x}, expected 0x{int(ri[i]):x}")
    return out


def compare_packed(xb, x_f32, cz, x, c):
    """Every difference between a packed table's three buffers and pack_ref(x, c); [] when they agree bit for bit."""
    x = np.asarray(x)
    g = geometry(x.shape[0], x.shape[1], np.asarray(c).shape[1])
    rxb, rxf, rcz = pack_ref(x, c)
    return (mismatches(xb, rxb, "xb", (g["rows_alloc"] // TILE, g["nch"], TILE, PITCH)) + mismatches(x_f32, rxf, "x_f32")
            + mismatches(cz, rcz, "cz"))


# ---- the shapes and values of the pack tests (shared by the CPU self-test and the GPU tests) ---------------------------
PACK_N = (1, 255, 256, 257, 513)            # one row, a full tile, one row into the next tile, three tiles
# (D, C): D + C + 1 = 32 (Kx 32, half a chunk); Kx 64; the ones column last of chunk 0; first of chunk 1; the covariates
# across the chunk boundary; D around one chunk; no covariates (null c); three chunks.  D mod 4 takes 0, 1, 2 and 3
PACK_DC = ((2, 29), (3, 29), (34, 29), (35, 29), (40, 29), (63, 29), (64, 29), (65, 29), (31, 0), (32, 0), (130, 5))
assert {d % 4 for d, _ in PACK_DC} == {0, 1, 2, 3}

# a bf16 tie in each direction (to even: down, up), a negative tie, an fp32 subnormal, a finite value that rounds up to
# bf16 infinity, and a negative zero
PLANTED = np.array([1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, -(1 + 2.0 ** -8), 1e-40, 3.4e38, -0.0], dtype=np.float32)
PLANTED_BF16 = np.array([0x3F80, 0x3F82, 0xBF80, 0x0001, 0x7F80, 0x8000], dtype=np.uint16)


def pack_case(N, D, C, seed=0):
    """x [N, D], c [N, C] fp32: ordinary normals with the PLANTED values in live rows (first, last, both sides of the
    tile boundary), spread over x and c columns."""
    rng = np.random.default_rng(1000 * N + 10 * D + C + seed)
    xc = rng.standard_normal((N, D + C)).astype(np.float32)
    W = D + C
    assert W >= 3 * len(PLANTED)
    for r in sorted({0, N - 1, min(255, N - 1), min(256, N - 1)}):
        for i, v in enumerate(PLANTED):
            xc[r, (3 * i + 5 * r) % W] = v
    return np.ascontiguousarray(xc[:, :D]), np.ascontiguousarray(xc[:, D:])
