"""Both pack kernels (nm_pack_table through Table.repack, nm_pack_table_raw through the library on buffers allocated
here) against the plain layout of tests/pack_ref.py, bit for bit.  Every output buffer holds a NaN pattern before the
launch, so an element the kernel leaves unwritten shows; the inputs carry bf16 ties, an fp32 subnormal, a value that
rounds to bf16 infinity and a negative zero in live rows (pack_ref.pack_case)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import multi_modal_normative_modeling_amd as nm
from multi_modal_normative_modeling_amd import _lib, prep
from multi_modal_normative_modeling_amd.prep_device import DeviceCohort
from tests import pack_ref as R

DEV = "cuda:0"
CASES = [(N, D, C) for N in R.PACK_N for D, C in R.PACK_DC]


def _u16(t):
    return t.view(torch.int16).cpu().numpy().view(np.uint16)


def _operand_rows_f32(x, c, g):
    want = np.zeros((g["rows_alloc"], g["Kx"]), dtype=np.float32)
    want[:x.shape[0], :g["D"]], want[:x.shape[0], g["D"]:g["D"] + g["C"]], want[:x.shape[0], g["D"] + g["C"]] = x, c, 1.0
    return torch.from_numpy(want).to(torch.bfloat16)


@pytest.mark.parametrize("N,D,C", CASES)
def test_host_pack_against_the_plain_layout(N, D, C):
    x, c = R.pack_case(N, D, C)
    g = R.geometry(N, D, C)
    t = nm.Table(np.zeros_like(x), np.zeros_like(c), DEV)
    assert (t.N, t.D, t.C, t.Kx, t.rows_alloc, t.x_pitch, t.Cz) == tuple(g[k] for k in ("N", "D", "C", "Kx", "rows_alloc", "x_pitch", "Cz"))
    assert t.xb.numel() == R.xb_elems(g["rows_alloc"], g["Kx"])
    for buf in (t.xb, t.x_f32, t.cz):
        buf.fill_(float("nan"))
    assert t.repack(torch.from_numpy(x), torch.from_numpy(c))
    torch.cuda.synchronize()
    assert R.compare_packed(_u16(t.xb), t.x_f32.cpu().numpy(), _u16(t.cz), x, c) == []
    assert torch.equal(t.packed_rows().cpu().view(torch.int16), _operand_rows_f32(x, c, g).view(torch.int16))


def _raw_pack(sources, rows, center, scale, c, g):
    """nm_pack_table_raw on NaN-filled buffers of our own -> (xb, x_f32, cz) as numpy (uint16, float32, uint16)."""
    lib = _lib.load()
    srcs = [torch.from_numpy(np.ascontiguousarray(s, dtype=np.float64)).to(DEV) for s in sources]
    ptrs = torch.tensor([s.data_ptr() for s in srcs], dtype=torch.int64, device=DEV)
    widths = torch.tensor([s.shape[1] for s in srcs], dtype=torch.int32, device=DEV)
    rows_d = torch.from_numpy(np.asarray(rows, dtype=np.int32)).to(DEV)
    cen, sc = torch.from_numpy(np.asarray(center, dtype=np.float64)).to(DEV), torch.from_numpy(np.asarray(scale, dtype=np.float64)).to(DEV)
    c_d = torch.from_numpy(c).to(DEV) if g["C"] > 0 else None
    xb = torch.full((R.xb_elems(g["rows_alloc"], g["Kx"]),), float("nan"), dtype=torch.bfloat16, device=DEV)
    xf = torch.full((g["rows_alloc"], g["x_pitch"]), float("nan"), dtype=torch.float32, device=DEV)
    cz = torch.full((g["rows_alloc"], g["Cz"]), float("nan"), dtype=torch.bfloat16, device=DEV)
    _lib.check(lib.nm_pack_table_raw(ptrs.data_ptr(), widths.data_ptr(), len(srcs), rows_d.data_ptr(), g["N"], cen.data_ptr(),
                                     sc.data_ptr(), c_d.data_ptr() if c_d is not None else None, g["rows_alloc"], g["D"], g["C"],
                                     g["Kx"], xb.data_ptr(), xf.data_ptr(), g["x_pitch"], cz.data_ptr(), g["Cz"], None),
               "nm_pack_table_raw")
    torch.cuda.synchronize()
    return _u16(xb), xf.cpu().numpy(), _u16(cz)


@pytest.mark.parametrize("N,D,C", CASES)
def test_raw_pack_unscaled_against_the_plain_layout(N, D, C):
    """fp64 sources that hold the fp32 values exactly, center 0, scale 1: the cast gives x back, bit for bit."""
    x, c = R.pack_case(N, D, C)
    g = R.geometry(N, D, C)
    xb, xf, cz = _raw_pack([x.astype(np.float64)], np.arange(N), np.zeros(D), np.ones(D), c, g)
    assert R.compare_packed(xb, xf, cz, x, c) == []


@pytest.mark.parametrize("N,D,C", CASES)
def test_raw_pack_scaled_gathered_and_fused(N, D, C):
    """Non-trivial center / scale, two source tables side by side (early fusion), rows gathered with repeats from a larger
    cohort: expected x_f32 is ((x - center) / scale).astype(float32) in numpy."""
    _, c = R.pack_case(N, D, C)
    g = R.geometry(N, D, C)
    rng = np.random.default_rng(N * 131 + D)
    n_all = N + 5
    raw = rng.standard_normal((n_all, D)) * rng.lognormal(0.0, 2.0, size=D) + rng.normal(0.0, 3.0, size=D)
    center, scale = rng.normal(0.0, 3.0, size=D), rng.lognormal(0.0, 1.0, size=D)
    center[0], scale[0] = 0.0, 1.0
    rows = rng.integers(0, n_all, size=N)
    raw[rows[-1], 0], raw[rows[N // 2], 1], raw[rows[0], 0] = -0.0, 3.5e38, 1e-40      # (kept as they are by column 0: an fp32 subnormal)
    with np.errstate(over="ignore"):
        x = ((raw[rows] - center) / scale).astype(np.float32)
    d0 = max(1, D // 3)
    xb, xf, cz = _raw_pack([raw[:, :d0], raw[:, d0:]], rows, center, scale, c, g)
    assert R.compare_packed(xb, xf, cz, x, c) == []


@pytest.mark.parametrize("n", [257, 513])
def test_subnormal_survives_the_whole_device_path(n):
    """A column with odd n, median exactly 0, IQR exactly 1 and one entry 1e-40: the scaled value is the fp32 subnormal
    with the bit pattern 71362 on the host; a flush to zero anywhere on the device path (the sort keys, the fp64
    arithmetic, the cast, the bf16 conversion) would lose it."""
    q = (n - 1) // 4
    col = np.concatenate([np.full(q + 1, -0.5), np.full(q - 1, -0.25), [0.0, 1e-40], np.full(q - 2, 0.25), np.full(q + 1, 0.5)])
    assert col.size == n
    rng = np.random.default_rng(n)
    col = col[rng.permutation(n)]
    x = rng.standard_normal((n, 6))
    x[:, 2] = col
    cohort = prep.SyntheticCohort(iid=np.arange(100001, 100001 + n), age=rng.integers(22, 37, n).astype(np.float64),
                                  gender=rng.integers(0, 2, n).astype(np.float64), dia=np.ones(n, np.int64), fi=np.zeros(n), x={"fMRI": x})
    rows = np.arange(n)
    center, scale = prep.robust_scaler_fit(x)
    assert center[2] == 0.0 and scale[2] == 1.0
    (xh,), ch = prep.fold_train_tables(cohort, ["fMRI"], rows)
    at = int(np.flatnonzero(col == 1e-40)[0])
    assert xh[at, 2].view(np.uint32) == 71362
    dc = DeviceCohort(cohort, DEV)
    cd, sd = dc.scaler_fit("fMRI", torch.from_numpy(rows.astype(np.int32)).to(DEV))
    assert np.array_equal(cd.cpu().numpy(), center) and np.array_equal(sd.cpu().numpy(), scale)
    (t,) = dc.fold_tables(["fMRI"], rows)
    torch.cuda.synchronize()
    assert int(t.x_f32[at, 2].cpu().view(torch.int32)) == 71362
    assert R.compare_packed(_u16(t.xb), t.x_f32.cpu().numpy(), _u16(t.cz), xh, ch) == []
    assert int(t.packed_rows()[at, 2].cpu().view(torch.int16)) == 1       # (71362 >> 16, nothing to round: the smallest bf16 subnormal)
