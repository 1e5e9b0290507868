// ---------------------------------------------------------------------------------------------------------------------
// nm_chart_kernel / nm_chart_merge_kernel -- the normative chart pass: nm_decode_kernel's grid request with the loop over
// the cells (and over the decoders) turned into grid dimensions, and the per-cell moments of x_hat folded in the output
// epilogue (nmhip.h states the definition).  The sources of the kernels above stay as they are (this file is included at
// the end of nm_devpass.hip): the decoder loop body and the output-chunk epilogue are repeated here for ONE (cell, decoder).
//
// A workgroup owns one (128-row tile, cell g, decoder m) of a job: blockIdx = (job, tile, g * NM_MAX_EXP + m); the
// workgroups of decoders the job does not have, of cells the request does not have and of decoders that want nothing
// leave at once.  LDS: nm_decode_kernel's plan (P, W, two vector slots, scalars, Z [128][32] bf16).  With one decoder per
// workgroup dec_build_zc runs once, and behind the first hidden layer's opening barrier nobody reads Z again: its 8 KB
// become the two [8 waves][64 columns] fp64 merge areas of the fold (the sums, the squared deviations), 4 KB each.
//
// Fold of one 64-ROI chunk, per column, fp64 from the conversion of the fp32 x_hat on, contraction off:
//   1. wave w: butterfly over its 16 row lanes (xor 1, 2, 4, 8) of the values, rows past the request's end adding +0 -- run
//      as a reduce-scatter over the lane's 16 values (ch_rscatter: the same tree, 15 exchanges for 64), which leaves the
//      total of one column with each lane -> sum area [w][column]; barrier
//   2. each lane for its own column: S = area[0] + area[1] + ... over the tile's live waves in wave order, mean_t = S / live;
//      the 16 lanes of a group hand each other their means; butterfly of (x_hat - mean_t)^2, dead rows +0 -> M2 area
//      [w][column]; barrier
//   3. thread `column` of wave 0: S and mean_t once more (the same operations: the same bits), M2_t = the M2 area over the
//      live waves in wave order; (mean_t, M2_t) -> part[m][g][tile][column], one 16-byte store
// The next chunk's first barrier separates step 3's reads from the next writes of either area.
//
// nm_chart_merge_kernel: block (job, cell, decoder), thread per column; tiles in ascending order (ch_merge_step).
namespace {

constexpr int CH_AREA_BYTES = 8 * OCH * 8;                              // [8 waves][64 columns] fp64
static_assert(2 * CH_AREA_BYTES <= DVM_Z_BYTES, "the fold's merge areas live in Z");
constexpr int DVC_SMEM = DVM_SMEM;
static_assert(2 * DVC_SMEM <= 160 * 1024, "two workgroups per CU");

// The butterfly over the 16 row lanes (xor 1, 2, 4, 8) of 16 values at once, as a reduce-scatter: at every level a lane keeps
// the half of its values whose index bit equals its own lane bit and takes the partner's partial sums of exactly those, so 15
// exchanges do the work of 64 and lane c16 ends with the wave's total of value j = c16.  The tree of additions is the
// butterfly's -- level k adds the partial sums of lanes l and l ^ k -- only the order of the two operands differs from lane
// to lane, and IEEE addition commutes: the same bits as v = v + v[lane ^ k] on every value (tests/chart_ref.py: _bfly).
__device__ __forceinline__ double ch_rscatter(const double (&v)[16], int c16) {
#pragma clang fp contract(off)
  const bool b0 = (c16 & 1) != 0, b1 = (c16 & 2) != 0, b2 = (c16 & 4) != 0, b3 = (c16 & 8) != 0;
  double a[8], b[4], d[2];
#pragma unroll
  for (int i = 0; i < 8; ++i) {                    // a[i]: value 2 i + b0 over lanes {l, l ^ 1}
    const double keep = b0 ? v[2 * i + 1] : v[2 * i], send = b0 ? v[2 * i] : v[2 * i + 1];
    a[i] = keep + __shfl_xor(send, 1, 64);
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {                    // b[i]: value 4 i + 2 b1 + b0 over four lanes
    const double keep = b1 ? a[2 * i + 1] : a[2 * i], send = b1 ? a[2 * i] : a[2 * i + 1];
    b[i] = keep + __shfl_xor(send, 2, 64);
  }
#pragma unroll
  for (int i = 0; i < 2; ++i) {                    // d[i]: value 8 i + 4 b2 + 2 b1 + b0 over eight lanes
    const double keep = b2 ? b[2 * i + 1] : b[2 * i], send = b2 ? b[2 * i] : b[2 * i + 1];
    d[i] = keep + __shfl_xor(send, 4, 64);
  }
  const double keep = b3 ? d[1] : d[0], send = b3 ? d[0] : d[1];
  return keep + __shfl_xor(send, 8, 64);           // value c16 over the 16 lanes
}
__device__ __forceinline__ double ch_waves(const double* area, int col, int nw) {
#pragma clang fp contract(off)
  double s = area[col];
  for (int w = 1; w < nw; ++w) s = s + area[w * OCH + col];
  return s;
}
__device__ __forceinline__ double ch_sqdev(float xh, double mean) {
#pragma clang fp contract(off)
  const double d = (double)xh - mean;
  return d * d;
}
// the pairwise update of (n_a, mean, M2) with a tile (n_b, mean_b, M2_b); the counts are exact in fp64
__device__ __forceinline__ void ch_merge_step(double na, double& mean, double& m2, double nb, double mb, double m2b) {
#pragma clang fp contract(off)
  const double n = na + nb;
  const double delta = mb - mean;
  mean = mean + (delta * nb) / n;
  m2 = (m2 + m2b) + ((delta * delta) * (na * nb)) / n;
}

__device__ __forceinline__ bool ch_request_bad(const nm_chart_t* rq) {
  const int n_rows = rq->n_rows, ralloc = rq->rows_alloc, n_cells = rq->n_cells;
  return n_rows < 1 || n_rows > NM_CHART_MAX_ROWS || ralloc < n_rows || ralloc % TROWS != 0 || n_cells < 1 ||
         n_cells > NM_MAX_CELLS || !rq->z || !rq->cgrid;
}

__global__ __launch_bounds__(WG, 4) void nm_chart_kernel(const nm_job_t* __restrict__ jobs, const nm_chart_t* __restrict__ reqs,
                                                           int tile0) {
  constexpr int ROWS = DV_ROWS;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const nm_job_t* J = jobs + blockIdx.x;
  const nm_chart_t* const rq = reqs + blockIdx.x;
  if (dec_refused(J)) return;
  if (ch_request_bad(rq)) return;
  const int n_rows = rq->n_rows, ralloc = rq->rows_alloc, n_cells = rq->n_cells;
  const int g = (int)blockIdx.z / NM_MAX_EXP, m = (int)blockIdx.z % NM_MAX_EXP;
  if (g >= n_cells || m >= J->M) return;
  const nm_modality_t& md = J->mod[m];
  const int D = md.D, xp = md.x_pitch;
  GAS double* opart = asg(rq->part[m]);
  gf32 oloc = asg(rq->loc[m]);
  if (!opart && !oloc) return;                     // (workgroup-uniform) nothing of this decoder is wanted
  const int t128 = tile0 + (int)blockIdx.y;
  const int row0 = t128 * ROWS;
  if (oloc) oloc += (int64_t)g * ralloc * xp;
  if (row0 >= n_rows) {
    // the second half of a ragged last 256-row tile: the cell's loc rows come back as zeros (tiles beyond it are not this
    // request's; a tile without a row has no partial: the merge never asks for it)
    if (oloc && row0 < (n_rows + TROWS - 1) / TROWS * TROWS)
      dvs_zero_dead_rows((int)threadIdx.x, xp, oloc, (gf32)nullptr, (gf32)nullptr, row0, 0);
    return;
  }
  if (opart) opart += (((int64_t)g * (ralloc / ROWS) + t128) * xp) * 2;
  Ctx c;
  c.job = J;
  c.part = -1; c.nparts = 1; c.lstep = 0;
  c.slope = J->act_slope;
  dv_carve(c, smem);
  relaunder(c);
  c.flags = NM_F_EXPORT;
  c.t_last = 0;
  c.ws = nullptr;
  for (int i = c.tid; i < DVM_SMEM / 4; i += WG) reinterpret_cast<uint32_t*>(smem)[i] = 0u;
  __syncthreads();
  c.row0 = row0;
  c.rloc0 = row0 % TROWS;
  c.nrows = min(ROWS, n_rows - row0);
  c.inv_b = 1.0f / (float)c.nrows;
  const int live = c.nrows;
  const int L = J->L, Z = J->Z, C = J->C;
  const bool nl = J->non_linear != 0;
  const bool vec4 = (Z & 3) == 0;
  GAS char* const wsh = (GAS char*)J->wsh;
  char* const Wb = reinterpret_cast<char*>(c.Q);
  __bf16* const zlds = reinterpret_cast<__bf16*>(smem + DV_SMEM);
  double* const asum = reinterpret_cast<double*>(smem + DV_SMEM);                  // (Z, once dec_build_zc has been read)
  double* const asq = reinterpret_cast<double*>(smem + DV_SMEM + CH_AREA_BYTES);
  auto to_W = [&](const GAS char* blob, int vs, int rows, int K) {
    return Next{blob, Wb, IMG_BYTES >> 10, blob + cimg_bytes(rows, K), reinterpret_cast<char*>(c.vec) + vs * VEC_BYTES, rows, blob_kp(K)};
  };
  // W and P are free: the decoder's first image lands while z is converted
  issue_next(c, to_W(wsh + md.dec_s[0], 0, J->H[L - 1], Z + C));

  // ---- z: fp32 rows -> bf16 [128][32] in LDS; rows past the request's end hold zeros ----
  {
    gcf32 zg = asg(rq->z) + (int64_t)row0 * Z;
    if (vec4) {
      const int nq4 = Z >> 2;
      const float rq4 = 1.0f / (float)nq4;
#pragma unroll 2
      for (int e = c.tid; e < ROWS * nq4; e += WG) {
        const int r = idiv(e, nq4, rq4), z0 = 4 * (e - r * nq4);
        f32x4 v = f32x4{0.f, 0.f, 0.f, 0.f};
        if (r < live) v = *(const GAS f32x4*)(zg + (int64_t)r * Z + z0);
        bf16x4 zk;
#pragma unroll
        for (int i = 0; i < 4; ++i) zk[i] = (__bf16)v[i];
        *reinterpret_cast<bf16x4*>(zlds + r * 32 + z0) = zk;
      }
    } else {
      const float rZ = 1.0f / (float)Z;
#pragma unroll 2
      for (int e = c.tid; e < ROWS * Z; e += WG) {
        const int r = idiv(e, Z, rZ), z = e - r * Z;
        const float v = r < live ? zg[(int64_t)r * Z + z] : 0.f;
        zlds[r * 32 + z] = (__bf16)v;
      }
    }
  }
  lds_barrier();                                   // z is complete (the decoder image requested above stays in flight)

  // ---- the cell's decoder ----
  const int Hl = J->H[0];
  const int ob = L & 1;                            // (see nm_devpass_kernel: chunk 0's vectors avoid the last hidden layer's bias)
  relaunder(c);
  dec_build_zc(c, c.P, asg(rq->cgrid) + (int64_t)g * md.Cz, 0, Z, C, zlds);
  int vs = 0;
  const GAS char* oblob = wsh + md.out_s;
  const int nck = (D + OCH - 1) / OCH;
  auto out_blob = [&](int ch) {
    return Next{oblob + (int64_t)ch * OBLOB_BYTES, Wb + (ch & 1) * OIMG_BYTES, OIMG_BYTES >> 10,
                oblob + (int64_t)ch * OBLOB_BYTES + OIMG_BYTES, reinterpret_cast<char*>(c.vec) + ((ch + ob) & 1) * VEC_BYTES, 0, 0};
  };
  for (int d = 0; d < L; ++d) {
    const int Kin = (d == 0) ? Z + C : J->H[L - d], Nout = J->H[L - 1 - d];
    const Next nx = (d + 1 < L) ? to_W(wsh + md.dec_s[d + 1], vs ^ 1, J->H[L - 2 - d], Nout) : out_blob(0);
    dv_layer(c, vs, nx, Nout, Kin, nl, live);      // (its first barrier also publishes z | c | 1: Z is free behind it)
    vs ^= 1;
  }
  // output layer in 64-ROI chunks, wave w owns rows [16 w, 16 w + 16) and all 64 columns: see nm_devpass_kernel
  const int orow = c.wave * 16 + c.c16;
  const bool wave_live = c.wave * 16 < live;
  const bool rv = orow < c.nrows;
  const int nw = (live + 15) >> 4;                 // the tile's live waves
  const double dlive = (double)live;
  int stores_prev = 0;
  for (int ch = 0; ch < nck; ++ch) {
    relaunder(c);
    const int d0 = ch * OCH;
    const int cown = (c.c16 >> 2) * 16 + 4 * c.g + (c.c16 & 3);      // the chunk column whose wave totals this lane ends up with
    const __bf16* Wc = reinterpret_cast<const __bf16*>(Wb + (ch & 1) * OIMG_BYTES);
    const float* vb = c.vec + ((ch + ob) & 1) * (VEC_BYTES / 4);
    wait_vm(ch > 0 ? stores_prev : 0);
    lds_barrier();
    if (ch + 1 < nck) issue_next(c, out_blob(ch + 1));
    stores_prev = 0;
    f32x4 lo[4];
#pragma unroll
    for (int ft = 0; ft < 4; ++ft) lo[ft] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (wave_live) {
      f32x4 acc[4];
#pragma unroll
      for (int ft = 0; ft < 4; ++ft) acc[ft] = f32x4{0.f, 0.f, 0.f, 0.f};
      const int ksteps = wpad(Hl) / 32;
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) {
        if (ks < ksteps) {
          const bf16x8 a = lds_frag(c.P, LDP, orow, ks * 32 + 8 * c.g);
#pragma unroll
          for (int ft = 0; ft < 4; ++ft) acc[ft] = mfma(lds_frag(Wc, LDP, ft * 16 + c.c16, ks * 32 + 8 * c.g), a, acc[ft]);
        }
      }
      const bool full = live == ROWS && d0 + OCH <= D;                   // no row / column masks needed (wave-uniform)
#pragma unroll
      for (int ft = 0; ft < 4; ++ft) {
        const int dg0 = d0 + ft * 16 + 4 * c.g;
        const f32x4 bo = *reinterpret_cast<const f32x4*>(vb + ft * 16 + 4 * c.g);
        if (full) {
          lo[ft] = acc[ft] + bo;
        } else {
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const float xh = acc[ft][i] + bo[i];
            const bool dv = rv && dg0 + i < D;
            lo[ft][i] = dv ? xh : 0.f;
          }
        }
        if (oloc && d0 + ft * 16 < xp) {                // wave-uniform
          if (dg0 < xp) *(GAS f32x4*)(oloc + (int64_t)(row0 + orow) * xp + dg0) = lo[ft];
          stores_prev += 1;
        }
      }
      if (opart) {                                  // step 1: the wave's column sums (dead rows and pad columns hold +0)
        double v[16];
#pragma unroll
        for (int j = 0; j < 16; ++j) v[j] = (double)lo[j >> 2][j & 3];
        asum[c.wave * OCH + cown] = ch_rscatter(v, c.c16);
      }
    }
    if (!opart) continue;                           // (workgroup-uniform)
    lds_barrier();                                  // the sums of every live wave are in place
    if (wave_live) {                                // step 2: tile mean, the wave's squared deviations
      // the mean of the lane's own column once, the 16 columns of its row from the 16 lanes of its group
      const double mown = ch_waves(asum, cown, nw) / dlive;
      double q[16];
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        const double mean = __shfl(mown, (c.lane & 48) | j, 64);
        const bool dv = rv && d0 + (j >> 2) * 16 + 4 * c.g + (j & 3) < D;
        q[j] = dv ? ch_sqdev(lo[j >> 2][j & 3], mean) : 0.0;
      }
      asq[c.wave * OCH + cown] = ch_rscatter(q, c.c16);
    }
    lds_barrier();                                  // the squared deviations of every live wave are in place
    if (c.tid < OCH && d0 + c.tid < xp) {           // step 3: one thread per column
      const double mean = ch_waves(asum, c.tid, nw) / dlive;
      const double m2 = ch_waves(asq, c.tid, nw);
      typedef double d64x2 __attribute__((ext_vector_type(2)));
      *(GAS d64x2*)(opart + (int64_t)(d0 + c.tid) * 2) = d64x2{mean, m2};
    }
  }
  // (a ragged tile only: the loc rows no wave has stored)
  if (oloc && live < ROWS) { relaunder(c); dvs_zero_dead_rows(c.tid, xp, oloc, (gf32)nullptr, (gf32)nullptr, row0, live); }
}

// block (job, cell, decoder), thread per column: the tile partials of the column in ascending tile order -> the chart row
__global__ __launch_bounds__(256) void nm_chart_merge_kernel(const nm_job_t* __restrict__ jobs, const nm_chart_t* __restrict__ reqs,
                                                              int n_tiles) {
  const nm_job_t* J = jobs + blockIdx.x;
  const nm_chart_t* const rq = reqs + blockIdx.x;
  if (dec_refused(J)) return;
  if (ch_request_bad(rq)) return;
  const int n_rows = rq->n_rows, g = (int)blockIdx.y, m = (int)blockIdx.z;
  if (g >= rq->n_cells || m >= J->M || (int64_t)n_tiles * DV_ROWS < n_rows) return;
  const GAS double* part = asg(rq->part[m]);
  GAS double* chart = asg(rq->chart[m]);
  if (!part || !chart) return;
  const int D = J->mod[m].D, xp = J->mod[m].x_pitch;
  const int T = (n_rows + DV_ROWS - 1) / DV_ROWS, tiles_alloc = rq->rows_alloc / DV_ROWS;
  part += (int64_t)g * tiles_alloc * xp * 2;
  chart += (int64_t)g * xp * NM_CHART_COLUMNS;
  for (int col = (int)threadIdx.x; col < xp; col += (int)blockDim.x) {
    double o_mean = 0.0, o_var = 0.0, o_n = 0.0, o_st = 0.0;
    if (col < D) {
      double na = (double)min(DV_ROWS, n_rows);
      double mean = part[(int64_t)col * 2], m2 = part[(int64_t)col * 2 + 1];
      for (int t = 1; t < T; ++t) {
        const double nb = (double)min(DV_ROWS, n_rows - t * DV_ROWS);
        const GAS double* p = part + ((int64_t)t * xp + col) * 2;
        ch_merge_step(na, mean, m2, nb, p[0], p[1]);
        na = na + nb;
      }
      o_n = na;
      if (n_rows < 2 || !isfinite(mean)) {
        o_mean = o_var = __builtin_nan(""); o_st = -2.0;
      } else {
        o_mean = mean; o_var = m2 / (na - 1.0);
      }
    }
    GAS double* o = chart + (int64_t)col * NM_CHART_COLUMNS;
    o[0] = o_mean; o[1] = o_var; o[2] = o_n; o[3] = o_st;
  }
}

}  // namespace

extern "C" {

/* 0: the job's chart can run on nm_chart_pass: exactly what nm_decode_pass_ok admits; NM_E_DEVPASS otherwise. */
int nm_chart_pass_ok(const nm_job_t* j) {
  if (!j) return NM_E_NULL;
  return dec_refused(j);
}

/* The chart pass over rows [tile0 * 128, (tile0 + n_tiles) * 128) of every job's request (nmhip.h: nm_chart_t): the fold,
 * then -- tile0 == 0 only, and per request only where n_tiles covers its rows -- the merge on the same stream.  Status is
 * decided here, on the host, before the device is asked anything: the descriptors and the requests live in device memory. */
int nm_chart_pass(const nm_job_t* jobs_dev, int n_jobs, const nm_chart_t* req_dev, int tile0, int n_tiles, int max_cells, int flags,
                  void* stream) {
  (void)flags;
  if (!jobs_dev || !req_dev) return NM_E_NULL;
  if (int bad = check_launch_geometry(jobs_dev, n_jobs, n_tiles, 1, tile0, 0)) return bad;
  if (max_cells < 1 || max_cells > NM_MAX_CELLS || n_tiles > 65535) return NM_E_GEOMETRY;
  if (int bad = launch_kernel(nm_chart_kernel, dim3(n_jobs, n_tiles, max_cells * NM_MAX_EXP), dim3(WG), DVC_SMEM, stream, jobs_dev,
                              req_dev, tile0))
    return bad;
  if (tile0 != 0) return NM_OK;
  return launch_kernel(nm_chart_merge_kernel, dim3(n_jobs, max_cells, NM_MAX_EXP), dim3(256), 0, stream, jobs_dev, req_dev, n_tiles);
}

}  // extern "C"
