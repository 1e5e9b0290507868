// nm_normative.inc -- normative z-maps on the device (included at the end of nm_metrics.hip; include/nmhip.h has the
// definitions): nm_cohort_moments, nm_normative_z, nm_cohort_cov, nm_mahalanobis.
//
//   moments  one workgroup per (set, 64-column tile), a lane per column: a wave reads 64 consecutive floats of a row.  The
//            four waves take every fourth row, four rows at a time so that four loads are in flight, and add in row order;
//            the waves' partials are merged through LDS in wave order by every wave alike, so all of them hold the column's
//            mean for the second pass without another hand-off.  Pass 1: n_ref, the non-finite count, sum, min, max; pass 2
//            (the tile comes from L2 this time): sum (v - mean)^2 and sum (v - mean), var = (M2 - c^2 / n) / (n - ddof).
//   z rows   one workgroup per (set, NM_NORM_ROWS_PER_WG rows): mean and sd of the D columns staged once in LDS (sd = NaN
//            marks a column without valid moments), then a wave per row, a lane per column lane, lane + 64, ...: the fp32
//            z is stored as it is made (coalesced), the row's counts and sums stay in the lane and the 64 lanes are merged
//            by an xor butterfly (a + b == b + a bit for bit, so every lane ends with the same sum of a fixed shape).
//   z cols   the moments kernel's grid and row walk with mean and sd of the lane's column in registers; counts are int32.
//   cov      one workgroup per set, the Z x Z matrix in dynamic LDS.  Column means by a thread per column in row order; the
//            lower triangle in 4 x 4 blocks, a block at a time per thread with its 16 sums in named registers, the rows in
//            row order; then Cholesky column by column: thread i owns row i, the pivot goes through a two-slot LDS word so a
//            column costs two barriers.
//   maha     a thread per row, the solved vector y in LDS as [k][thread] (conflict-free), L read at addresses the whole
//            wave shares.
// No kernel indexes a register array at run time (the unrolled four-row batches and the 4 x 4 block are indexed by constants).

namespace {

constexpr int NORM_TILE = 64;                      // columns per workgroup of the moments and the column pass
constexpr int NORM_WAVES = MT / 64;
constexpr int NORM_RB = 4;                         // rows a wave has in flight
constexpr int NORM_RW = NM_NORM_ROWS_PER_WG;
constexpr int MAHA_T = 64;                         // rows (threads) per workgroup of the distance pass
static_assert(sizeof(nm_norm_set_t) == 56, "nm_norm_set_t is mirrored by _lib.NmNormSet");
static_assert(NM_NORM_MAX_D * 16 <= 64 * 1024, "the rows pass stages mean and sd of every column");
static_assert(NM_WIDE_MAX_LATENT * (NM_WIDE_MAX_LATENT + 1) * 8 + (NM_WIDE_MAX_LATENT + 2) * 8 <= 160 * 1024, "the covariance lives in LDS");
static_assert(NM_WIDE_MAX_LATENT <= MT, "a thread per column and per factor row");

__device__ __forceinline__ double norm_nan() { return __longlong_as_double(0x7FF8000000000000ll); }
__device__ __forceinline__ bool norm_finite(double v) { return fabs(v) <= 1.7976931348623157e308; }   // false for NaN

// the table entry's own checks: what a kernel may read of the set (width = D or Z)
__device__ __forceinline__ bool norm_set_ok(const nm_norm_set_t& S, int width, int max_rows, bool needs_group) {
  if (S.rows < 0 || S.rows > max_rows || S.pitch < width) return false;
  if (S.sub && S.sub_pitch < width) return false;
  if (S.rows > 0 && (!S.x || (needs_group && !S.group))) return false;
  return true;
}

__device__ __forceinline__ double norm_value(const nm_norm_set_t& S, int r, int c) {
  double v = (double)S.x[(int64_t)r * S.pitch + c];
  if (S.sub) v -= (double)S.sub[(int64_t)r * S.sub_pitch + c];
  return v;
}

__global__ __launch_bounds__(MT) void cohort_moments_kernel(const nm_norm_set_t* __restrict__ sets, int D, int max_rows, int tiles,
                                                            int ddof, double* __restrict__ out) {
  __shared__ double pd[3][NORM_WAVES * NORM_TILE];
  __shared__ int32_t pi[2][NORM_WAVES * NORM_TILE];
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  const int s = blockIdx.x / tiles, tile = blockIdx.x - s * tiles;
  const nm_norm_set_t S = sets[s];
  const int col = tile * NORM_TILE + lane;
  const bool cv = col < D;
  double* o = out + ((int64_t)s * D + col) * NM_METRICS_STRIDE;
  const double qnan = norm_nan();
  if (!norm_set_ok(S, D, max_rows, true)) {
    if (w == 0 && cv) {
      o[0] = qnan; o[1] = qnan; o[2] = qnan; o[3] = 0.0; o[4] = qnan; o[5] = qnan; o[6] = 0.0; o[7] = -2.0;
    }
    return;
  }
  const int rows = S.rows;
  double sum = 0.0, mn = INFINITY, mx = -INFINITY;
  int n = 0, nbad = 0;
  for (int r0 = w; r0 < rows; r0 += NORM_WAVES * NORM_RB) {
    double v[NORM_RB];
    bool in[NORM_RB];
#pragma unroll
    for (int k = 0; k < NORM_RB; ++k) {
      const int r = r0 + NORM_WAVES * k;
      in[k] = r < rows && S.group[min(r, rows - 1)] == 0;
      v[k] = (in[k] && cv) ? norm_value(S, r, col) : 0.0;
    }
#pragma unroll
    for (int k = 0; k < NORM_RB; ++k)
      if (in[k]) {
        ++n;
        if (norm_finite(v[k])) { sum += v[k]; mn = fmin(mn, v[k]); mx = fmax(mx, v[k]); }
        else ++nbad;
      }
  }
  pd[0][t] = sum; pd[1][t] = mn; pd[2][t] = mx; pi[0][t] = n; pi[1][t] = nbad;
  __syncthreads();
  int N = 0, NB = 0;
  double SUM = 0.0, MN = INFINITY, MX = -INFINITY;
  for (int q = 0; q < NORM_WAVES; ++q) {
    const int i = q * NORM_TILE + lane;
    N += pi[0][i]; NB += pi[1][i]; SUM += pd[0][i]; MN = fmin(MN, pd[1][i]); MX = fmax(MX, pd[2][i]);
  }
  const double mean = SUM / (double)N;               // (every wave: the same bits)
  double m2 = 0.0, c1 = 0.0;
  if (N > ddof) {                                     // (N is the set's: the same for every thread)
    for (int r0 = w; r0 < rows; r0 += NORM_WAVES * NORM_RB) {
      double v[NORM_RB];
      bool in[NORM_RB];
#pragma unroll
      for (int k = 0; k < NORM_RB; ++k) {
        const int r = r0 + NORM_WAVES * k;
        in[k] = r < rows && S.group[min(r, rows - 1)] == 0;
        v[k] = (in[k] && cv) ? norm_value(S, r, col) : 0.0;
      }
#pragma unroll
      for (int k = 0; k < NORM_RB; ++k)
        if (in[k]) { const double d = v[k] - mean; m2 += d * d; c1 += d; }
    }
  }
  __syncthreads();                                   // pass 1's partials are read
  pd[0][t] = m2; pd[1][t] = c1;
  __syncthreads();
  if (w == 0 && cv) {
    double M2 = 0.0, C1 = 0.0;
    for (int q = 0; q < NORM_WAVES; ++q) { M2 += pd[0][q * NORM_TILE + lane]; C1 += pd[1][q * NORM_TILE + lane]; }
    double var = (M2 - C1 * C1 / (double)N) / (double)(N - ddof);
    if (var < 0.0) var = 0.0;
    const bool ok = N > ddof && NB == 0 && MX > MN;     // (a constant column is told by min == max, not by a rounded sum)
    o[0] = ok ? mean : qnan;
    o[1] = ok ? sqrt(var) : qnan;
    o[2] = ok ? var : qnan;
    o[3] = (double)N;
    o[4] = (N - NB > 0) ? MN : qnan;
    o[5] = (N - NB > 0) ? MX : qnan;
    o[6] = (double)NB;
    o[7] = ok ? 0.0 : -2.0;
  }
}

__global__ __launch_bounds__(MT) void normative_rows_kernel(const nm_norm_set_t* __restrict__ sets, int D, int max_rows, int chunks,
                                                            const double* __restrict__ moments, int n_moments,
                                                            const int32_t* __restrict__ ref_of, double thr,
                                                            double* __restrict__ rows_out) {
  extern __shared__ __attribute__((aligned(16))) double nlds[];       // mean [D], sd [D]
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  const int s = blockIdx.x / chunks, chunk = blockIdx.x - s * chunks;
  const nm_norm_set_t S = sets[s];
  const int rows = S.rows;
  if (rows < 0 || rows > max_rows) return;           // no rows to write
  const int r_begin = chunk * NORM_RW;
  if (r_begin >= rows) return;
  const int ref = ref_of ? ref_of[s] : s;
  const bool ok = norm_set_ok(S, D, max_rows, false) && (!S.z || S.z_pitch >= D) && ref >= 0 && ref < n_moments;
  const double qnan = norm_nan();
  double* mean_l = nlds;
  double* sd_l = nlds + D;
  if (ok) {
    const double* m = moments + (int64_t)ref * D * NM_METRICS_STRIDE;
    for (int c = t; c < D; c += MT) {
      const double st = m[(int64_t)c * NM_METRICS_STRIDE + 7], sd = m[(int64_t)c * NM_METRICS_STRIDE + 1];
      mean_l[c] = m[(int64_t)c * NM_METRICS_STRIDE];
      sd_l[c] = (st == 0.0 && sd > 0.0) ? sd : qnan;
    }
  }
  __syncthreads();
  for (int rr = w; rr < NORM_RW; rr += NORM_WAVES) {
    const int r = r_begin + rr;
    if (r >= rows) break;
    double* o = rows_out + ((int64_t)S.row_off + r) * NM_METRICS_STRIDE;
    if (!ok) {
      if (lane == 0) { o[0] = 0.0; o[1] = 0.0; o[2] = qnan; o[3] = qnan; o[4] = qnan; o[5] = -1.0; o[6] = 0.0; o[7] = -2.0; }
      continue;
    }
    int nhi = 0, nlo = 0, nv = 0, am = -1;
    double sz = 0.0, sa = 0.0, mz = -INFINITY;
    for (int c = lane; c < D; c += 64) {
      const double v = norm_value(S, r, c);
      const double sd = sd_l[c];
      const bool valid = norm_finite(v) && sd == sd;
      const double z = valid ? (v - mean_l[c]) / sd : qnan;
      if (S.z) S.z[(int64_t)r * S.z_pitch + c] = (float)z;
      if (valid) {
        nhi += z > thr; nlo += z < -thr; ++nv;
        sz += z; sa += fabs(z);
        if (am < 0 || z > mz) { mz = z; am = c; }
      }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
      nhi += __shfl_xor(nhi, off); nlo += __shfl_xor(nlo, off); nv += __shfl_xor(nv, off);
      sz += __shfl_xor(sz, off); sa += __shfl_xor(sa, off);
      const double oz = __shfl_xor(mz, off);
      const int oa = __shfl_xor(am, off);
      if (oa >= 0 && (am < 0 || oz > mz || (oz == mz && oa < am))) { mz = oz; am = oa; }
    }
    if (lane == 0) {
      o[0] = (double)nhi; o[1] = (double)nlo;
      o[2] = nv ? sz / (double)nv : qnan;
      o[3] = nv ? sa / (double)nv : qnan;
      o[4] = nv ? mz : qnan;
      o[5] = (double)am;
      o[6] = (double)nv;
      o[7] = nv ? 0.0 : -2.0;
    }
  }
}

__global__ __launch_bounds__(MT) void normative_cols_kernel(const nm_norm_set_t* __restrict__ sets, int D, int max_rows, int tiles,
                                                            const double* __restrict__ moments, int n_moments,
                                                            const int32_t* __restrict__ ref_of, double thr,
                                                            double* __restrict__ out) {
  __shared__ int32_t pc[6][NORM_WAVES * NORM_TILE];
  __shared__ double ps[2][NORM_WAVES * NORM_TILE];
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  const int s = blockIdx.x / tiles, tile = blockIdx.x - s * tiles;
  const nm_norm_set_t S = sets[s];
  const int col = tile * NORM_TILE + lane;
  const bool cv = col < D;
  double* o = out + ((int64_t)s * D + col) * NM_METRICS_STRIDE;
  const double qnan = norm_nan();
  const int ref = ref_of ? ref_of[s] : s;
  if (!norm_set_ok(S, D, max_rows, true) || ref < 0 || ref >= n_moments) {
    if (w == 0 && cv)
      for (int k = 0; k < NM_METRICS_STRIDE; ++k) o[k] = qnan;
    return;
  }
  double mean = 0.0, sd = qnan;
  if (cv) {
    const double* m = moments + ((int64_t)ref * D + col) * NM_METRICS_STRIDE;
    mean = m[0];
    if (m[7] == 0.0 && m[1] > 0.0) sd = m[1];
  }
  const bool mv = sd == sd;
  const int rows = S.rows;
  int hx = 0, lx = 0, hy = 0, ly = 0, nx = 0, ny = 0;
  double zx = 0.0, zy = 0.0;
  for (int r0 = w; r0 < rows; r0 += NORM_WAVES * NORM_RB) {
    double v[NORM_RB];
    int g[NORM_RB];
#pragma unroll
    for (int k = 0; k < NORM_RB; ++k) {
      const int r = r0 + NORM_WAVES * k;
      g[k] = r < rows ? S.group[min(r, rows - 1)] : -1;
      v[k] = ((g[k] == 0 || g[k] == 1) && mv) ? norm_value(S, r, col) : qnan;
    }
#pragma unroll
    for (int k = 0; k < NORM_RB; ++k)
      if (norm_finite(v[k])) {
        const double z = (v[k] - mean) / sd;
        const int hi = z > thr, lo = z < -thr;
        if (g[k] == 1) { hx += hi; lx += lo; ++nx; zx += z; }
        else { hy += hi; ly += lo; ++ny; zy += z; }
      }
  }
  pc[0][t] = hx; pc[1][t] = lx; pc[2][t] = hy; pc[3][t] = ly; pc[4][t] = nx; pc[5][t] = ny; ps[0][t] = zx; ps[1][t] = zy;
  __syncthreads();
  if (w == 0 && cv) {
    int c[6] = {0, 0, 0, 0, 0, 0};
    double ZX = 0.0, ZY = 0.0;
    for (int q = 0; q < NORM_WAVES; ++q) {
      const int i = q * NORM_TILE + lane;
#pragma unroll
      for (int k = 0; k < 6; ++k) c[k] += pc[k][i];
      ZX += ps[0][i]; ZY += ps[1][i];
    }
#pragma unroll
    for (int k = 0; k < 6; ++k) o[k] = (double)c[k];
    o[6] = (mv && c[4]) ? ZX / (double)c[4] : qnan;
    o[7] = (mv && c[5]) ? ZY / (double)c[5] : qnan;
  }
}

__global__ __launch_bounds__(MT) void cohort_cov_kernel(const nm_norm_set_t* __restrict__ sets, int Z, int max_rows, double ridge,
                                                        double* __restrict__ mean_out, double* __restrict__ chol_out,
                                                        int32_t* __restrict__ status_out) {
  extern __shared__ __attribute__((aligned(16))) double clds[];       // A [Z][P], mean [Z], pivot [2]
  const int P = Z | 1;                               // an odd row pitch: the threads of a column step read different banks
  double* A = clds;
  double* mean_l = clds + Z * P;
  double* piv = mean_l + Z;
  const int t = threadIdx.x, s = blockIdx.x;
  const nm_norm_set_t S = sets[s];
  double* mo = mean_out + (int64_t)s * Z;
  double* co = chol_out + (int64_t)s * Z * Z;
  const double qnan = norm_nan();
  const bool set_ok = norm_set_ok(S, Z, max_rows, true);
  const int rows = set_ok ? S.rows : 0;
  // column means: a thread per column, the rows in row order
  int n = 0, bad = 0;
  double sum = 0.0;
  for (int r = 0; r < rows; ++r) {
    if (S.group[r] != 0) continue;
    ++n;
    if (t < Z) {
      const double v = norm_value(S, r, t);
      if (norm_finite(v)) sum += v; else bad = 1;
    }
  }
  bad = __syncthreads_or(bad);
  const bool mean_ok = set_ok && n >= 1 && !bad;
  if (t < Z) {
    const double m = mean_ok ? sum / (double)n : qnan;
    mean_l[t] = m;
    mo[t] = m;
  }
  bool valid = mean_ok && n >= 2 && (ridge > 0.0 || n > Z);
  __syncthreads();
  if (valid) {
    // the lower triangle in 4 x 4 blocks: block (bi, bj), bj <= bi, is thread b's for b = bi * nb + bj = t, t + MT, ...
    const int nb = (Z + 3) / 4;
    const double inv = 1.0 / (double)(n - 1);
    for (int b = t; b < nb * nb; b += MT) {
      const int bi = b / nb, bj = b - bi * nb;
      if (bj > bi) continue;
      const int i0 = bi * 4, j0 = bj * 4;
      const int i1 = min(i0 + 1, Z - 1), i2 = min(i0 + 2, Z - 1), i3 = min(i0 + 3, Z - 1);
      const int j1 = min(j0 + 1, Z - 1), j2 = min(j0 + 2, Z - 1), j3 = min(j0 + 3, Z - 1);
      const double mi0 = mean_l[i0], mi1 = mean_l[i1], mi2 = mean_l[i2], mi3 = mean_l[i3];
      const double mj0 = mean_l[j0], mj1 = mean_l[j1], mj2 = mean_l[j2], mj3 = mean_l[j3];
      double a00 = 0, a01 = 0, a02 = 0, a03 = 0, a10 = 0, a11 = 0, a12 = 0, a13 = 0;
      double a20 = 0, a21 = 0, a22 = 0, a23 = 0, a30 = 0, a31 = 0, a32 = 0, a33 = 0;
      for (int r = 0; r < rows; ++r) {
        if (S.group[r] != 0) continue;
        const double x0 = norm_value(S, r, i0) - mi0, x1 = norm_value(S, r, i1) - mi1;
        const double x2 = norm_value(S, r, i2) - mi2, x3 = norm_value(S, r, i3) - mi3;
        const double y0 = norm_value(S, r, j0) - mj0, y1 = norm_value(S, r, j1) - mj1;
        const double y2 = norm_value(S, r, j2) - mj2, y3 = norm_value(S, r, j3) - mj3;
        a00 += x0 * y0; a01 += x0 * y1; a02 += x0 * y2; a03 += x0 * y3;
        a10 += x1 * y0; a11 += x1 * y1; a12 += x1 * y2; a13 += x1 * y3;
        a20 += x2 * y0; a21 += x2 * y1; a22 += x2 * y2; a23 += x2 * y3;
        a30 += x3 * y0; a31 += x3 * y1; a32 += x3 * y2; a33 += x3 * y3;
      }
      // (an index clamped to Z - 1 repeats the last column: its sums are dropped here)
#define NM_COV_PUT(di, dj, a)                                                                       \
      if (i0 + di < Z && j0 + dj < Z && j0 + dj <= i0 + di)                                         \
        A[(i0 + di) * P + (j0 + dj)] = (a) * inv + ((i0 + di) == (j0 + dj) ? ridge : 0.0);
      NM_COV_PUT(0, 0, a00) NM_COV_PUT(0, 1, a01) NM_COV_PUT(0, 2, a02) NM_COV_PUT(0, 3, a03)
      NM_COV_PUT(1, 0, a10) NM_COV_PUT(1, 1, a11) NM_COV_PUT(1, 2, a12) NM_COV_PUT(1, 3, a13)
      NM_COV_PUT(2, 0, a20) NM_COV_PUT(2, 1, a21) NM_COV_PUT(2, 2, a22) NM_COV_PUT(2, 3, a23)
      NM_COV_PUT(3, 0, a30) NM_COV_PUT(3, 1, a31) NM_COV_PUT(3, 2, a32) NM_COV_PUT(3, 3, a33)
#undef NM_COV_PUT
    }
    __syncthreads();
    double maxdiag = 0.0;
    for (int k = 0; k < Z; ++k) maxdiag = fmax(maxdiag, A[k * P + k]);
    const double tol = (double)Z * 2.220446049250313e-16 * maxdiag;
    // Cholesky, column by column: thread i holds row i; the pivot travels through piv[j & 1]
    for (int j = 0; j < Z; ++j) {
      double sij = 0.0;
      if (t >= j && t < Z) {
        sij = A[t * P + j];
        for (int k = 0; k < j; ++k) sij -= A[t * P + k] * A[j * P + k];
        if (t == j) piv[j & 1] = sij;
      }
      __syncthreads();
      const double d = piv[j & 1];
      if (!(d > tol)) { valid = false; break; }        // (d is the same for every thread; NaN ends here too)
      const double l = sqrt(d);
      if (t >= j && t < Z) A[t * P + j] = (t == j) ? l : sij / l;
      __syncthreads();
    }
  }
  __syncthreads();
  for (int e = t; e < Z * Z; e += MT) {
    const int i = e / Z, j = e - i * Z;
    co[e] = !valid ? qnan : (j <= i ? A[i * P + j] : 0.0);
  }
  if (t == 0) status_out[s] = valid ? 0 : -2;
}

__global__ __launch_bounds__(MAHA_T) void mahalanobis_kernel(const nm_norm_set_t* __restrict__ sets, int Z, int max_rows, int chunks,
                                                             const double* __restrict__ mean, const double* __restrict__ chol,
                                                             const int32_t* __restrict__ status, int n_factors,
                                                             const int32_t* __restrict__ ref_of, double* __restrict__ d2_out,
                                                             double* __restrict__ d_out) {
  extern __shared__ __attribute__((aligned(16))) double ylds[];       // y [Z][MAHA_T]
  const int t = threadIdx.x;
  const int s = blockIdx.x / chunks, chunk = blockIdx.x - s * chunks;
  const nm_norm_set_t S = sets[s];
  const int rows = S.rows;
  if (rows < 0 || rows > max_rows) return;           // no rows to write
  const int r = chunk * MAHA_T + t;
  if (r >= rows) return;                             // (no barrier below: a thread may leave alone)
  const int ref = ref_of ? ref_of[s] : s;
  const bool ok = norm_set_ok(S, Z, max_rows, false) && ref >= 0 && ref < n_factors && status[min(max(ref, 0), n_factors - 1)] == 0;
  const int64_t orow = (int64_t)S.row_off + r;
  const double qnan = norm_nan();
  if (!ok) { d2_out[orow] = qnan; d_out[orow] = qnan; return; }
  const double* L = chol + (int64_t)ref * Z * Z;
  const double* m = mean + (int64_t)ref * Z;
  double d2 = 0.0;
  bool bad = false;
  for (int k = 0; k < Z; ++k) {
    const double v = norm_value(S, r, k);
    bad |= !norm_finite(v);
    double acc = v - m[k];
    for (int j = 0; j < k; ++j) acc -= L[k * Z + j] * ylds[j * MAHA_T + t];
    const double yk = acc / L[k * Z + k];
    ylds[k * MAHA_T + t] = yk;
    d2 += yk * yk;
  }
  d2_out[orow] = bad ? qnan : d2;
  d_out[orow] = bad ? qnan : sqrt(d2);
}

inline bool norm_common_bad(int n_sets, int max_rows) { return n_sets < 1 || max_rows < 1 || max_rows > MAXN; }

}  // namespace

extern "C" {

int nm_cohort_moments(const nm_norm_set_t* sets_dev, int n_sets, int D, int max_rows, int ddof, double* out, void* stream) {
  if (!sets_dev || !out) return NM_E_NULL;
  if (norm_common_bad(n_sets, max_rows) || D < 1 || (ddof != 0 && ddof != 1)) return NM_E_METRICS;
  const int tiles = (D + NORM_TILE - 1) / NORM_TILE;
  if ((int64_t)n_sets * tiles > 0x7FFFFFFFll) return NM_E_METRICS;
  return launch_kernel(cohort_moments_kernel, dim3(n_sets * tiles), dim3(MT), 0, stream, sets_dev, D, max_rows, tiles, ddof, out);
}

int nm_normative_z(const nm_norm_set_t* sets_dev, int n_sets, int D, int max_rows, const double* moments, int n_moments,
                   const int32_t* ref_of, double thr, double* rows_out, double* cols_out, void* stream) {
  if (!sets_dev || !moments || !rows_out || !cols_out) return NM_E_NULL;
  if (norm_common_bad(n_sets, max_rows) || D < 1 || D > NM_NORM_MAX_D || n_moments < 1 || !(thr > 0.0) || !(thr < INFINITY))
    return NM_E_METRICS;
  const int tiles = (D + NORM_TILE - 1) / NORM_TILE, chunks = (max_rows + NORM_RW - 1) / NORM_RW;
  if ((int64_t)n_sets * tiles > 0x7FFFFFFFll || (int64_t)n_sets * chunks > 0x7FFFFFFFll) return NM_E_METRICS;
  int e = launch_kernel(normative_rows_kernel, dim3(n_sets * chunks), dim3(MT), D * 16, stream, sets_dev, D, max_rows, chunks,
                        moments, n_moments, ref_of, thr, rows_out);
  if (e) return e;
  return launch_kernel(normative_cols_kernel, dim3(n_sets * tiles), dim3(MT), 0, stream, sets_dev, D, max_rows, tiles, moments,
                       n_moments, ref_of, thr, cols_out);
}

int nm_cohort_cov(const nm_norm_set_t* sets_dev, int n_sets, int Z, int max_rows, double ridge, double* mean_out, double* chol_out,
                  int32_t* status_out, void* stream) {
  if (!sets_dev || !mean_out || !chol_out || !status_out) return NM_E_NULL;
  if (Z < 1 || Z > NM_WIDE_MAX_LATENT) return NM_E_LATENT;
  if (norm_common_bad(n_sets, max_rows) || !(ridge >= 0.0) || !(ridge < INFINITY)) return NM_E_METRICS;
  return launch_kernel(cohort_cov_kernel, dim3(n_sets), dim3(MT), (Z * (Z | 1) + Z + 2) * 8, stream, sets_dev, Z, max_rows, ridge, mean_out,
                       chol_out, status_out);
}

int nm_mahalanobis(const nm_norm_set_t* sets_dev, int n_sets, int Z, int max_rows, const double* mean, const double* chol,
                   const int32_t* status, int n_factors, const int32_t* ref_of, double* d2_out, double* d_out, void* stream) {
  if (!sets_dev || !mean || !chol || !status || !d2_out || !d_out) return NM_E_NULL;
  if (Z < 1 || Z > NM_WIDE_MAX_LATENT) return NM_E_LATENT;
  if (norm_common_bad(n_sets, max_rows) || n_factors < 1) return NM_E_METRICS;
  const int chunks = (max_rows + MAHA_T - 1) / MAHA_T;
  if ((int64_t)n_sets * chunks > 0x7FFFFFFFll) return NM_E_METRICS;
  return launch_kernel(mahalanobis_kernel, dim3(n_sets * chunks), dim3(MAHA_T), Z * MAHA_T * 8, stream, sets_dev, Z, max_rows, chunks,
                       mean, chol, status, n_factors, ref_of, d2_out, d_out);
}

}  // extern "C"
