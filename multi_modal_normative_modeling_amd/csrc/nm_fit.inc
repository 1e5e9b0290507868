// nm_fit.inc -- model fit per ROI on the device (included at the end of nm_metrics.hip; include/nmhip.h has the
// definitions): nm_fit_quality, nm_fit_rank.
//
//   quality  one workgroup per (set, 64-column tile), a lane per column: a wave reads 64 consecutive floats of a row of each of
//            the (up to) three tables.  The four waves take every fourth row, four rows at a time, and add in row order; the
//            waves' partials are merged through LDS in wave order by every wave alike, so all of them hold the column's means
//            for the second pass without another hand-off (cohort_moments_kernel's walk).  Pass 1: n, the non-finite count,
//            n_var, the coverage count, the sums of y, f, e and z, min and max of y and f, the two log-loss sums.  Pass 2 (the
//            tiles come from L2 this time): the centred sums of y, f, e and z with the sums of the centred values, SSE, sum |e|.
//   rank     one workgroup per (set, column).  The evaluated values of x and of loc become 32-bit order-preserving keys (-0 and
//            +0 one key) in dynamic LDS, packed in row order, and both arrays are bitonic-sorted between the same barriers.  A
//            thread per evaluated row then reads its two values again (L2) and searches each array twice; the sums are int64
//            and order-free, merged by an xor butterfly and through LDS.
// No atomics; every output element is written on every call; two runs give the same bytes.
#pragma clang fp contract(off)

namespace {

static_assert(sizeof(nm_fit_set_t) == 56, "nm_fit_set_t is mirrored by _lib.NmFitSet");
constexpr int FIT_P1 = 10, FIT_P2 = 13;            // fp64 partials of the two passes
constexpr double FIT_TWO_PI = 6.283185307179586;

// the table entry's own checks: what a kernel may read of the set
__device__ __forceinline__ bool fit_set_ok(const nm_fit_set_t& S, int D, int max_rows) {
  if (S.rows < 0 || S.rows > max_rows || S.pitch < D || S.loc_pitch < D) return false;
  if (S.var && S.var_pitch < D) return false;
  if (S.rows > 0 && (!S.x || !S.loc || !S.group)) return false;
  return true;
}

// t = r sqrt((n - 2) / ((1 - r)(1 + r))) and its two-sided p; r^2 >= 1: t = +-inf, p = 0 (n >= 3)
__device__ __forceinline__ void fit_t_and_p(double r, int n, double& t, double& p) {
  if (r * r >= 1.0) { t = r > 0.0 ? INFINITY : -INFINITY; p = 0.0; return; }
  const double df = (double)(n - 2);
  t = r * sqrt(df / ((1.0 - r) * (1.0 + r)));
  p = reg_student_t_two_sided(t, df);
}

__global__ __launch_bounds__(MT) void fit_quality_kernel(const nm_fit_set_t* __restrict__ sets, int D, int max_rows, int tiles,
                                                         const double* __restrict__ moments, int n_moments,
                                                         const int32_t* __restrict__ ref_of, double thr,
                                                         double* __restrict__ fit_out, double* __restrict__ cal_out) {
  __shared__ double pd[FIT_P2][NORM_WAVES * NORM_TILE];
  __shared__ int32_t pi[4][NORM_WAVES * NORM_TILE];
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  const int s = blockIdx.x / tiles, tile = blockIdx.x - s * tiles;
  const nm_fit_set_t S = sets[s];
  const int col = tile * NORM_TILE + lane;
  const bool cv = col < D;
  double* fo = fit_out + ((int64_t)s * D + col) * NM_METRICS_STRIDE;
  double* co = cal_out + ((int64_t)s * D + col) * NM_METRICS_STRIDE;
  const double qnan = norm_nan();
  if (!fit_set_ok(S, D, max_rows)) {
    if (w == 0 && cv) {
      for (int k = 0; k < 6; ++k) { fo[k] = qnan; co[k] = qnan; }
      fo[6] = 0.0; fo[7] = -2.0; co[6] = qnan; co[7] = 0.0;
    }
    return;
  }
  const int rows = S.rows;
  const bool has_var = S.var || S.col_var;
  const double cvar = (S.col_var && cv) ? (double)S.col_var[col] : 0.0;
  // the trivial model of the column: mean and variance of the train cohort
  double m_t = 0.0, v_t = qnan;
  {
    const int ref = (moments && ref_of) ? ref_of[s] : (moments ? s : -1);
    if (cv && ref >= 0 && ref < n_moments) {
      const double* m = moments + ((int64_t)ref * D + col) * NM_METRICS_STRIDE;
      if (m[7] == 0.0 && m[2] > 0.0) { m_t = m[0]; v_t = m[2]; }
    }
  }
  const bool triv = v_t == v_t;
  double sy = 0.0, sf = 0.0, se = 0.0, sz = 0.0, nll = 0.0, trv = 0.0;
  double ymn = INFINITY, ymx = -INFINITY, fmn = INFINITY, fmx = -INFINITY;
  int n = 0, nbad = 0, nvar = 0, ncov = 0;
  for (int r0 = w; r0 < rows; r0 += NORM_WAVES * NORM_RB) {
    double y[NORM_RB], f[NORM_RB], v[NORM_RB];
    bool in[NORM_RB];
#pragma unroll
    for (int k = 0; k < NORM_RB; ++k) {
      const int r = r0 + NORM_WAVES * k;
      in[k] = r < rows && S.group[min(r, rows - 1)] == 0;
      const bool ld = in[k] && cv;
      y[k] = ld ? (double)S.x[(int64_t)r * S.pitch + col] : 0.0;
      f[k] = ld ? (double)S.loc[(int64_t)r * S.loc_pitch + col] : 0.0;
      v[k] = (ld && S.var) ? (double)S.var[(int64_t)r * S.var_pitch + col] : 0.0;
    }
#pragma unroll
    for (int k = 0; k < NORM_RB; ++k)
      if (in[k]) {
        ++n;
        const double s2 = v[k] + cvar;
        const bool s2ok = has_var && norm_finite(s2) && s2 > 0.0;
        nvar += s2ok;
        if (norm_finite(y[k]) && norm_finite(f[k])) {
          const double e = y[k] - f[k];
          sy += y[k]; sf += f[k]; se += e;
          ymn = fmin(ymn, y[k]); ymx = fmax(ymx, y[k]); fmn = fmin(fmn, f[k]); fmx = fmax(fmx, f[k]);
          if (s2ok) {
            const double z = e / sqrt(s2);
            sz += z;
            nll += 0.5 * log(FIT_TWO_PI * s2) + e * e / (2.0 * s2);
            ncov += fabs(z) <= thr;
          }
          if (triv) { const double dt = y[k] - m_t; trv += dt * dt; }
        } else ++nbad;
      }
  }
  pd[0][t] = sy; pd[1][t] = sf; pd[2][t] = se; pd[3][t] = sz; pd[4][t] = nll; pd[5][t] = trv;
  pd[6][t] = ymn; pd[7][t] = ymx; pd[8][t] = fmn; pd[9][t] = fmx;
  pi[0][t] = n; pi[1][t] = nbad; pi[2][t] = nvar; pi[3][t] = ncov;
  __syncthreads();
  int N = 0, NB = 0, NV = 0, NC = 0;
  double SY = 0.0, SF = 0.0, SE = 0.0, SZ = 0.0, NLL = 0.0, TRV = 0.0;
  double YMN = INFINITY, YMX = -INFINITY, FMN = INFINITY, FMX = -INFINITY;
  for (int q = 0; q < NORM_WAVES; ++q) {
    const int i = q * NORM_TILE + lane;
    N += pi[0][i]; NB += pi[1][i]; NV += pi[2][i]; NC += pi[3][i];
    SY += pd[0][i]; SF += pd[1][i]; SE += pd[2][i]; SZ += pd[3][i]; NLL += pd[4][i]; TRV += pd[5][i];
    YMN = fmin(YMN, pd[6][i]); YMX = fmax(YMX, pd[7][i]); FMN = fmin(FMN, pd[8][i]); FMX = fmax(FMX, pd[9][i]);
  }
  const double dn = (double)N;
  const double my = SY / dn, mf = SF / dn, me = SE / dn, mz = SZ / dn;      // (every wave: the same bits)
  const bool zok = has_var && NV == N;               // every evaluated s2 is finite and > 0
  double syy = 0.0, sff = 0.0, syf = 0.0, see = 0.0, cy = 0.0, cf = 0.0, ce = 0.0, sse = 0.0, sae = 0.0;
  double c1 = 0.0, m2 = 0.0, m3 = 0.0, m4 = 0.0;
  if (N >= 2) {                                       // (N is the set's: the same for every thread)
    for (int r0 = w; r0 < rows; r0 += NORM_WAVES * NORM_RB) {
      double y[NORM_RB], f[NORM_RB], v[NORM_RB];
      bool in[NORM_RB];
#pragma unroll
      for (int k = 0; k < NORM_RB; ++k) {
        const int r = r0 + NORM_WAVES * k;
        in[k] = r < rows && S.group[min(r, rows - 1)] == 0;
        const bool ld = in[k] && cv;
        y[k] = ld ? (double)S.x[(int64_t)r * S.pitch + col] : 0.0;
        f[k] = ld ? (double)S.loc[(int64_t)r * S.loc_pitch + col] : 0.0;
        v[k] = (ld && S.var) ? (double)S.var[(int64_t)r * S.var_pitch + col] : 0.0;
      }
#pragma unroll
      for (int k = 0; k < NORM_RB; ++k)
        if (in[k]) {
          const double e = y[k] - f[k];
          const double dy = y[k] - my, df = f[k] - mf, de = e - me;
          syy += dy * dy; sff += df * df; syf += dy * df; see += de * de;
          cy += dy; cf += df; ce += de;
          sse += e * e; sae += fabs(e);
          if (zok) {
            const double dz = e / sqrt(v[k] + cvar) - mz;
            const double dz2 = dz * dz;
            c1 += dz; m2 += dz2; m3 += dz2 * dz; m4 += dz2 * dz2;
          }
        }
    }
  }
  __syncthreads();                                   // pass 1's partials are read
  pd[0][t] = syy; pd[1][t] = sff; pd[2][t] = syf; pd[3][t] = see; pd[4][t] = cy; pd[5][t] = cf; pd[6][t] = ce;
  pd[7][t] = sse; pd[8][t] = sae; pd[9][t] = c1; pd[10][t] = m2; pd[11][t] = m3; pd[12][t] = m4;
  __syncthreads();
  if (w == 0 && cv) {
    double a[FIT_P2];
#pragma unroll
    for (int k = 0; k < FIT_P2; ++k) {
      double acc = 0.0;
      for (int q = 0; q < NORM_WAVES; ++q) acc += pd[k][q * NORM_TILE + lane];
      a[k] = acc;
    }
    const bool ok = N >= 2 && NB == 0 && YMX > YMN;    // (Syy == 0 is told by min == max, not by a rounded sum)
    if (!ok) {
      for (int k = 0; k < 6; ++k) { fo[k] = qnan; co[k] = qnan; }
      fo[6] = dn; fo[7] = -2.0; co[6] = qnan; co[7] = (double)NV;
      return;
    }
    // the centred sums, corrected by the sums of the centred values
    const double Syy = a[0] - a[4] * a[4] / dn, Sff = a[1] - a[5] * a[5] / dn, Syf = a[2] - a[4] * a[5] / dn;
    const double See = a[3] - a[6] * a[6] / dn, SSE = a[7];
    const bool f_const = !(FMX > FMN);
    const bool b1 = f_const || N < 3, b2 = !zok, b4 = !triv;
    double rho = qnan, p_rho = qnan;
    if (!f_const) {
      rho = Syf / sqrt(Syy * Sff);
      if (N >= 3) { double tt; fit_t_and_p(rho, N, tt, p_rho); }
    }
    double msll = qnan;
    if (!b2 && !b4) msll = NLL / dn - (0.5 * log(FIT_TWO_PI * v_t) + TRV / (2.0 * v_t * dn));
    fo[0] = rho; fo[1] = p_rho; fo[2] = SSE / Syy; fo[3] = 1.0 - See / Syy; fo[4] = msll; fo[5] = sqrt(SSE / dn);
    fo[6] = dn; fo[7] = (double)((b1 ? 1 : 0) + (b2 ? 2 : 0) + (b4 ? 4 : 0));
    co[0] = me; co[1] = a[8] / dn;
    if (b2) { co[2] = qnan; co[3] = qnan; co[4] = qnan; co[5] = qnan; co[6] = qnan; }
    else {
      // the central moments of z about the exact mean mz + dl, from the sums about mz
      const double dl = a[9] / dn;
      const double u2 = a[10] / dn - dl * dl;
      const double u3 = a[11] / dn - 3.0 * dl * (a[10] / dn) + 2.0 * dl * dl * dl;
      const double u4 = a[12] / dn - 4.0 * dl * (a[11] / dn) + 6.0 * dl * dl * (a[10] / dn) - 3.0 * dl * dl * dl * dl;
      const double sd = sqrt(u2);
      co[2] = mz + dl; co[3] = sd; co[4] = u3 / (u2 * sd); co[5] = u4 / (u2 * u2) - 3.0; co[6] = (double)NC / dn;
    }
    co[7] = (double)NV;
  }
}

// ascending bitonic sort of both a[0..npad) and b[0..npad) between the same barriers, npad a power of two; all threads call
__device__ __forceinline__ void fit_sort_pair(uint32_t* a, uint32_t* b, int npad) {
  const int t = threadIdx.x;
  for (int k = 2; k <= npad; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int i = t; i < npad; i += MT) {
        const int p = i ^ j;
        if (p > i) {
          const bool up = (i & k) == 0;
          const uint32_t a0 = a[i], a1 = a[p], b0 = b[i], b1 = b[p];
          if ((a0 > a1) == up) { a[i] = a1; a[p] = a0; }
          if ((b0 > b1) == up) { b[i] = b1; b[p] = b0; }
        }
      }
      __syncthreads();
    }
  }
}

// left = #{a < kv}, right = #{a <= kv} among the sorted key[0..n): returns left + right, tied = the value occurs more than once
__device__ __forceinline__ int fit_k2(const uint32_t* key, int n, uint32_t kv, bool& tied) {
  int lo = 0, hi = n;
  while (lo < hi) { const int m = (lo + hi) >> 1; if (key[m] < kv) lo = m + 1; else hi = m; }
  const int left = lo;
  hi = n;
  while (lo < hi) { const int m = (lo + hi) >> 1; if (key[m] <= kv) lo = m + 1; else hi = m; }
  tied = lo - left > 1;
  return left + lo;
}

__global__ __launch_bounds__(MT) void fit_rank_kernel(const nm_fit_set_t* __restrict__ sets, int D, int max_rows,
                                                      double* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  __shared__ int32_t part[2][MT];
  __shared__ long long red[NORM_WAVES][8];
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  const int s = blockIdx.x / D, col = blockIdx.x - s * D;
  const nm_fit_set_t S = sets[s];
  double* o = out + ((int64_t)s * D + col) * NM_METRICS_STRIDE;
  const double qnan = norm_nan();
  if (!fit_set_ok(S, D, max_rows)) {
    if (t == 0) { o[0] = qnan; o[1] = qnan; o[2] = qnan; o[3] = 0.0; o[4] = qnan; o[5] = qnan; o[6] = 0.0; o[7] = -2.0; }
    return;
  }
  // the evaluated rows, packed in row order: a count and a prefix over the threads' row ranges (cent_sort_ref)
  const int rows = S.rows;
  const int per = (rows + MT - 1) / MT;
  const int lo = min(t * per, rows), hi = min(lo + per, rows);
  int cn = 0;
  for (int r = lo; r < hi; ++r) cn += (S.group[r] == 0);
  part[0][t] = cn;
  __syncthreads();
  int n = 0, pos = 0;
  for (int q = 0; q < MT; ++q) {
    const int c = part[0][q];
    if (q < t) pos += c;
    n += c;
  }
  int npad = 2;
  while (npad < n) npad <<= 1;                       // (n <= rows <= max_rows: inside the launch's dynamic LDS)
  uint32_t* ky = reinterpret_cast<uint32_t*>(smem);  // [npad]
  uint32_t* kf = ky + npad;                          // [npad]
  for (int i = n + t; i < npad; i += MT) { ky[i] = ~0u; kf[i] = ~0u; }
  int bad = 0;
  for (int r = lo; r < hi; ++r)
    if (S.group[r] == 0) {
      const float y = S.x[(int64_t)r * S.pitch + col], f = S.loc[(int64_t)r * S.loc_pitch + col];
      bad += !norm_finite((double)y) || !norm_finite((double)f);
      ky[pos] = asc_key(y); kf[pos] = asc_key(f);
      ++pos;
    }
  part[1][t] = bad;
  __syncthreads();
  int nbad = 0;
  for (int q = 0; q < MT; ++q) nbad += part[1][q];
  if (n < 2 || nbad > 0) {                           // (the same in every thread)
    if (t == 0) { o[0] = qnan; o[1] = qnan; o[2] = qnan; o[3] = (double)n; o[4] = qnan; o[5] = qnan; o[6] = 0.0; o[7] = -2.0; }
    return;
  }
  fit_sort_pair(ky, kf, npad);
  long long syf = 0, sy = 0, sf = 0, syy = 0, sff = 0, ty = 0, tf = 0;
  for (int r = t; r < rows; r += MT) {
    if (S.group[r] != 0) continue;
    bool tiey, tief;
    const long long ay = fit_k2(ky, n, asc_key(S.x[(int64_t)r * S.pitch + col]), tiey);
    const long long af = fit_k2(kf, n, asc_key(S.loc[(int64_t)r * S.loc_pitch + col]), tief);
    syf += ay * af; sy += ay; sf += af; syy += ay * ay; sff += af * af; ty += tiey; tf += tief;
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    syf += __shfl_xor(syf, off); sy += __shfl_xor(sy, off); sf += __shfl_xor(sf, off); syy += __shfl_xor(syy, off);
    sff += __shfl_xor(sff, off); ty += __shfl_xor(ty, off); tf += __shfl_xor(tf, off);
  }
  if (lane == 0) { red[w][0] = syf; red[w][1] = sy; red[w][2] = sf; red[w][3] = syy; red[w][4] = sff; red[w][5] = ty; red[w][6] = tf; }
  __syncthreads();
  if (t == 0) {
    long long a[7];
    for (int k = 0; k < 7; ++k) { a[k] = 0; for (int q = 0; q < NORM_WAVES; ++q) a[k] += red[q][k]; }
    const long long nn = n;
    const long long A = nn * a[0] - a[1] * a[2], B = nn * a[3] - a[1] * a[1], Cc = nn * a[4] - a[2] * a[2];
    const bool flat = B == 0 || Cc == 0;
    double rs = qnan, ts = qnan, ps = qnan;
    if (!flat) {
      rs = (double)A / sqrt((double)B * (double)Cc);
      if (n >= 3) fit_t_and_p(rs, n, ts, ps);
    }
    o[0] = rs; o[1] = ps; o[2] = ts; o[3] = (double)n; o[4] = (double)a[5]; o[5] = (double)a[6]; o[6] = 0.0;
    o[7] = (flat || n < 3) ? 1.0 : 0.0;
  }
}

}  // namespace

extern "C" {

int nm_fit_quality(const nm_fit_set_t* sets_dev, int n_sets, int D, int max_rows, const double* moments, int n_moments,
                   const int32_t* ref_of, double thr, double* fit_out, double* cal_out, void* stream) {
  if (!sets_dev || !fit_out || !cal_out || (ref_of && !moments)) return NM_E_NULL;
  if (norm_common_bad(n_sets, max_rows) || D < 1 || !(thr > 0.0) || !(thr < INFINITY) || (moments && n_moments < 1))
    return NM_E_METRICS;
  const int tiles = (D + NORM_TILE - 1) / NORM_TILE;
  if ((int64_t)n_sets * tiles > 0x7FFFFFFFll) return NM_E_METRICS;
  return launch_kernel(fit_quality_kernel, dim3(n_sets * tiles), dim3(MT), 0, stream, sets_dev, D, max_rows, tiles, moments,
                       moments ? n_moments : 0, ref_of, thr, fit_out, cal_out);
}

int nm_fit_rank(const nm_fit_set_t* sets_dev, int n_sets, int D, int max_rows, double* rank_out, void* stream) {
  if (!sets_dev || !rank_out) return NM_E_NULL;
  if (norm_common_bad(n_sets, max_rows) || D < 1) return NM_E_METRICS;
  if ((int64_t)n_sets * D > 0x7FFFFFFFll) return NM_E_METRICS;
  return launch_kernel(fit_rank_kernel, dim3(n_sets * D), dim3(MT), pow2_at_least(max_rows) * 8, stream, sets_dev, D, max_rows,
                       rank_out);
}

}  // extern "C"
