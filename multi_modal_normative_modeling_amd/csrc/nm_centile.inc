// nm_centile.inc -- normative centiles on the device (included at the end of nm_metrics.hip; include/nmhip.h has the
// definitions): nm_cohort_quantiles, nm_normative_centile_workspace, nm_normative_centile.
//
//   quantiles  one workgroup per (set, column).  The values of the rows with group 0 become order-preserving 64-bit keys
//              (-0 and +0 one key) in dynamic LDS, packed in row order by a count and a prefix over the threads' row
//              ranges, and are bitonic-sorted there as roi_rank_kernel sorts (sort_keys).  Every thread reads the median
//              from LDS; the requested quantiles are a thread each, numpy's linear rule one operation at a time.  The keys
//              are then replaced by those of |v - median| and sorted again: the MAD is the same median of that.
//   rank       one workgroup per (scored set, column): ONE column, not a tile.  A tile of two or four columns per workgroup
//              (the neighbouring floats of a row share a sector) was built and measured: the sorts of a tile run one after
//              another between the same barriers, and both sorting kernels got slower (DESIGN.md has the figures).
//              The reference column is sorted as above, then a thread per row searches its value twice
//              (#{a < v}, #{a <= v}) and writes k2 = left + right as uint16 to the workspace [total_rows][D]; 0xFFFF
//              marks a non-finite value, an invalid column or an invalid element.
//   rows       one workgroup per (set, NM_NORM_ROWS_PER_WG rows), a wave per row, lanes over the columns of the k2 row
//              (coalesced).  The workgroup counts the reference rows once.  Sums are int64 until the last operations; the
//              lanes are merged by an xor butterfly (integers: any shape gives the same sum).
//   cols       one workgroup per (set, 64 columns), a lane per column, the four waves take every fourth row; integer
//              partials merged through LDS.
// No atomics; every output element is written on every call; two runs give the same bytes.
#pragma clang fp contract(off)

namespace {

struct CentProbs { double p[NM_CENT_MAX_Q]; };
static_assert(sizeof(CentProbs) <= 1024, "the probabilities travel as a kernel argument");
static_assert(2 * NM_METRICS_MAX_N < 0xFFFF, "k2 = left + right fits a uint16 below the invalid mark");
constexpr uint16_t CENT_INVALID = 0xFFFF;

// ascending order-preserving key of a double (-0 and +0 are one value), and back
__device__ __forceinline__ uint64_t cent_key(double x) {
  if (x == 0.0) x = 0.0;
  const uint64_t b = (uint64_t)__double_as_longlong(x);
  return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
__device__ __forceinline__ double cent_val(uint64_t k) {
  const uint64_t b = (k >> 63) ? (k & 0x7FFFFFFFFFFFFFFFull) : ~k;
  return __longlong_as_double((long long)b);
}

// what the centile pass may read and write of a scored set: the table entry's own checks, the optional pct table's pitch,
// and its rows inside the caller's per-row arrays
__device__ __forceinline__ bool cent_rows_in_range(const nm_norm_set_t& S, int max_rows, int total_rows) {
  return S.rows >= 0 && S.rows <= max_rows && S.row_off >= 0 && (int64_t)S.row_off + S.rows <= (int64_t)total_rows;
}
__device__ __forceinline__ bool cent_scored_ok(const nm_norm_set_t& S, int D, int max_rows, int total_rows) {
  return norm_set_ok(S, D, max_rows, true) && (!S.z || S.z_pitch >= D) && cent_rows_in_range(S, max_rows, total_rows);
}

// n = the rows of R with group 0 (all threads call, R passes norm_set_ok); part is [MT] ints of LDS
__device__ __forceinline__ int cent_count_ref(const nm_norm_set_t& R, int32_t* part) {
  const int t = threadIdx.x;
  int cn = 0;
  for (int r = t; r < R.rows; r += MT) cn += (R.group[r] == 0);
  part[t] = cn;
  __syncthreads();
  int n = 0;
  for (int q = 0; q < MT; ++q) n += part[q];
  __syncthreads();
  return n;
}

// The sorted reference column (all threads call, R passes norm_set_ok): key[0..npad) <- the keys of column col over the rows
// of R with group 0, ascending, the pad at the maximum key.  Returns n; nbad = the non-finite among them, and with n < 1 or
// nbad > 0 the keys are left unsorted (the column is not valid).  part is [2][MT] ints of LDS.
__device__ __forceinline__ int cent_sort_ref(const nm_norm_set_t& R, int col, uint64_t* key, int32_t (*part)[MT], int& nbad, int& npad) {
  const int t = threadIdx.x;
  const int rows = R.rows;
  const int per = (rows + MT - 1) / MT;
  const int lo = min(t * per, rows), hi = min(lo + per, rows);
  int cn = 0;
  for (int r = lo; r < hi; ++r) cn += (R.group[r] == 0);
  part[0][t] = cn;
  __syncthreads();
  int n = 0, pos = 0;
  for (int q = 0; q < MT; ++q) {
    const int c = part[0][q];
    if (q < t) pos += c;
    n += c;
  }
  npad = 2;
  while (npad < n) npad <<= 1;
  for (int i = n + t; i < npad; i += MT) key[i] = ~0ull;
  int bad = 0;
  for (int r = lo; r < hi; ++r)
    if (R.group[r] == 0) {
      const double v = norm_value(R, r, col);
      bad += !norm_finite(v);
      key[pos++] = cent_key(v);
    }
  part[1][t] = bad;
  __syncthreads();
  nbad = 0;
  for (int q = 0; q < MT; ++q) nbad += part[1][q];
  if (n >= 1 && nbad == 0) sort_keys(key, npad);     // (n and nbad are the same in every thread)
  return n;
}

// np.median of the sorted keys: the middle value, or the mean of the two middle ones
__device__ __forceinline__ double cent_median(const uint64_t* key, int n) {
  if (n & 1) return cent_val(key[n >> 1]);
  return (cent_val(key[n / 2 - 1]) + cent_val(key[n / 2])) / 2.0;
}

// np.quantile(method="linear") of the sorted keys at p in [0, 1], one operation at a time
__device__ __forceinline__ double cent_quantile(const uint64_t* key, int n, double p) {
  const double top = (double)(n - 1);
  const double h = top * p;
  const double jf = floor(h);
  const double g = h - jf;
  double a, b;
  if (h >= top) { a = cent_val(key[n - 1]); b = a; }
  else { const int j = (int)jf; a = cent_val(key[j]); b = cent_val(key[j + 1]); }
  const double d = b - a;
  double r = a + d * g;
  if (g >= 0.5) r = b - d * (1.0 - g);
  return r;
}

__global__ __launch_bounds__(MT) void cohort_quantiles_kernel(const nm_norm_set_t* __restrict__ sets, int D, int max_rows,
                                                              CentProbs P, int n_q, double* __restrict__ q_out,
                                                              double* __restrict__ stats_out) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  uint64_t* key = reinterpret_cast<uint64_t*>(smem);            // [npad]
  __shared__ int32_t part[2][MT];
  const int t = threadIdx.x;
  const int s = blockIdx.x / D, col = blockIdx.x - s * D;
  const nm_norm_set_t S = sets[s];
  const int64_t ci = (int64_t)s * D + col;
  double* so = stats_out + ci * NM_METRICS_STRIDE;
  double* qo = q_out ? q_out + ci * n_q : nullptr;
  const double qnan = norm_nan();
  int n = 0, nbad = 0, npad = 2;
  const bool set_ok = norm_set_ok(S, D, max_rows, true);
  if (set_ok) n = cent_sort_ref(S, col, key, part, nbad, npad);
  if (!set_ok || n < 1 || nbad > 0) {
    for (int q = t; q < n_q; q += MT) qo[q] = qnan;
    if (t == 0) {
      so[0] = qnan; so[1] = qnan; so[2] = qnan; so[3] = qnan; so[4] = qnan;
      so[5] = (double)n; so[6] = (double)nbad; so[7] = -2.0;
    }
    return;
  }
  const double med = cent_median(key, n);              // (every thread: the same bits, LDS broadcasts)
  double q1 = 0.0, q3 = 0.0;
  if (t == 0) { q1 = cent_quantile(key, n, 0.25); q3 = cent_quantile(key, n, 0.75); }
  for (int q = 0; q < n_q; ++q)                        // (q is uniform: P.p[q] is a scalar load)
    if (t == (q & (MT - 1))) qo[q] = cent_quantile(key, n, P.p[q]);
  __syncthreads();                                     // the sorted values are read
  for (int i = t; i < n; i += MT) key[i] = cent_key(fabs(cent_val(key[i]) - med));
  __syncthreads();
  sort_keys(key, npad);                                // (the pad stays at the maximum key)
  if (t == 0) {
    so[0] = med; so[1] = cent_median(key, n); so[2] = q1; so[3] = q3; so[4] = q3 - q1;
    so[5] = (double)n; so[6] = 0.0; so[7] = 0.0;
  }
}

__global__ __launch_bounds__(MT) void centile_rank_kernel(const nm_norm_set_t* __restrict__ sets, int n_sets, int D, int max_rows,
                                                          int total_rows, const int32_t* __restrict__ ref_of, int loo,
                                                          uint16_t* __restrict__ k2) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  uint64_t* key = reinterpret_cast<uint64_t*>(smem);            // [npad]
  __shared__ int32_t part[2][MT];
  const int t = threadIdx.x;
  const int s = blockIdx.x / D, col = blockIdx.x - s * D;
  const int ref = ref_of ? ref_of[s] : s;
  if (ref == -1) return;                               // a reference only: it owns no rows
  const nm_norm_set_t S = sets[s];
  if (!cent_scored_ok(S, D, max_rows, total_rows)) return;   // refused: the rows pass writes status rows and reads no k2
  const int rows = S.rows;
  if (rows == 0) return;
  bool usable = ref >= 0 && ref < n_sets;
  int n = 0, nbad = 0, npad = 2;
  if (usable) {
    const nm_norm_set_t R = sets[ref];
    usable = norm_set_ok(R, D, max_rows, true);
    if (usable) n = cent_sort_ref(R, col, key, part, nbad, npad);
  }
  const bool col_ok = usable && n >= 1 && nbad == 0;
  const bool self = loo && ref == s;
  uint16_t* o = k2 + (int64_t)S.row_off * D + col;
  for (int r = t; r < rows; r += MT) {
    uint16_t w = CENT_INVALID;
    if (col_ok) {
      const double v = norm_value(S, r, col);
      if (norm_finite(v)) {
        const uint64_t kv = cent_key(v);
        int lo = 0, hi = n;                            // left = #{a < v}
        while (lo < hi) { const int m = (lo + hi) >> 1; if (key[m] < kv) lo = m + 1; else hi = m; }
        const int left = lo;
        hi = n;                                        // right = #{a <= v}, from left on
        while (lo < hi) { const int m = (lo + hi) >> 1; if (key[m] <= kv) lo = m + 1; else hi = m; }
        int k = left + lo;
        bool ok = true;
        if (self && S.group[r] == 0) { k -= 1; ok = n > 1; }    // leave-one-out: the row itself is among the a <= v
        if (ok) w = (uint16_t)k;
      }
    }
    o[(int64_t)r * D] = w;
  }
}

__global__ __launch_bounds__(MT) void centile_rows_kernel(const nm_norm_set_t* __restrict__ sets, int n_sets, int D, int max_rows,
                                                          int chunks, int total_rows, const int32_t* __restrict__ ref_of,
                                                          double tail, int loo, const uint16_t* __restrict__ k2,
                                                          double* __restrict__ rows_out) {
  __shared__ int32_t part[MT];
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  const int s = blockIdx.x / chunks, chunk = blockIdx.x - s * chunks;
  const int ref = ref_of ? ref_of[s] : s;
  if (ref == -1) return;
  const nm_norm_set_t S = sets[s];
  if (!cent_rows_in_range(S, max_rows, total_rows)) return;     // no rows to write
  const int rows = S.rows;
  const int r_begin = chunk * NORM_RW;
  if (r_begin >= rows) return;
  const bool ok = cent_scored_ok(S, D, max_rows, total_rows);
  int n = 0;
  if (ok && ref >= 0 && ref < n_sets) {                // (the same in every thread)
    const nm_norm_set_t R = sets[ref];
    if (norm_set_ok(R, D, max_rows, true)) n = cent_count_ref(R, part);
  }
  const bool self = loo && ref == s;
  const double qnan = norm_nan();
  const double hi_thr = 100.0 - tail;
  for (int rr = w; rr < NORM_RW; rr += NORM_WAVES) {
    const int r = r_begin + rr;
    if (r >= rows) break;
    double* o = rows_out + ((int64_t)S.row_off + r) * NM_METRICS_STRIDE;
    if (!ok) {
      if (lane == 0) { o[0] = 0.0; o[1] = 0.0; o[2] = qnan; o[3] = qnan; o[4] = qnan; o[5] = -1.0; o[6] = 0.0; o[7] = -2.0; }
      continue;
    }
    const int nd = (self && S.group[r] == 0) ? n - 1 : n;        // the row's own divisor
    const double f = 50.0 / (double)nd;                // (nd < 1: every element of the row is marked invalid)
    const uint16_t* kr = k2 + ((int64_t)S.row_off + r) * D;
    int nhi = 0, nlo = 0, nv = 0, am = -1, mk = -1;
    long long sk = 0, sa = 0;
    for (int c = lane; c < D; c += 64) {
      const int kk = kr[c];
      const bool valid = kk != CENT_INVALID;
      const double pct = valid ? (double)kk * f : qnan;
      if (S.z) S.z[(int64_t)r * S.z_pitch + c] = (float)pct;
      if (valid) {
        nhi += pct > hi_thr; nlo += pct < tail; ++nv;
        sk += kk; sa += abs(kk - nd);
        if (kk > mk) { mk = kk; am = c; }
      }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
      nhi += __shfl_xor(nhi, off); nlo += __shfl_xor(nlo, off); nv += __shfl_xor(nv, off);
      sk += __shfl_xor(sk, off); sa += __shfl_xor(sa, off);
      const int ok2 = __shfl_xor(mk, off), oa = __shfl_xor(am, off);
      if (ok2 > mk || (ok2 == mk && oa >= 0 && oa < am)) { mk = ok2; am = oa; }
    }
    if (lane == 0) {
      o[0] = (double)nhi; o[1] = (double)nlo;
      o[2] = nv ? (double)sk * f / (double)nv : qnan;
      o[3] = nv ? (double)sa * f / (double)nv : qnan;
      o[4] = nv ? (double)mk * f : qnan;
      o[5] = (double)am;
      o[6] = (double)nv;
      o[7] = nv ? 0.0 : -2.0;
    }
  }
}

__global__ __launch_bounds__(MT) void centile_cols_kernel(const nm_norm_set_t* __restrict__ sets, int n_sets, int D, int max_rows,
                                                          int tiles, int total_rows, const int32_t* __restrict__ ref_of,
                                                          double tail, int loo, const uint16_t* __restrict__ k2,
                                                          double* __restrict__ out) {
  __shared__ int32_t pc[6][NORM_WAVES * NORM_TILE];
  __shared__ long long ps[2][NORM_WAVES * NORM_TILE];
  __shared__ int32_t part[MT];
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  const int s = blockIdx.x / tiles, tile = blockIdx.x - s * tiles;
  const int col = tile * NORM_TILE + lane;
  const bool cv = col < D;
  double* o = out + ((int64_t)s * D + col) * NM_METRICS_STRIDE;
  const double qnan = norm_nan();
  const int ref = ref_of ? ref_of[s] : s;
  const nm_norm_set_t S = sets[s];
  bool ok = ref >= 0 && ref < n_sets && cent_scored_ok(S, D, max_rows, total_rows);
  int n = 0;
  if (ok) {                                            // (the same in every thread)
    const nm_norm_set_t R = sets[ref];
    ok = norm_set_ok(R, D, max_rows, true);
    if (ok) n = cent_count_ref(R, part);
  }
  if (!ok) {
    if (w == 0 && cv)
      for (int k = 0; k < NM_METRICS_STRIDE; ++k) o[k] = qnan;
    return;
  }
  const bool self = loo && ref == s;
  const double fx = 50.0 / (double)n, fy = 50.0 / (double)(self ? n - 1 : n);
  const double hi_thr = 100.0 - tail;
  const int rows = S.rows;
  const uint16_t* kc = k2 + (int64_t)S.row_off * D + col;
  int hx = 0, lx = 0, hy = 0, ly = 0, nx = 0, ny = 0;
  long long sx = 0, sy = 0;
  for (int r = w; r < rows; r += NORM_WAVES) {
    const int g = S.group[r];
    if (g != 0 && g != 1) continue;
    const int kk = cv ? kc[(int64_t)r * D] : CENT_INVALID;
    if (kk == CENT_INVALID) continue;
    const double pct = (double)kk * (g == 1 ? fx : fy);
    const int hi = pct > hi_thr, lo = pct < tail;
    if (g == 1) { hx += hi; lx += lo; ++nx; sx += kk; }
    else { hy += hi; ly += lo; ++ny; sy += kk; }
  }
  pc[0][t] = hx; pc[1][t] = lx; pc[2][t] = hy; pc[3][t] = ly; pc[4][t] = nx; pc[5][t] = ny; ps[0][t] = sx; ps[1][t] = sy;
  __syncthreads();
  if (w == 0 && cv) {
    int c[6] = {0, 0, 0, 0, 0, 0};
    long long SX = 0, SY = 0;
    for (int q = 0; q < NORM_WAVES; ++q) {
      const int i = q * NORM_TILE + lane;
#pragma unroll
      for (int k = 0; k < 6; ++k) c[k] += pc[k][i];
      SX += ps[0][i]; SY += ps[1][i];
    }
#pragma unroll
    for (int k = 0; k < 6; ++k) o[k] = (double)c[k];
    o[6] = c[4] ? (double)SX * fx / (double)c[4] : qnan;
    o[7] = c[5] ? (double)SY * fy / (double)c[5] : qnan;
  }
}

inline size_t cent_workspace(int total_rows, int D) {
  if (total_rows < 0 || D < 1) return 0;
  const size_t b = (size_t)total_rows * (size_t)D * 2;
  return (b / 256 + 1) * 256;                          // (never 0 for arguments a launch accepts)
}

}  // namespace

extern "C" {

int nm_cohort_quantiles(const nm_norm_set_t* sets_dev, int n_sets, int D, int max_rows, const double* probs_host, int n_q,
                        double* q_out, double* stats_out, void* stream) {
  if (!sets_dev || !stats_out) return NM_E_NULL;
  if (n_q < 0 || n_q > NM_CENT_MAX_Q) return NM_E_METRICS;
  if (n_q > 0 && (!probs_host || !q_out)) return NM_E_NULL;
  if (norm_common_bad(n_sets, max_rows) || D < 1) return NM_E_METRICS;
  CentProbs P = {};
  for (int q = 0; q < n_q; ++q) {
    if (!(probs_host[q] >= 0.0 && probs_host[q] <= 1.0)) return NM_E_METRICS;      // (NaN fails both)
    P.p[q] = probs_host[q];
  }
  if ((int64_t)n_sets * D > 0x7FFFFFFFll) return NM_E_METRICS;
  return launch_kernel(cohort_quantiles_kernel, dim3(n_sets * D), dim3(MT), pow2_at_least(max_rows) * 8, stream, sets_dev, D,
                       max_rows, P, n_q, q_out, stats_out);
}

size_t nm_normative_centile_workspace(int total_rows, int D) { return cent_workspace(total_rows, D); }

int nm_normative_centile(const nm_norm_set_t* sets_dev, int n_sets, int D, int max_rows, int total_rows, const int32_t* ref_of,
                         double tail, int loo, void* workspace, size_t workspace_bytes, double* rows_out, double* cols_out,
                         void* stream) {
  if (!sets_dev || !workspace || !rows_out || !cols_out) return NM_E_NULL;
  if (norm_common_bad(n_sets, max_rows) || D < 1 || total_rows < 0 || !(tail > 0.0) || !(tail < 50.0) || (loo != 0 && loo != 1))
    return NM_E_METRICS;
  if (workspace_bytes < cent_workspace(total_rows, D)) return NM_E_METRICS;
  const int tiles = (D + NORM_TILE - 1) / NORM_TILE, chunks = (max_rows + NORM_RW - 1) / NORM_RW;
  if ((int64_t)n_sets * D > 0x7FFFFFFFll || (int64_t)n_sets * chunks > 0x7FFFFFFFll) return NM_E_METRICS;
  uint16_t* k2 = (uint16_t*)workspace;
  int e = launch_kernel(centile_rank_kernel, dim3(n_sets * D), dim3(MT), pow2_at_least(max_rows) * 8, stream, sets_dev, n_sets, D,
                        max_rows, total_rows, ref_of, loo, k2);
  if (e) return e;
  e = launch_kernel(centile_rows_kernel, dim3(n_sets * chunks), dim3(MT), 0, stream, sets_dev, n_sets, D, max_rows, chunks,
                    total_rows, ref_of, tail, loo, (const uint16_t*)k2, rows_out);
  if (e) return e;
  return launch_kernel(centile_cols_kernel, dim3(n_sets * tiles), dim3(MT), 0, stream, sets_dev, n_sets, D, max_rows, tiles,
                       total_rows, ref_of, tail, loo, (const uint16_t*)k2, cols_out);
}

}  // extern "C"
