// Post-hoc metrics of the sweep on the device: the numbers the final RCCL gather carries.
//
//   nm_posthoc_metrics    per-subject deviation scores + class labels -> ROC-AUC, Youden-J threshold, accuracy,
//                         sensitivity, specificity, significance ratio
//                         (compute_classification_performance, multimodal_kfold_cvae_group_analysis_1x1.py:105-157;
//                          sklearn.metrics.roc_curve / auc as called there at :125-126)
//   nm_confusion_metrics  hard predictions + labels -> accuracy, auroc, sensitivity, specificity, f1, precision
//                         (evaluate, multimodal_kfold_cvae_nmpmcont.py:29-70)
//   nm_latent_stats       exported joint latent means of a cohort -> column means and population variances
//   nm_latent_score       ... and a cohort's (mu, logvar) against them -> z-score per latent dimension, its mean |z|
//                         (latent_deviation / separate_latent_deviation, utils_vae.py:155-161)
//   nm_roi_effect         ROI-wise squared errors of two groups -> Cliff's delta, ROC-AUC, pair counts, group means per ROI
//                         (cliff_delta, utils.py:97-109, once per column; further down in this file)
//   nm_roi_significance   the same tables -> Mann-Whitney U, z and asymptotic p per ROI, Benjamini-Hochberg q, and the
//                         label-permutation p-values, per ROI and against the maximum over the ROIs
//   nm_auc_bootstrap      score sets -> the ROC-AUC with its stratified-bootstrap percentile interval, mean and standard error,
//                         and for pairs of sets on the same subjects the difference with its interval and p (at the end)
//   nm_column_regress     tables and a target per set -> per column the OLS or Logit fit target ~ const + column + covariates:
//                         both reported parameters, their standard errors and p-values
//                         (latent_pvalues, utils_vae.py:163-174, once per column; after the bootstrap)
//   nm_cohort_moments, nm_normative_z, nm_cohort_cov, nm_mahalanobis
//                         ROI tables -> z-scores against a reference cohort, the per-subject and per-ROI counts beyond a threshold;
//                         latent tables -> a cohort's covariance factor and every row's Mahalanobis distance to it
//                         (the sigma-normalised extra of SURVEY.md; nm_normative.inc, included at the end of this file)
//   nm_operating_points   score sets -> the threshold of every rule of compute_classification_performance (roc, f1, pr, cost,
//                         eer) and two more, scored on the same or on another set; PR-AUC, partial AUC, ROC on a grid
//                         (nm_curve.inc, included at the end of this file)
//   nm_cohort_quantiles, nm_normative_centile
//                         ROI tables -> a reference cohort's quantiles, median and MAD per ROI; every subject's percentile rank
//                         in it, the per-subject and per-ROI counts in the tails (nm_centile.inc, included at the end of this file)
//   nm_fit_quality, nm_fit_rank
//                         observed and predicted ROI tables -> per ROI the model's fit on the hold-out controls: Pearson and
//                         Spearman rho, SMSE, EXPV, MSLL, RMSE and the shape of the z distribution (nm_fit.inc, included at the
//                         end of this file)
//
// One workgroup per score set (a (fold, procedure) cell); sets are segments of one concatenated array.  The
// whole set lives in LDS: order-preserving 64-bit keys (score, label) are bitonic-sorted descending, label
// prefix sums give (tps, fps) at every distinct-score boundary exactly as sklearn's _binary_clf_curve builds
// them, and counts stay integers until the final divisions (fp64, IEEE) -- so counts, thresholds and the
// chosen operating point are bit-exact against the CPU restatement; the AUC is the exactly rounded value of
// the integer trapezoid sum.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>
#include "nmhip.h"
#include "nm_host.inc"

namespace {

constexpr int MT = 256;                 // threads per workgroup
constexpr int MAXN = NM_METRICS_MAX_N;  // scores per set (power of two)

__device__ __forceinline__ uint32_t desc_key(float x) {
  if (x == 0.0f) x = 0.0f;                               // -0 and +0 are one threshold (np.diff == 0)
  uint32_t b = __float_as_uint(x);
  uint32_t asc = (b & 0x80000000u) ? ~b : (b | 0x80000000u);   // ascending order-preserving key
  return ~asc;                                           // ascending sort of this = descending scores
}
__device__ __forceinline__ float key_score(uint32_t k) {
  uint32_t asc = ~k;
  uint32_t b = (asc & 0x80000000u) ? (asc & 0x7FFFFFFFu) : ~asc;
  return __uint_as_float(b);
}

// inclusive prefix sum of v[0..npad) in place (npad a power of two >= MT or smaller), all threads call
__device__ __forceinline__ void block_scan(int32_t* v, int npad, int32_t* part) {
  const int per = (npad + MT - 1) / MT;
  const int t = threadIdx.x;
  const int lo = min(t * per, npad), hi = min(lo + per, npad);
  int32_t s = 0;
  for (int i = lo; i < hi; ++i) { s += v[i]; v[i] = s; }
  part[t] = s;
  __syncthreads();
  for (int off = 1; off < MT; off <<= 1) {
    int32_t add = (t >= off) ? part[t - off] : 0;
    __syncthreads();
    part[t] += add;
    __syncthreads();
  }
  const int32_t base = (t > 0) ? part[t - 1] : 0;
  for (int i = lo; i < hi; ++i) v[i] += base;
  __syncthreads();
}

// The sorted set both curve kernels work on (posthoc_kernel here, select_kernel in nm_curve.inc), all threads call, 1 <= n <= MAXN:
// key[0..n) = (desc_key(score) << 32 | label != 0) ascending = scores descending, cum[i] = positives among the first i + 1,
// bnd[j] = sorted position of the j-th distinct score's last member (sklearn's distinct_value_indices + the last position).
// Returns K, the number of distinct scores; nan != 0 in a thread that loaded a NaN score.
__device__ __forceinline__ int build_curve(const float* __restrict__ scores, const int32_t* __restrict__ labels, int base, int n,
                                           uint64_t* key, int32_t* cum, int32_t* bnd, int32_t* part, int& nan) {
  const int t = threadIdx.x;
  nan = 0;
  int npad = 2;
  while (npad < n) npad <<= 1;
  for (int i = t; i < npad; i += MT) {
    uint64_t k = ~0ull;
    if (i < n) {
      const float v = scores[base + i];
      nan |= (v != v);
      k = ((uint64_t)desc_key(v) << 32) | (uint64_t)(labels[base + i] != 0);
    }
    key[i] = k;
  }
  __syncthreads();
  // bitonic sort, ascending in key = descending in score
  for (int k = 2; k <= npad; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int i = t; i < npad; i += MT) {
        int p = i ^ j;
        if (p > i) {
          uint64_t a = key[i], b = key[p];
          bool up = (i & k) == 0;
          if ((a > b) == up) { key[i] = b; key[p] = a; }
        }
      }
      __syncthreads();
    }
  }
  for (int i = t; i < npad; i += MT) {
    cum[i] = (i < n) ? (int32_t)(key[i] & 1ull) : 0;
    bnd[i] = (i < n && (i == n - 1 || (key[i] >> 32) != (key[i + 1] >> 32))) ? 1 : 0;   // distinct_value_indices + last
  }
  __syncthreads();
  block_scan(cum, npad, part);
  // compact the boundaries: bnd[j] = sorted position of the j-th threshold.  After the scan, position i is a
  // boundary iff its inclusive count differs from its predecessor's; targets lie at or below i, so every
  // thread first collects its (target, position) pairs, then all write after a barrier.
  block_scan(bnd, npad, part);
  const int K = bnd[npad - 1];
  __syncthreads();
  {
    const int per = (npad + MT - 1) / MT;
    const int lo = min(t * per, npad), hi = min(lo + per, npad);
    int32_t mypos[32], myidx[32];          // per <= MAXN / MT = 32
    int cnt = 0;
    for (int i = lo; i < hi; ++i) {
      int32_t c = bnd[i], p = (i > 0) ? bnd[i - 1] : 0;
      if (c != p) { mypos[cnt] = c - 1; myidx[cnt] = i; ++cnt; }
    }
    __syncthreads();
    for (int q = 0; q < cnt; ++q) bnd[mypos[q]] = myidx[q];
    __syncthreads();
  }
  return K;
}

__global__ __launch_bounds__(MT) void posthoc_kernel(const float* __restrict__ scores, const int32_t* __restrict__ labels,
                                                     const int32_t* __restrict__ offsets, const double* __restrict__ thr_in,
                                                     double* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  uint64_t* key = reinterpret_cast<uint64_t*>(smem);            // [MAXN]
  int32_t* cum = reinterpret_cast<int32_t*>(key + MAXN);        // [MAXN] label prefix sums (tps)
  int32_t* bnd = cum + MAXN;                                    // [MAXN] boundary flags -> compacted indices
  __shared__ int32_t part[MT];
  __shared__ double redJ[MT];
  __shared__ int32_t redI[MT];
  __shared__ long long redA[MT];

  const int s = blockIdx.x, t = threadIdx.x;
  const int base = offsets[s], n = offsets[s + 1] - base;
  double* o = out + (int64_t)s * NM_METRICS_STRIDE;
  const double qnan = __longlong_as_double(0x7FF8000000000000ll);
  if (n <= 0 || n > MAXN) {
    if (t < NM_METRICS_STRIDE) o[t] = qnan;
    return;
  }
  int nan;
  const int K = build_curve(scores, labels, base, n, key, cum, bnd, part, nan);
  const int P = cum[n - 1], Nn = n - P;
  if (P == 0 || Nn == 0) {                 // roc_curve is undefined with one class
    if (t < NM_METRICS_STRIDE) o[t] = qnan;
    if (t == 0) { o[6] = (double)P; o[7] = (double)Nn; }
    return;
  }
  // points j = 0..K-1: (fps_j, tps_j); origin (0,0) precedes them with threshold +inf (sklearn >= 1.3)
  double bestJ = 0.0;                      // the origin's J; a point must beat it strictly (argmax takes the first)
  int bestj = -1;
  long long area2 = 0;
  for (int j = t; j < K; j += MT) {
    const int i = bnd[j];
    const long long tp = cum[i], fp = (long long)i + 1 - tp;
    long long tp0 = 0, fp0 = 0;
    if (j > 0) { const int i0 = bnd[j - 1]; tp0 = cum[i0]; fp0 = (long long)i0 + 1 - tp0; }
    area2 += (fp - fp0) * (tp + tp0);
    bool kept = (j == 0) || (j == K - 1);
    if (!kept) {                           // drop_intermediate: keep only corners of the curve
      const int i1 = bnd[j + 1];
      const long long tp1 = cum[i1], fp1 = (long long)i1 + 1 - tp1;
      kept = (fp1 - 2 * fp + fp0 != 0) || (tp1 - 2 * tp + tp0 != 0);
    }
    if (kept) {
      const double J = (double)tp / (double)P - (double)fp / (double)Nn;      // tpr - fpr as numpy forms it
      if (J > bestJ) { bestJ = J; bestj = j; }                               // j ascends per thread: first max kept
    }
  }
  redJ[t] = bestJ; redI[t] = bestj; redA[t] = area2;
  __syncthreads();
  if (t == 0) {
    double bj = 0.0; int bi = -1; long long a2 = 0;
    for (int w = 0; w < MT; ++w) {
      a2 += redA[w];
      if (redI[w] >= 0 && (redJ[w] > bj || (redJ[w] == bj && bi >= 0 && redI[w] < bi))) { bj = redJ[w]; bi = redI[w]; }
    }
    const double auc = (double)a2 / (2.0 * (double)P * (double)Nn);
    double thr;
    long long TP, FP;
    if (thr_in) {
      thr = thr_in[s];
      TP = -1; FP = -1;                    // counted below by everyone
    } else if (bi < 0) {
      thr = __longlong_as_double(0x7FF0000000000000ll); TP = 0; FP = 0;
    } else {
      const int i = bnd[bi];
      thr = (double)key_score((uint32_t)(key[i] >> 32));
      TP = cum[i]; FP = (long long)i + 1 - TP;
    }
    o[0] = auc; o[1] = thr; o[5] = auc / (1.0 - auc); o[6] = (double)P; o[7] = (double)Nn;
    redA[0] = TP; redA[1] = FP;
  }
  __syncthreads();
  long long TP = redA[0], FP = redA[1];
  if (thr_in) {                            // given threshold: predicted = score >= thr
    const double thr = thr_in[s];
    int tp = 0, fp = 0;
    for (int i = t; i < n; i += MT) {
      const bool pos = (double)key_score((uint32_t)(key[i] >> 32)) >= thr;
      const bool lab = (key[i] & 1ull) != 0;
      tp += (pos && lab) ? 1 : 0;
      fp += (pos && !lab) ? 1 : 0;
    }
    __syncthreads();
    part[t] = tp; redI[t] = fp;
    __syncthreads();
    if (t == 0) {
      long long a = 0, b = 0;
      for (int w = 0; w < MT; ++w) { a += part[w]; b += redI[w]; }
      redA[0] = a; redA[1] = b;
    }
    __syncthreads();
    TP = redA[0]; FP = redA[1];
  }
  if (t == 0) {
    const long long FN = P - TP, TN = Nn - FP;
    o[2] = (double)(TP + TN) / (double)n;                // accuracy
    o[3] = (double)TP / (double)(TP + FN);               // recall / sensitivity
    o[4] = (double)TN / (double)(TN + FP);               // specificity
  }
}

__global__ __launch_bounds__(MT) void confusion_kernel(const int32_t* __restrict__ pred, const int32_t* __restrict__ labels,
                                                       const int32_t* __restrict__ offsets, double* __restrict__ out) {
  __shared__ int32_t cnt[4][MT];
  const int s = blockIdx.x, t = threadIdx.x;
  const int base = offsets[s], n = offsets[s + 1] - base;
  int tp = 0, fp = 0, tn = 0, fn = 0;
  for (int i = t; i < n; i += MT) {
    const bool p = pred[base + i] != 0, l = labels[base + i] != 0;
    tp += (p && l); fp += (p && !l); tn += (!p && !l); fn += (!p && l);
  }
  cnt[0][t] = tp; cnt[1][t] = fp; cnt[2][t] = tn; cnt[3][t] = fn;
  __syncthreads();
  if (t == 0) {
    long long TP = 0, FP = 0, TN = 0, FN = 0;
    for (int w = 0; w < MT; ++w) { TP += cnt[0][w]; FP += cnt[1][w]; TN += cnt[2][w]; FN += cnt[3][w]; }
    double* o = out + (int64_t)s * NM_METRICS_STRIDE;
    const double qnan = __longlong_as_double(0x7FF8000000000000ll);
    const double sens = (TP + FN) ? (double)TP / (double)(TP + FN) : 0.0;          // recall_score: 0 when undefined
    const double spec = (double)TN / (double)(TN + FP);                            // numpy division: nan when 0/0
    o[0] = n > 0 ? (double)(TP + TN) / (double)n : qnan;                           // accuracy_score
    // roc_auc_score on hard predictions = mean of the two rates; ValueError (-> nan) with one class present
    o[1] = ((TP + FN) && (TN + FP)) ? 0.5 * ((double)TP / (double)(TP + FN) + (double)TN / (double)(TN + FP)) : qnan;
    o[2] = sens;
    o[3] = spec;
    o[4] = (2 * TP + FP + FN) ? 2.0 * (double)TP / (double)(2 * TP + FP + FN) : 0.0;   // f1_score
    o[5] = (TP + FP) ? (double)TP / (double)(TP + FP) : 0.0;                       // precision_score
    o[6] = (double)(TP + FN);
    o[7] = (double)(TN + FP);
  }
}

constexpr int METRICS_SMEM = MAXN * (8 + 4 + 4);

// ---- latent deviation (utils_vae.py:155-161): cohort statistics of the exported joint mu, then the z-scores -------------
// nm_latent_stats: one workgroup per cohort (a segment of the concatenated [rows][pitch] array).  A thread owns one
// (128-row chunk, column) pair at a time: the chunk's mean and its sum of squared deviations from that mean, two passes in
// fp64; thread z < Z then merges the chunks' partials in row order with Chan's formula.  No atomics, a fixed order of
// every sum: the result is the same run to run.  Rounded once to fp32 at the end.
constexpr int LAT_CHUNK = 128;

__global__ __launch_bounds__(MT) void latent_stats_kernel(const float* __restrict__ mu, const int32_t* __restrict__ offsets, int Z,
                                                          int pitch, float* __restrict__ mean_out, float* __restrict__ var_out) {
  __shared__ double pmean[MT], pm2[MT];
  const int s = blockIdx.x, t = threadIdx.x;
  const int base = offsets[s], n = offsets[s + 1] - base;
  if (n <= 0) {                                                 // an empty cohort has no statistics
    if (t < Z) { mean_out[(int64_t)s * Z + t] = __int_as_float(0x7FC00000); var_out[(int64_t)s * Z + t] = __int_as_float(0x7FC00000); }
    return;
  }
  const int per = MT / Z;                                       // chunks per round (Z <= 64: at least 4)
  const int nchunks = (n + LAT_CHUNK - 1) / LAT_CHUNK;
  const int cl = t / Z, z = t - cl * Z;
  double cnt = 0.0, mean = 0.0, m2 = 0.0;                       // thread z < Z: the running statistics of column z
  for (int c0 = 0; c0 < nchunks; c0 += per) {
    const int ch = c0 + cl;
    if (cl < per && ch < nchunks) {
      const int r0 = ch * LAT_CHUNK, r1 = min(r0 + LAT_CHUNK, n);
      const float* col = mu + (int64_t)(base + r0) * pitch + z;
      double sum = 0.0;
      for (int r = 0; r < r1 - r0; ++r) sum += (double)col[(int64_t)r * pitch];
      const double cm = sum / (double)(r1 - r0);
      double q = 0.0;
      for (int r = 0; r < r1 - r0; ++r) { const double d = (double)col[(int64_t)r * pitch] - cm; q += d * d; }
      pmean[t] = cm; pm2[t] = q;
    }
    __syncthreads();
    if (t < Z) {
      for (int k = 0; k < per && c0 + k < nchunks; ++k) {
        const double nb = (double)(min((c0 + k + 1) * LAT_CHUNK, n) - (c0 + k) * LAT_CHUNK);
        const double delta = pmean[k * Z + t] - mean, tot = cnt + nb;
        mean += delta * (nb / tot);
        m2 += pm2[k * Z + t] + delta * delta * (cnt * nb / tot);
        cnt = tot;
      }
    }
    __syncthreads();
  }
  if (t < Z) {
    mean_out[(int64_t)s * Z + t] = (float)mean;
    var_out[(int64_t)s * Z + t] = (float)(m2 / cnt);            // population variance (np.var, ddof 0)
  }
}

// nm_latent_score: one workgroup per set, a thread per row.  The library's expf / sqrtf / division (<= 1 ulp, correctly
// rounded, correctly rounded); no product anywhere, so nothing for the compiler to contract.
__global__ __launch_bounds__(MT) void latent_score_kernel(const float* __restrict__ mu, const float* __restrict__ logvar,
                                                          const int32_t* __restrict__ offsets, int Z, int pitch,
                                                          const float* __restrict__ mean, const float* __restrict__ var,
                                                          float* __restrict__ zsep_out, float* __restrict__ score_out) {
  __shared__ float smean[NM_MAX_LATENT], svar[NM_MAX_LATENT];
  const int s = blockIdx.x, t = threadIdx.x;
  const int base = offsets[s], n = offsets[s + 1] - base;
  if (t < Z) { smean[t] = mean[(int64_t)s * Z + t]; svar[t] = var[(int64_t)s * Z + t]; }
  __syncthreads();
  for (int r = t; r < n; r += MT) {
    const int64_t row = (int64_t)(base + r) * pitch;
    float acc = 0.f;
    for (int z = 0; z < Z; ++z) {
      const float a = mu[row + z] - smean[z];
      const float d = sqrtf(svar[z] + expf(logvar[row + z]));
      if (zsep_out) zsep_out[row + z] = a / d;
      acc += fabsf(a) / d;
    }
    if (score_out) score_out[base + r] = acc / (float)Z;
  }
}

// ---- ROI-wise group effect sizes (cliff_delta, utils.py:97-109, for every column of a table at once) --------------------
// nm_roi_effect: one workgroup per (set, 64-column tile), a lane per column, so a wave reads 64 consecutive floats of a row.
// The group words are read first: the set's X rows (group 1) are listed from the front of an LDS index array, its Y rows
// (group 0) from its back, both in row order; every other row is on neither list.  The Y rows then pass through LDS in
// chunks of NM_ROI_Y_CHUNK rows ([row][column]: consecutive lanes on consecutive banks); the four waves take every fourth
// X row, ROI_XR of them at a time in registers, so one LDS read serves ROI_XR pairs and each pair is two compares whose
// results are added to int32 counters (a thread sees at most 8192 / 4 x 8192 pairs).  A NaN compares false both ways: its
// pairs are ties.  Group sums in fp64, per thread in the order of its rows; counters and sums of the four waves are merged
// through LDS in wave order -- no atomics, the same bits on every run -- and the two quotients are single IEEE divisions
// of exactly represented integers.
constexpr int ROI_TILE = 64;                      // columns per workgroup
constexpr int ROI_WAVES = MT / 64;
constexpr int ROI_XR = 8;                         // X rows a thread holds while a Y chunk streams past
constexpr int ROI_YCH = NM_ROI_Y_CHUNK;
static_assert(sizeof(nm_roi_set_t) == 24, "nm_roi_set_t is mirrored by _lib.NmRoiSet");
static_assert(ROI_YCH * ROI_TILE * 4 >= ROI_WAVES * ROI_TILE * (4 + 4 + 8 + 8), "the merge arrays reuse the Y chunk");

__global__ __launch_bounds__(MT) void roi_effect_kernel(const nm_roi_set_t* __restrict__ sets, int D, int max_rows, int tiles,
                                                        double* __restrict__ out) {
  __shared__ __attribute__((aligned(16))) float ys[ROI_YCH * ROI_TILE];      // the Y chunk; at the end the merge arrays
  __shared__ uint16_t idx[MAXN];                                             // X rows from [0] up, Y rows from [MAXN - 1] down
  __shared__ int32_t part[2][MT];

  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  const int s = blockIdx.x / tiles, tile = blockIdx.x - s * tiles;
  const nm_roi_set_t S = sets[s];
  const int col = tile * ROI_TILE + lane;
  const bool cv = col < D;
  double* o = out + ((int64_t)s * D + col) * NM_METRICS_STRIDE;
  const double qnan = __longlong_as_double(0x7FF8000000000000ll);
  const int rows = S.rows, pitch = S.pitch;
  if (rows < 0 || rows > max_rows || pitch < D || (rows > 0 && (!S.x || !S.group))) {
    if (w == 0 && cv)
      for (int k = 0; k < NM_METRICS_STRIDE; ++k) o[k] = qnan;
    return;
  }
  // the two row lists: a thread counts its stretch of rows, takes its place from the counts before it, writes its rows
  const int per = (rows + MT - 1) / MT;
  const int lo = min(t * per, rows), hi = min(lo + per, rows);
  {
    int cx = 0, cy = 0;
    for (int r = lo; r < hi; ++r) { const int32_t g = S.group[r]; cx += (g == 1); cy += (g == 0); }
    part[0][t] = cx; part[1][t] = cy;
  }
  __syncthreads();
  int nx = 0, ny = 0;
  {
    int bx = 0, by = 0;
    for (int q = 0; q < MT; ++q) {
      const int cx = part[0][q], cy = part[1][q];
      if (q < t) { bx += cx; by += cy; }
      nx += cx; ny += cy;
    }
    for (int r = lo; r < hi; ++r) {
      const int32_t g = S.group[r];
      if (g == 1) idx[bx++] = (uint16_t)r;
      else if (g == 0) idx[MAXN - 1 - by++] = (uint16_t)r;
    }
  }
  const float* xc = S.x + col;                     // (read only where cv: beyond D lies padding, or the next row)
  int32_t more[ROI_XR], less[ROI_XR];
#pragma unroll
  for (int k = 0; k < ROI_XR; ++k) { more[k] = 0; less[k] = 0; }
  double sumx = 0.0, sumy = 0.0;
  for (int y0 = 0; y0 == 0 || y0 < ny; y0 += ROI_YCH) {          // (once with an empty chunk when there is no Y row: X's sums)
    const int yn = min(ROI_YCH, ny - y0);
    __syncthreads();                               // the lists are written / the chunk before this one is used up
    for (int r = w; r < yn; r += ROI_WAVES) {
      const float v = cv ? xc[(int64_t)idx[MAXN - 1 - (y0 + r)] * pitch] : 0.f;
      ys[r * ROI_TILE + lane] = v;
      sumy += (double)v;
    }
    __syncthreads();
    for (int p0 = w; p0 < nx; p0 += ROI_WAVES * ROI_XR) {
      float xv[ROI_XR];
#pragma unroll
      for (int k = 0; k < ROI_XR; ++k) {
        const int p = p0 + ROI_WAVES * k;
        xv[k] = (p < nx && cv) ? xc[(int64_t)idx[min(p, nx - 1)] * pitch] : __int_as_float(0x7FC00000);   // NaN: counts nothing
      }
      if (y0 == 0) {
#pragma unroll
        for (int k = 0; k < ROI_XR; ++k)
          if (p0 + ROI_WAVES * k < nx) sumx += (double)xv[k];
      }
#pragma unroll 4
      for (int j = 0; j < yn; ++j) {
        const float y = ys[j * ROI_TILE + lane];
#pragma unroll
        for (int k = 0; k < ROI_XR; ++k) {
          more[k] += (xv[k] > y) ? 1 : 0;
          less[k] += (xv[k] < y) ? 1 : 0;
        }
      }
    }
  }
  __syncthreads();                                 // the last chunk is used up: its place takes the waves' partial results
  int32_t* pm = reinterpret_cast<int32_t*>(ys);                         // [ROI_WAVES][ROI_TILE] each
  int32_t* pl = pm + ROI_WAVES * ROI_TILE;
  double* px = reinterpret_cast<double*>(pl + ROI_WAVES * ROI_TILE);
  double* py = px + ROI_WAVES * ROI_TILE;
  {
    int32_t m = 0, l = 0;
#pragma unroll
    for (int k = 0; k < ROI_XR; ++k) { m += more[k]; l += less[k]; }
    pm[t] = m; pl[t] = l; px[t] = sumx; py[t] = sumy;
  }
  __syncthreads();
  if (w == 0 && cv) {
    long long M = 0, L = 0;
    double sx = 0.0, sy = 0.0;
    for (int q = 0; q < ROI_WAVES; ++q) {
      M += pm[q * ROI_TILE + lane]; L += pl[q * ROI_TILE + lane];
      sx += px[q * ROI_TILE + lane]; sy += py[q * ROI_TILE + lane];
    }
    const long long pairs = (long long)nx * ny, ties = pairs - M - L;
    o[0] = pairs ? (double)(M - L) / (double)pairs : qnan;              // cliff_delta
    o[1] = pairs ? (double)(2 * M + ties) / (double)(2 * pairs) : qnan; // ROC-AUC of the column as a patient score
    o[2] = (double)M;
    o[3] = (double)L;
    o[4] = (double)nx;
    o[5] = (double)ny;
    o[6] = nx ? sx / (double)nx : qnan;
    o[7] = ny ? sy / (double)ny : qnan;
  }
}

// ---- ROI-wise significance (Mann-Whitney p, Benjamini-Hochberg q, max-statistic label permutations) --------------------
// nm_roi_significance, six launches on one stream over a workspace (include/nmhip.h has the definitions):
//   rank   one workgroup per (set, column): the included rows' (order-preserving key of the value, position, is-X) as 64-bit
//          keys, bitonic-sorted in LDS as posthoc_kernel sorts; a thread that finds the first key of a tie run walks the run
//          and writes twice its mid-rank for every member to r2 [set][position][D] (uint16), and the column's tie term, S
//          and validity.  -0 and +0 share a key.
//   label  one workgroup per (set, permutation): the n hash keys sorted the same way, the n_x smallest marked in a byte
//          array, the bytes gathered into ceil(max_rows / 32) label words.
//   sum    one workgroup per (set, 64-column tile, NM_ROI_PERM_CHUNK permutations), a lane per column.  The tile's rank rows
//          pass through LDS NM_ROI_ROW_CHUNK rows at a time ([row][column] uint16: a wave reads 128 consecutive bytes); each
//          of the four waves carries SIG_PW permutations in int32 accumulators, reads a row once and adds it SIG_PW times
//          as v * bit, the bit taken from a label word that is the same for the whole wave (a scalar operand: one multiply-
//          add per row and permutation).  Per permutation the tile's largest |S*| over valid columns (a wave reduction), per
//          column the chunk's count of |S*| >= |S| (the waves' counts merged through LDS in wave order).
//   max    the tiles' maxima -> maxstat_t;  count: per column the chunks' counts added in chunk order and the number of
//          maxstat_t >= |S|;  close: one workgroup per set -- z and p per column, the BH sort over the columns in LDS, the
//          suffix minimum, the table.
// No atomics; integers until the last divisions.
constexpr int SIG_PW = 16;                         // permutations a wave carries through a row chunk
constexpr int SIG_PCH = NM_ROI_PERM_CHUNK;
constexpr int SIG_RCH = NM_ROI_ROW_CHUNK;
constexpr int SIG_MAX_D = 8192;                    // the BH sort's limit
static_assert(SIG_PCH == ROI_WAVES * SIG_PW, "a chunk is what the four waves carry");
static_assert(SIG_RCH % 32 == 0 && MAXN % SIG_RCH == 0, "row chunks are whole label words");

struct SigPlan {                                   // byte offsets into the workspace, each a multiple of 256
  size_t r2, colS, coltie, info, lab, tmax, ccnt, ms, cnt, total;
  int W, tiles, chunks;
};
inline SigPlan sig_plan(int n_sets, int D, int max_rows, int n_perm) {
  SigPlan p;
  p.W = (max_rows + 31) / 32;
  p.tiles = (D + ROI_TILE - 1) / ROI_TILE;
  p.chunks = (n_perm + SIG_PCH - 1) / SIG_PCH;
  const size_t ns = (size_t)n_sets, sd = ns * (size_t)D, sp = ns * (size_t)n_perm;
  size_t o = 0;
  auto take = [&o](size_t bytes) { const size_t at = o; o += (bytes + 255) & ~(size_t)255; return at; };
  p.r2 = take(sd * (size_t)max_rows * 2);          // uint16 [set][position][D]
  p.colS = take(sd * 4);                           // int32  [set][D]
  p.coltie = take(sd * 8);                         // double [set][D]: the tie term, -1 where the column is not valid
  p.info = take(ns * 16);                          // int32  [set][4]: n, n_x, usable
  p.lab = take(sp * (size_t)p.W * 4);              // uint32 [set][perm][W]
  p.tmax = take(sp * (size_t)p.tiles * 4);         // int32  [set][perm][tile]
  p.ccnt = take(ns * (size_t)p.chunks * (size_t)D * 4);   // int32 [set][chunk][D]
  p.ms = take(sp * 4);                             // int32  [set][perm]
  p.cnt = take(sd * 8);                            // int32  [set][D][2]: #|S*| >= |S|, #maxstat >= |S|
  p.total = o;
  return p;
}
inline int pow2_at_least(int n) { int p = 2; while (p < n) p <<= 1; return p; }

__device__ __forceinline__ uint64_t sig_splitmix64(uint64_t x) {      // splitmix64 of nm_core.inc
  x += 0x9E3779B97F4A7C15ull;
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
  return x ^ (x >> 31);
}
__device__ __forceinline__ uint32_t asc_key(float x) {
  if (x == 0.0f) x = 0.0f;                               // -0 and +0 are one value
  const uint32_t b = __float_as_uint(x);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
// ascending bitonic sort of key[0..npad), npad a power of two; all threads call
__device__ __forceinline__ void sort_keys(uint64_t* key, int npad) {
  const int t = threadIdx.x;
  for (int k = 2; k <= npad; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int i = t; i < npad; i += MT) {
        const int p = i ^ j;
        if (p > i) {
          const uint64_t a = key[i], b = key[p];
          if ((a > b) == ((i & k) == 0)) { key[i] = b; key[p] = a; }
        }
      }
      __syncthreads();
    }
  }
}

__global__ __launch_bounds__(MT) void roi_rank_kernel(const nm_roi_set_t* __restrict__ sets, int D, int max_rows,
                                                      uint16_t* __restrict__ r2, int32_t* __restrict__ colS,
                                                      double* __restrict__ coltie, int32_t* __restrict__ info) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  uint64_t* key = reinterpret_cast<uint64_t*>(smem);            // [npad]: value key << 32 | position << 1 | is X
  __shared__ int32_t part[2][MT];
  __shared__ long long red[2][MT];
  const int t = threadIdx.x;
  const int s = blockIdx.x / D, col = blockIdx.x - s * D;
  const nm_roi_set_t S = sets[s];
  const int64_t ci = (int64_t)s * D + col;
  const int rows = S.rows, pitch = S.pitch;
  if (rows < 0 || rows > max_rows || pitch < D || (rows > 0 && (!S.x || !S.group))) {
    if (t == 0) {
      colS[ci] = 0; coltie[ci] = -1.0;
      if (col == 0) { info[4 * s] = 0; info[4 * s + 1] = 0; info[4 * s + 2] = 0; info[4 * s + 3] = 0; }
    }
    return;
  }
  const int per = (rows + MT - 1) / MT;
  const int lo = min(t * per, rows), hi = min(lo + per, rows);
  {
    int cn = 0, cx = 0;
    for (int r = lo; r < hi; ++r) { const int32_t g = S.group[r]; cn += (g == 1 || g == 0); cx += (g == 1); }
    part[0][t] = cn; part[1][t] = cx;
  }
  __syncthreads();
  int n = 0, nx = 0, pos = 0;
  for (int q = 0; q < MT; ++q) {
    const int cn = part[0][q];
    if (q < t) pos += cn;
    n += cn; nx += part[1][q];
  }
  const bool usable = nx >= 1 && n - nx >= 1;
  if (t == 0 && col == 0) { info[4 * s] = n; info[4 * s + 1] = nx; info[4 * s + 2] = usable ? 1 : 0; info[4 * s + 3] = 0; }
  if (!usable) {
    if (t == 0) { colS[ci] = 0; coltie[ci] = -1.0; }
    return;
  }
  const int npad = [n] { int p = 2; while (p < n) p <<= 1; return p; }();
  for (int i = n + t; i < npad; i += MT) key[i] = ~0ull;
  int nan = 0;
  for (int r = lo; r < hi; ++r) {
    const int32_t g = S.group[r];
    if (g == 1 || g == 0) {
      const float v = S.x[(int64_t)r * pitch + col];
      nan |= (v != v);
      key[pos] = ((uint64_t)asc_key(v) << 32) | ((uint64_t)pos << 1) | (uint64_t)(g == 1);
      ++pos;
    }
  }
  if (__syncthreads_or(nan)) {                     // a NaN in an included row: the column is not valid
    if (t == 0) { colS[ci] = 0; coltie[ci] = -1.0; }
    return;
  }
  sort_keys(key, npad);
  long long sumx = 0, tie = 0;
  uint16_t* rc = r2 + (int64_t)s * max_rows * D + col;
  for (int j = t; j < n; j += MT) {
    const uint32_t v = (uint32_t)(key[j] >> 32);
    if (j > 0 && (uint32_t)(key[j - 1] >> 32) == v) continue;   // not the first of its tie run
    int e = j + 1;
    while (e < n && (uint32_t)(key[e] >> 32) == v) ++e;
    const long long tn = e - j;
    tie += tn * tn * tn - tn;
    const int rr = j + 1 + e;                      // twice the mid-rank of ranks j + 1 .. e
    for (int q = j; q < e; ++q) {
      const uint32_t low = (uint32_t)key[q];
      rc[(int64_t)((low >> 1) & 0x1FFFu) * D] = (uint16_t)rr;
      if (low & 1u) sumx += rr;
    }
  }
  red[0][t] = sumx; red[1][t] = tie;
  __syncthreads();
  if (t == 0) {
    long long sx = 0, tt = 0;
    for (int q = 0; q < MT; ++q) { sx += red[0][q]; tt += red[1][q]; }
    colS[ci] = (int32_t)(sx - (long long)nx * (n + 1));
    coltie[ci] = (double)tt;
  }
}

__global__ __launch_bounds__(MT) void roi_label_kernel(const int32_t* __restrict__ info, int n_perm, int W, uint64_t seed,
                                                       uint32_t* __restrict__ lab) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  uint64_t* key = reinterpret_cast<uint64_t*>(smem);            // [npad]
  __shared__ uint8_t flag[MAXN];
  const int t = threadIdx.x;
  const int s = blockIdx.x / n_perm, p = blockIdx.x - s * n_perm;
  const int n = info[4 * s], nx = info[4 * s + 1];
  if (!info[4 * s + 2]) return;                    // no valid column in this set: nothing reads its labels
  int npad = 2;
  while (npad < n) npad <<= 1;
  const uint64_t base = seed ^ 0x5160C0DEull ^ ((uint64_t)s << 40) ^ ((uint64_t)(p + 1) << 16);
  for (int i = t; i < npad; i += MT)
    key[i] = (i < n) ? ((sig_splitmix64(base ^ (uint64_t)i) & ~0x1FFFull) | (uint64_t)i) : ~0ull;
  for (int i = t; i < W * 32; i += MT) flag[i] = 0;
  __syncthreads();
  sort_keys(key, npad);
  for (int j = t; j < nx; j += MT) flag[(uint32_t)key[j] & 0x1FFFu] = 1;
  __syncthreads();
  for (int wd = t; wd < W; wd += MT) {
    uint32_t word = 0;
#pragma unroll
    for (int b = 0; b < 32; ++b) word |= (uint32_t)flag[wd * 32 + b] << b;
    lab[((int64_t)s * n_perm + p) * W + wd] = word;
  }
}

// acc + v * bit with the bit in a scalar register: one v_mad_u32_u24 per (row, permutation).  (Left to itself the compiler
// forms a 0 / -1 mask, an AND and an add3 over two rows: three instructions for two.)
__device__ __forceinline__ int32_t mad_bit(uint32_t v, uint32_t bit, int32_t acc) {
  int32_t r;
  asm("v_mad_u32_u24 %0, %1, %2, %3" : "=v"(r) : "v"(v), "s"(bit), "v"(acc));
  return r;
}

__global__ __launch_bounds__(MT) void roi_sum_kernel(const int32_t* __restrict__ info, const uint16_t* __restrict__ r2,
                                                     const int32_t* __restrict__ colS, const double* __restrict__ coltie,
                                                     const uint32_t* __restrict__ lab, int D, int max_rows, int n_perm, int W,
                                                     int tiles, int chunks, int32_t* __restrict__ tmax,
                                                     int32_t* __restrict__ ccnt) {
  __shared__ uint16_t rs[SIG_RCH * ROI_TILE];
  __shared__ int32_t pc[ROI_WAVES][ROI_TILE];
  const int t = threadIdx.x, lane = t & 63;
  const int w = __builtin_amdgcn_readfirstlane(t >> 6);
  int b = blockIdx.x;
  const int chunk = b % chunks; b /= chunks;
  const int tile = b % tiles, s = b / tiles;
  const int n = info[4 * s], nx = info[4 * s + 1];
  if (!info[4 * s + 2]) return;                    // (the max and close kernels know it from the same word)
  const int col = tile * ROI_TILE + lane;
  const bool cv = col < D;
  const int64_t ci = (int64_t)s * D + (cv ? col : 0);
  const bool valid = cv && coltie[ci] >= 0.0;
  const int absS = valid ? abs(colS[ci]) : 0;
  const int p0 = chunk * SIG_PCH + w * SIG_PW;     // this wave's first permutation (0-based)
  const int pw = max(0, min(SIG_PW, n_perm - p0));
  const uint32_t* lw[SIG_PW];
#pragma unroll
  for (int k = 0; k < SIG_PW; ++k) lw[k] = lab + ((int64_t)s * n_perm + min(p0 + k, n_perm - 1)) * W;
  int32_t acc[SIG_PW];
#pragma unroll
  for (int k = 0; k < SIG_PW; ++k) acc[k] = 0;
  const uint16_t* rc = r2 + (int64_t)s * max_rows * D + col;
  for (int r0 = 0; r0 < n; r0 += SIG_RCH) {
    const int rn = min(SIG_RCH, n - r0);
    __syncthreads();                               // the chunk before this one is used up
    for (int r = w; r < rn; r += ROI_WAVES) rs[r * ROI_TILE + lane] = cv ? rc[(int64_t)(r0 + r) * D] : (uint16_t)0;
    __syncthreads();
    if (pw > 0) {
      const int ng = (rn + 31) >> 5;               // (rows past rn within the last word: their label bits are 0)
      for (int g = 0; g < ng; ++g) {
        uint32_t wk[SIG_PW];
#pragma unroll
        for (int k = 0; k < SIG_PW; ++k) wk[k] = lw[k][(r0 >> 5) + g];
#pragma unroll
        for (int bit = 0; bit < 32; ++bit) {
          const uint32_t v = rs[((g << 5) + bit) * ROI_TILE + lane];
#pragma unroll
          for (int k = 0; k < SIG_PW; ++k) acc[k] = mad_bit(v, (wk[k] >> bit) & 1u, acc[k]);
        }
      }
    }
  }
  const int center = nx * (n + 1);
  int cnt = 0;
#pragma unroll
  for (int k = 0; k < SIG_PW; ++k) {
    const int a = abs(acc[k] - center);
    const bool live = k < pw;
    cnt += (live && valid && a >= absS) ? 1 : 0;
    int m = valid ? a : -1;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) m = max(m, __shfl_xor(m, off, 64));
    if (live && lane == 0) tmax[((int64_t)s * n_perm + p0 + k) * tiles + tile] = m;
  }
  pc[w][lane] = cnt;
  __syncthreads();
  if (w == 0 && cv) ccnt[((int64_t)s * chunks + chunk) * D + col] = pc[0][lane] + pc[1][lane] + pc[2][lane] + pc[3][lane];
}

__global__ __launch_bounds__(MT) void roi_max_kernel(const int32_t* __restrict__ info, const int32_t* __restrict__ tmax,
                                                     int n_perm, int tiles, int pblocks, int32_t* __restrict__ ms,
                                                     int32_t* __restrict__ maxstat_out) {
  const int s = blockIdx.x / pblocks, p = (blockIdx.x - s * pblocks) * MT + threadIdx.x;
  if (p >= n_perm) return;
  int m = -1;
  if (info[4 * s + 2])
    for (int tile = 0; tile < tiles; ++tile) m = max(m, tmax[((int64_t)s * n_perm + p) * tiles + tile]);
  ms[(int64_t)s * n_perm + p] = m;
  if (maxstat_out) maxstat_out[(int64_t)s * n_perm + p] = m;
}

__global__ __launch_bounds__(MT) void roi_count_kernel(const int32_t* __restrict__ info, const int32_t* __restrict__ colS,
                                                       const int32_t* __restrict__ ccnt, const int32_t* __restrict__ ms, int D,
                                                       int n_perm, int chunks, int dblocks, int32_t* __restrict__ cnt) {
  const int s = blockIdx.x / dblocks, col = (blockIdx.x - s * dblocks) * MT + threadIdx.x;
  if (col >= D) return;
  const int64_t ci = (int64_t)s * D + col;
  int cp = 0, cm = 0;
  if (info[4 * s + 2]) {
    const int absS = abs(colS[ci]);
    for (int c = 0; c < chunks; ++c) cp += ccnt[((int64_t)s * chunks + c) * D + col];
    const int32_t* m = ms + (int64_t)s * n_perm;
    for (int p = 0; p < n_perm; ++p) cm += (m[p] >= absS) ? 1 : 0;
  }
  cnt[2 * ci] = cp; cnt[2 * ci + 1] = cm;
}

// z and the asymptotic p of one column: every operation on its own, in the order of the definitions
#pragma clang fp contract(off)
__device__ __forceinline__ void mwu_z_p(int n, int nx, int S, double tie, double& z, double& p) {
  const double a = (double)((long long)nx * (n - nx)) / 12.0;
  const double b = tie / ((double)n * (double)(n - 1));
  const double sd = __dsqrt_rn(a * ((double)(n + 1) - b));
  const double zabs = sd > 0.0 ? fmax(fabs((double)S) * 0.5 - 0.5, 0.0) / sd : 0.0;
  z = copysign(zabs, (double)S);
  p = erfc(zabs / 1.4142135623730951);              // sqrt(2.0), correctly rounded
}

__global__ __launch_bounds__(MT) void roi_close_kernel(const int32_t* __restrict__ info, const int32_t* __restrict__ colS,
                                                       const double* __restrict__ coltie, const int32_t* __restrict__ cnt, int D,
                                                       int npad, int n_perm, double* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  uint64_t* key = reinterpret_cast<uint64_t*>(smem);            // [npad]: the bits of p (p >= 0: their order is p's)
  uint16_t* idx = reinterpret_cast<uint16_t*>(key + npad);      // [npad]: the column of key[j]
  __shared__ int32_t part[MT];
  __shared__ double dpart[MT];
  const int s = blockIdx.x, t = threadIdx.x;
  const int n = info[4 * s], nx = info[4 * s + 1], usable = info[4 * s + 2];
  const double qnan = __longlong_as_double(0x7FF8000000000000ll);
  int mine = 0;
  for (int c = t; c < npad; c += MT) {
    uint64_t k = ~0ull;
    if (c < D) {
      const int64_t ci = (int64_t)s * D + c;
      double* o = out + ci * NM_METRICS_STRIDE;
      const double tie = usable ? coltie[ci] : -1.0;
      if (tie >= 0.0) {
        const int S = colS[ci];
        double z, p;
        mwu_z_p(n, nx, S, tie, z, p);
        o[0] = (double)((long long)S + (long long)nx * (n - nx)) * 0.5;
        o[1] = tie; o[2] = z; o[3] = p;
        o[5] = n_perm ? (double)(1 + cnt[2 * ci]) / (double)(1 + n_perm) : qnan;
        o[6] = n_perm ? (double)(1 + cnt[2 * ci + 1]) / (double)(1 + n_perm) : qnan;
        o[7] = (double)n_perm;
        k = (uint64_t)__double_as_longlong(p);
        ++mine;
      } else {
        for (int q = 0; q < NM_METRICS_STRIDE; ++q) o[q] = qnan;
      }
    }
    key[c] = k; idx[c] = (uint16_t)c;
  }
  part[t] = mine;
  __syncthreads();
  int m = 0;
  for (int q = 0; q < MT; ++q) m += part[q];
  // ascending in p, the column riding along
  for (int k = 2; k <= npad; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int i = t; i < npad; i += MT) {
        const int p = i ^ j;
        if (p > i) {
          const uint64_t a = key[i], b = key[p];
          if ((a > b) == ((i & k) == 0)) {
            key[i] = b; key[p] = a;
            const uint16_t ia = idx[i]; idx[i] = idx[p]; idx[p] = ia;
          }
        }
      }
      __syncthreads();
    }
  }
  // q_(i) = min(1, min_{j >= i} p_(j) * (m / j)): the products in place, then the suffix minimum by stretches
  double* v = reinterpret_cast<double*>(key);
  const int per = (m + MT - 1) / MT;
  const int lo = min(t * per, m), hi = min(lo + per, m);
  double run = __longlong_as_double(0x7FF0000000000000ll);
  for (int j = hi - 1; j >= lo; --j) {
    const double pj = __longlong_as_double((long long)key[j]);
    run = fmin(run, pj * ((double)m / (double)(j + 1)));
    v[j] = run;
  }
  dpart[t] = run;
  __syncthreads();
  double tail = __longlong_as_double(0x7FF0000000000000ll);
  for (int q = t + 1; q < MT; ++q) tail = fmin(tail, dpart[q]);
  for (int j = lo; j < hi; ++j)
    out[((int64_t)s * D + idx[j]) * NM_METRICS_STRIDE + 4] = fmin(1.0, fmin(v[j], tail));
}

// ---- bootstrap of the per-subject ROC-AUC, paired comparison (include/nmhip.h has the definitions) ---------------------
// nm_auc_bootstrap, three launches on one stream over a workspace:
//   prepare   one workgroup per set: the (value key, ordinal within its class, is-positive) triples as 64-bit keys, sorted
//             once in LDS; the distinct values numbered g = 0..G-1 (a scan over the boundaries); per positive ordinal and per
//             negative ordinal its value group (uint16, positives first); G, n_pos, n_neg, A2 and the validity to info.
//   resample  one workgroup per (set, NM_BOOT_CHUNK resamples), a wave per resample in flight.  With V the histogram of the
//             resample's negative draws over the value groups and C its inclusive prefix sum (C[-1] = 0),
//             A2* = sum over positive draws of C[g - 1] + C[g]  (= 2 #{smaller negatives} + #{equal negatives}):
//             n_neg hashed increments into the wave's LDS histogram, one wave scan over G bins, n_pos hashed gathers.  No
//             sort and no float per resample.  The LDS is sized from max_set: the set's groups once, a histogram per wave.
//   close     one workgroup per set and per pair: the n_boot integers (differences) as biased uint32 keys in LDS, the two
//             order statistics by radix selection over them (no sort: two of n_boot ranks are asked for), the counts, and the
//             sums as integers: sum d in int64, sum (d - m)^2 about the integer
//             m = sum d / n_boot in 128 bits, so T = n_boot sum (d - m)^2 - (sum d - n_boot m)^2 is exact.
// Integer LDS atomics only (their sum has no order).
constexpr int BOOT_CHUNK = NM_BOOT_CHUNK;
constexpr int BOOT_WAVES = MT / 64;
constexpr int BOOT_INFO = 8;                       // int32 per set: n, n_pos, n_neg, G, A2, valid, stream id, 0
static_assert(BOOT_CHUNK % BOOT_WAVES == 0, "every wave of the resample pass makes the same number of rounds");
static_assert(NM_BOOT_MAX * 4 <= 64 * 1024, "the close pass holds n_boot int32 in LDS");
static_assert(MT == 256, "the close pass's radix selection has a bin per thread");

struct BootPlan {                                  // byte offsets into the workspace, each a multiple of 256
  size_t info, grp, boot, total;
  int chunks, hpitch, grp_lds, resample_lds;
};
inline BootPlan boot_plan(int n_sets, int max_set, int n_boot) {
  BootPlan p;
  const size_t ns = (size_t)n_sets;
  size_t o = 0;
  auto take = [&o](size_t bytes) { const size_t at = o; o += (bytes + 255) & ~(size_t)255; return at; };
  p.info = take(ns * BOOT_INFO * 4);               // int32  [set][BOOT_INFO]
  p.grp = take(ns * (size_t)max_set * 2);          // uint16 [set][max_set]: the positives' groups, then the negatives'
  p.boot = take(ns * (size_t)n_boot * 4);          // int32  [set][n_boot]
  p.total = o;
  p.chunks = (n_boot + BOOT_CHUNK - 1) / BOOT_CHUNK;
  p.hpitch = max_set + 1;                          // a wave's histogram: C[-1] and at most max_set groups
  p.grp_lds = (max_set * 2 + 15) & ~15;
  p.resample_lds = p.grp_lds + BOOT_WAVES * p.hpitch * 4;
  return p;
}

__global__ __launch_bounds__(MT) void boot_prepare_kernel(const float* __restrict__ scores, const int32_t* __restrict__ labels,
                                                          const int32_t* __restrict__ offsets, const int32_t* __restrict__ streams,
                                                          int max_set, int npad_max, uint16_t* __restrict__ grp,
                                                          int32_t* __restrict__ info) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  uint64_t* key = reinterpret_cast<uint64_t*>(smem);            // [npad_max]: value key << 32 | ordinal << 1 | is positive
  int32_t* arr = reinterpret_cast<int32_t*>(key + npad_max);    // [npad_max]: label prefix sums, then the group numbers
  __shared__ int32_t part[MT];
  __shared__ long long red[MT];
  const int s = blockIdx.x, t = threadIdx.x;
  const int base = offsets[s], n = offsets[s + 1] - base;
  int32_t* inf = info + (int64_t)s * BOOT_INFO;
  const int32_t sg = streams ? streams[s] : s;
  if (n < 1 || n > max_set || sg < 0 || sg >= (1 << 24)) {
    if (t < BOOT_INFO) inf[t] = 0;
    return;
  }
  int npad = 2;
  while (npad < n) npad <<= 1;
  for (int i = t; i < npad; i += MT) arr[i] = (i < n && labels[base + i] != 0) ? 1 : 0;
  __syncthreads();
  block_scan(arr, npad, part);
  const int npos = arr[n - 1], nneg = n - npos;
  int nan = 0;
  for (int i = t; i < npad; i += MT) {
    uint64_t k = ~0ull;
    if (i < n) {
      const float v = scores[base + i];
      nan |= (v != v);
      const int c = arr[i], before = (i > 0) ? arr[i - 1] : 0;
      const uint32_t pos = (uint32_t)(c - before);
      const uint32_t ord = pos ? (uint32_t)(c - 1) : (uint32_t)(i - c);
      k = ((uint64_t)asc_key(v) << 32) | (uint64_t)(ord << 1) | (uint64_t)pos;
    }
    key[i] = k;
  }
  const int bad = __syncthreads_or(nan);
  if (bad || npos < 1 || nneg < 1) {
    if (t < BOOT_INFO) inf[t] = 0;
    return;
  }
  sort_keys(key, npad);
  for (int i = t; i < npad; i += MT)
    arr[i] = (i > 0 && i < n && (uint32_t)(key[i] >> 32) != (uint32_t)(key[i - 1] >> 32)) ? 1 : 0;
  __syncthreads();
  block_scan(arr, npad, part);                     // arr[j]: the value group of sorted position j
  const int G = arr[n - 1] + 1;
  __syncthreads();
  uint16_t* gs = grp + (int64_t)s * max_set;
  for (int j = t; j < n; j += MT) {
    const uint32_t low = (uint32_t)key[j], pos = low & 1u, ord = (low >> 1) & 0x1FFFu;
    gs[pos ? ord : (uint32_t)npos + ord] = (uint16_t)arr[j];
    arr[j] = (arr[j] << 1) | (int32_t)pos;
  }
  __syncthreads();                                 // the keys are used up: their place takes the histogram
  int32_t* hist = reinterpret_cast<int32_t*>(key); // [G + 1] <= n + 1 <= 2 npad
  for (int g = t; g <= G; g += MT) hist[g] = 0;
  __syncthreads();
  for (int j = t; j < n; j += MT)
    if (!(arr[j] & 1)) atomicAdd(&hist[(arr[j] >> 1) + 1], 1);
  __syncthreads();
  block_scan(hist, G + 1, part);                   // hist[g + 1] = C[g], hist[0] = C[-1] = 0
  long long a2 = 0;
  for (int j = t; j < n; j += MT)
    if (arr[j] & 1) { const int g = arr[j] >> 1; a2 += hist[g] + hist[g + 1]; }
  red[t] = a2;
  __syncthreads();
  if (t == 0) {
    long long A2 = 0;
    for (int q = 0; q < MT; ++q) A2 += red[q];
    inf[0] = n; inf[1] = npos; inf[2] = nneg; inf[3] = G; inf[4] = (int32_t)A2; inf[5] = 1; inf[6] = sg; inf[7] = 0;
  }
}

__global__ __launch_bounds__(MT) void boot_resample_kernel(const int32_t* __restrict__ info, const uint16_t* __restrict__ grp,
                                                           int max_set, int grp_lds, int hpitch, int n_boot, int chunks,
                                                           uint64_t seed, int32_t* __restrict__ boot) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  const int s = blockIdx.x / chunks, chunk = blockIdx.x - s * chunks;
  const int32_t* inf = info + (int64_t)s * BOOT_INFO;
  const int b0 = chunk * BOOT_CHUNK;               // the chunk's first resample, 0-based
  const int nb = min(BOOT_CHUNK, n_boot - b0);
  int32_t* bo = boot + (int64_t)s * n_boot + b0;
  if (!inf[5]) {
    if (t < nb) bo[t] = -1;
    return;
  }
  const int n = inf[0], npos = inf[1], nneg = inf[2], G = inf[3];
  uint16_t* gl = reinterpret_cast<uint16_t*>(smem);                              // [n]: positives' groups, then negatives'
  int32_t* hist = reinterpret_cast<int32_t*>(smem + grp_lds) + w * hpitch;       // this wave's [G + 1]
  const uint16_t* gs = grp + (int64_t)s * max_set;
  for (int i = t; i < n; i += MT) gl[i] = gs[i];
  const uint64_t fixed = seed ^ 0xB0075712A9ull ^ ((uint64_t)(uint32_t)inf[6] << 40);
  for (int r = 0; r < BOOT_CHUNK / BOOT_WAVES; ++r) {
    const int q = r * BOOT_WAVES + w;              // this wave's resample within the chunk
    const bool live = q < nb;
    const uint64_t hb = fixed ^ ((uint64_t)(b0 + q + 1) << 16);
    for (int g = lane; g <= G; g += 64) hist[g] = 0;
    __syncthreads();                               // (in the first round also: the groups are in place)
    if (live) {
      for (int u = lane; u < nneg; u += 64) {
        const uint32_t hi = (uint32_t)(sig_splitmix64(hb ^ (uint64_t)(npos + u)) >> 32);
        atomicAdd(&hist[(int)gl[npos + (int)__umulhi(hi, (uint32_t)nneg)] + 1], 1);
      }
    }
    __syncthreads();
    int carry = 0;                                 // inclusive prefix sums of hist[1..G], 64 bins at a time
    for (int g0 = 1; g0 <= G; g0 += 64) {
      const int g = g0 + lane;
      int v = (g <= G) ? hist[g] : 0;
#pragma unroll
      for (int off = 1; off < 64; off <<= 1) {
        const int o = __shfl_up(v, off, 64);
        if (lane >= off) v += o;
      }
      v += carry;
      if (g <= G) hist[g] = v;
      carry = __shfl(v, 63, 64);
    }
    __syncthreads();
    int acc = 0;
    if (live) {
      for (int u = lane; u < npos; u += 64) {
        const uint32_t hi = (uint32_t)(sig_splitmix64(hb ^ (uint64_t)u) >> 32);
        const int g = gl[__umulhi(hi, (uint32_t)npos)];
        acc += hist[g] + hist[g + 1];
      }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off, 64);
    if (live && lane == 0) bo[q] = acc;
    __syncthreads();                               // every gather is done before the next round clears the histogram
  }
}

__global__ __launch_bounds__(MT) void boot_close_kernel(const int32_t* __restrict__ info, const int32_t* __restrict__ boot,
                                                        const int32_t* __restrict__ labels, const int32_t* __restrict__ offsets,
                                                        const int32_t* __restrict__ pairs, int n_sets, int n_boot,
                                                        int lo_index, int hi_index, double* __restrict__ out,
                                                        double* __restrict__ pairs_out) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  uint32_t* key = reinterpret_cast<uint32_t*>(smem);            // [n_boot]: d ^ 0x80000000 (unsigned order = d's order)
  __shared__ long long rsum[MT];
  __shared__ unsigned long long rsq[MT];
  __shared__ int32_t rle[MT], rge[MT], bins[MT];
  const int t = threadIdx.x;
  const bool is_pair = (int)blockIdx.x >= n_sets;
  const double qnan = __longlong_as_double(0x7FF8000000000000ll);
  int a = blockIdx.x, c = -1;
  double* o = out + (int64_t)a * NM_METRICS_STRIDE;
  bool ok;
  if (!is_pair) {
    ok = info[(int64_t)a * BOOT_INFO + 5] != 0;
  } else {
    const int p = (int)blockIdx.x - n_sets;
    a = pairs[2 * (int64_t)p]; c = pairs[2 * (int64_t)p + 1];
    o = pairs_out + (int64_t)p * NM_METRICS_STRIDE;
    ok = a >= 0 && a < n_sets && c >= 0 && c < n_sets;
    if (ok) {
      const int32_t* ia = info + (int64_t)a * BOOT_INFO;
      const int32_t* ic = info + (int64_t)c * BOOT_INFO;
      ok = ia[5] && ic[5] && ia[6] == ic[6] && ia[0] == ic[0];
    }
    if (ok) {                                      // (the same for every thread so far) the labels, row by row
      const int n = info[(int64_t)a * BOOT_INFO];
      const int32_t* la = labels + offsets[a];
      const int32_t* lc = labels + offsets[c];
      int diff = 0;
      for (int i = t; i < n; i += MT) diff |= ((la[i] != 0) != (lc[i] != 0)) ? 1 : 0;
      ok = !__syncthreads_or(diff);
    }
  }
  if (!ok) {
    if (t < NM_METRICS_STRIDE) o[t] = qnan;
    return;
  }
  const int32_t* ia = info + (int64_t)a * BOOT_INFO;
  const int32_t* va = boot + (int64_t)a * n_boot;
  const int32_t* vc = is_pair ? boot + (int64_t)c * n_boot : nullptr;
  long long sum = 0;
  int le = 0, ge = 0;
  for (int i = t; i < n_boot; i += MT) {
    const int d = va[i] - (vc ? vc[i] : 0);
    sum += d; le += (d <= 0) ? 1 : 0; ge += (d >= 0) ? 1 : 0;
    key[i] = (uint32_t)d ^ 0x80000000u;
  }
  rsum[t] = sum; rle[t] = le; rge[t] = ge;
  __syncthreads();
  long long total = 0;
  for (int q = 0; q < MT; ++q) total += rsum[q];
  const long long m = total / n_boot;              // an integer near the mean: |d - m| <= 2^26
  unsigned long long sq = 0;                       // at most 64 squares below 2^52 each
  for (int i = t; i < n_boot; i += MT) {
    const long long e = (long long)(int32_t)(key[i] ^ 0x80000000u) - m;
    sq += (unsigned long long)(e * e);
  }
  rsq[t] = sq;
  __syncthreads();
  // the two order statistics by radix selection, a byte of the key per pass from the top: the histogram of that byte over
  // the keys that share the bytes chosen so far (LDS integer atomics), then every thread walks the 256 bins alike
  uint32_t stat_lo = 0, stat_hi = 0;
  for (int which = 0; which < 2; ++which) {
    int rank = which ? hi_index : lo_index;        // 0-based, among the keys that still match
    uint32_t prefix = 0, mask = 0;
    for (int shift = 24; shift >= 0; shift -= 8) {
      bins[t] = 0;
      __syncthreads();
      for (int i = t; i < n_boot; i += MT) {
        const uint32_t k = key[i];
        if ((k & mask) == prefix) atomicAdd(&bins[(k >> shift) & 0xFFu], 1);
      }
      __syncthreads();
      int b = 0, below = 0;
      for (; b < 255; ++b) {
        const int c = bins[b];
        if (below + c > rank) break;
        below += c;
      }
      rank -= below;
      prefix |= (uint32_t)b << shift;
      mask |= 0xFFu << shift;
      __syncthreads();                             // everyone has read the bins before the next pass clears them
    }
    if (which) stat_hi = prefix; else stat_lo = prefix;
  }
  if (t == 0) {
    int LE = 0, GE = 0;
    unsigned long long qlo = 0, qhi = 0;           // sum (d - m)^2 in 128 bits
    for (int q = 0; q < MT; ++q) {
      LE += rle[q]; GE += rge[q];
      const unsigned long long before = qlo;
      qlo += rsq[q];
      qhi += (qlo < before) ? 1ull : 0ull;
    }
    // T = n_boot * sum (d - m)^2 - r^2, r = sum d - n_boot m (|r| < n_boot): never negative, below 2^81
    const unsigned long long nb = (unsigned long long)n_boot;
    unsigned long long tlo = qlo * nb, thi = __umul64hi(qlo, nb) + qhi * nb;
    const long long r = total - m * (long long)n_boot;
    const unsigned long long r2 = (unsigned long long)(r * r);
    thi -= (tlo < r2) ? 1ull : 0ull;
    tlo -= r2;
    const double T = (double)thi * 18446744073709551616.0 + (double)tlo;
    const double den = (double)(2ll * ia[1] * ia[2]);
    const double lo = (double)(int32_t)(stat_lo ^ 0x80000000u) / den;
    const double hi = (double)(int32_t)(stat_hi ^ 0x80000000u) / den;
    const double mean = (double)total / (double)(2ll * ia[1] * ia[2] * (long long)n_boot);
    const double se = n_boot > 1 ? __dsqrt_rn(T / (double)((long long)n_boot * (n_boot - 1))) / den : qnan;
    o[1] = lo; o[2] = hi; o[3] = mean; o[4] = se;
    if (!is_pair) {
      o[0] = (double)ia[4] / den;
      o[5] = (double)n_boot; o[6] = (double)ia[1]; o[7] = (double)ia[2];
    } else {
      o[0] = (double)(ia[4] - info[(int64_t)c * BOOT_INFO + 4]) / den;
      o[5] = fmin(1.0, (double)(2ll * (1 + min(LE, GE))) / (double)(1 + n_boot));
      o[6] = (double)LE; o[7] = (double)GE;
    }
  }
}

// ---- one regression per column (latent_pvalues, utils_vae.py:163-174, for every column of a table at once) -------------
// nm_column_regress: one workgroup per (set, 64-column tile), a lane per column, as roi_effect_kernel; the four waves take
// every fourth row, and the target, covariates and include word of a row are wave-uniform loads.  Every pass over the rows
// ends with the waves' partial sums merged through LDS in wave order, and every wave then does the same P x P algebra on the
// same sums, so all four hold the same parameters for the next pass without a broadcast.  Pass 0 gives n, the means and the
// validity of the column; OLS takes two more (normal equations of the centred design, residuals), Logit one per Newton step
// and one for the Hessian at the final parameters.  The tile is re-read from L2 in every pass.  A lane that has finished
// keeps its state; the workgroup leaves the Newton loop when no lane is still iterating.  Templated on q and the kind: every
// index into the register arrays is a compile-time constant after unrolling.

// Continued fraction of the incomplete beta function (modified Lentz), converging fast for x < (a + 1) / (a + b + 2).
__host__ __device__ inline double reg_betacf(double a, double b, double x) {
  const double tiny = 1e-300, eps = 1e-15;
  const double qab = a + b, qap = a + 1.0, qam = a - 1.0;
  double c = 1.0, d = 1.0 - qab * x / qap;
  if (fabs(d) < tiny) d = tiny;
  d = 1.0 / d;
  double h = d;
  for (int m = 1; m <= 4000; ++m) {
    const double m2 = 2.0 * m;
    double aa = m * (b - m) * x / ((qam + m2) * (a + m2));
    d = 1.0 + aa * d; if (fabs(d) < tiny) d = tiny;
    c = 1.0 + aa / c; if (fabs(c) < tiny) c = tiny;
    d = 1.0 / d;
    h *= d * c;
    aa = -(a + m) * (qab + m) * x / ((a + m2) * (qap + m2));
    d = 1.0 + aa * d; if (fabs(d) < tiny) d = tiny;
    c = 1.0 + aa / c; if (fabs(c) < tiny) c = tiny;
    d = 1.0 / d;
    const double del = d * c;
    h *= del;
    if (fabs(del - 1.0) < eps) break;
  }
  return h;
}

// P(|T_df| >= |t|) = I_x(df / 2, 1 / 2) at x = df / (df + t^2); log x and log (1 - x) from t^2 / df, so neither tail cancels.
__host__ __device__ inline double reg_student_t_two_sided(double t, double df) {
  if (t != t || !(df > 0.0)) return NAN;
  const double r = t * t / df;
  if (r == 0.0) return 1.0;
  if (r > 1.7e308) return 0.0;
  const double a = 0.5 * df, b = 0.5;
  const double l1p = log1p(r);
  const double x = 1.0 / (1.0 + r), omx = r / (1.0 + r);
  const double front = exp(lgamma(a + b) - lgamma(a) - lgamma(b) - a * l1p + b * (log(r) - l1p));
  if (x < (a + 1.0) / (a + b + 2.0)) return front * reg_betacf(a, b, x) / a;
  return 1.0 - front * reg_betacf(b, a, omx) / b;
}

constexpr int REG_TILE = 64;                       // columns per workgroup
constexpr int REG_WAVES = MT / 64;
constexpr double REG_PIVOT = 1e-12;                // a Cholesky pivot at or below this share of its diagonal entry: not positive definite
static_assert(sizeof(nm_reg_set_t) == 48, "nm_reg_set_t is mirrored by _lib.NmRegSet");

// A = L L' (A's upper triangle is read, L's lower written); false where a pivot fails
template <int P>
__device__ __forceinline__ bool reg_chol(const double (&A)[P][P], double (&L)[P][P]) {
  bool ok = true;
#pragma unroll
  for (int j = 0; j < P; ++j) {
    double d = A[j][j];
#pragma unroll
    for (int k = 0; k < j; ++k) d -= L[j][k] * L[j][k];
    ok = ok && (d > REG_PIVOT * A[j][j]);
    const double l = sqrt(d);
    L[j][j] = l;
#pragma unroll
    for (int i = j + 1; i < P; ++i) {
      double v = A[j][i];
#pragma unroll
      for (int k = 0; k < j; ++k) v -= L[i][k] * L[j][k];
      L[i][j] = v / l;
    }
  }
  return ok;
}
template <int P>
__device__ __forceinline__ void reg_forward(const double (&L)[P][P], double (&y)[P]) {      // y := L^-1 y
#pragma unroll
  for (int i = 0; i < P; ++i) {
    double v = y[i];
#pragma unroll
    for (int k = 0; k < i; ++k) v -= L[i][k] * y[k];
    y[i] = v / L[i][i];
  }
}
template <int P>
__device__ __forceinline__ void reg_backward(const double (&L)[P][P], double (&y)[P]) {     // y := L'^-1 y
#pragma unroll
  for (int i = P - 1; i >= 0; --i) {
    double v = y[i];
#pragma unroll
    for (int k = i + 1; k < P; ++k) v -= L[k][i] * y[k];
    y[i] = v / L[i][i];
  }
}

// v[k] := the four waves' v[k] added in wave order (all threads call; every wave gets the same sums)
template <int N>
__device__ __forceinline__ void reg_merge(double (&v)[N], double* part, int w, int lane) {
#pragma unroll
  for (int k = 0; k < N; ++k) part[(w * N + k) * REG_TILE + lane] = v[k];
  __syncthreads();
#pragma unroll
  for (int k = 0; k < N; ++k) {
    double s = part[k * REG_TILE + lane];
#pragma unroll
    for (int q = 1; q < REG_WAVES; ++q) s += part[(q * N + k) * REG_TILE + lane];
    v[k] = s;
  }
  __syncthreads();
}

// One pass over the set's included rows at the parameters beta of the centred design z = (1, x - m1, cov - m2..).
// MODE 0: A = Z'Z, g = Z'y.   MODE 1: p = 1 / (1 + exp(-z.beta)), A = Z' diag(p (1 - p)) Z, g = Z'(y - p).
// MODE 2: rss = sum (y - z.beta)^2, A and g untouched.
template <int Q, int MODE>
__device__ __forceinline__ void reg_pass(const nm_reg_set_t& S, const float* xc, bool cv, int w, int lane, const double (&m)[2 + Q],
                                         const double (&beta)[2 + Q], double (&A)[2 + Q][2 + Q], double (&g)[2 + Q], double& rss,
                                         double* part) {
  constexpr int P = 2 + Q, NT = P * (P + 1) / 2;
  double acc[MODE == 2 ? 1 : NT + P];
#pragma unroll
  for (int k = 0; k < (MODE == 2 ? 1 : NT + P); ++k) acc[k] = 0.0;
  for (int r = w; r < S.rows; r += REG_WAVES) {
    if (S.include && S.include[r] == 0) continue;
    double z[P];
    z[0] = 1.0;
    z[1] = (cv ? (double)xc[(int64_t)r * S.pitch] : 0.0) - m[1];
#pragma unroll
    for (int k = 0; k < Q; ++k) z[2 + k] = (double)S.cov[(int64_t)r * S.cov_pitch + k] - m[2 + k];
    const double y = (double)S.target[r];
    double eta = beta[0];
#pragma unroll
    for (int i = 1; i < P; ++i) eta += z[i] * beta[i];
    if (MODE == 2) {
      const double e = y - eta;
      acc[0] += e * e;
    } else {
      double wt = 1.0, res = y;
      if (MODE == 1) {
        const double p = 1.0 / (1.0 + exp(-eta));
        wt = p * (1.0 - p);
        res = y - p;
      }
      int k = 0;
#pragma unroll
      for (int i = 0; i < P; ++i) {
        const double wz = MODE == 1 ? wt * z[i] : z[i];
#pragma unroll
        for (int j = i; j < P; ++j) acc[k++] += wz * z[j];
      }
#pragma unroll
      for (int i = 0; i < P; ++i) acc[NT + i] += z[i] * res;
    }
  }
  reg_merge(acc, part, w, lane);
  if (MODE == 2) {
    rss = acc[0];
  } else {
    int k = 0;
#pragma unroll
    for (int i = 0; i < P; ++i) {
#pragma unroll
      for (int j = i; j < P; ++j) A[i][j] = acc[k++];
    }
#pragma unroll
    for (int i = 0; i < P; ++i) g[i] = acc[NT + i];
  }
}

template <int Q, int KIND>
__global__ __launch_bounds__(MT) void column_regress_kernel(const nm_reg_set_t* __restrict__ sets, int D, int max_rows, int tiles,
                                                            double* __restrict__ out) {
  constexpr int P = 2 + Q;
  constexpr int NT = P * (P + 1) / 2;
  constexpr int N0 = P + 5;                        // pass 0: sums of target, column, covariates; n, ones, bad; min, max
  constexpr int NL = (NT + P) > N0 ? (NT + P) : N0;
  __shared__ double part[REG_WAVES * NL * REG_TILE];

  const int t = threadIdx.x, lane = t & 63, w = __builtin_amdgcn_readfirstlane(t >> 6);
  const int s = blockIdx.x / tiles, tile = blockIdx.x - s * tiles;
  const nm_reg_set_t S = sets[s];
  const int col = tile * REG_TILE + lane;
  const bool cv = col < D;
  double* o = out + ((int64_t)s * D + col) * NM_METRICS_STRIDE;
  const double qnan = __longlong_as_double(0x7FF8000000000000ll);
  const int rows = S.rows;
  if (rows < 0 || rows > max_rows || S.pitch < D || (Q > 0 && S.cov_pitch < Q) ||
      (rows > 0 && (!S.x || !S.target || (Q > 0 && !S.cov)))) {
    if (w == 0 && cv) {
      for (int k = 0; k < 6; ++k) o[k] = qnan;
      o[6] = 0.0; o[7] = -2.0;
    }
    return;
  }
  const float* xc = S.x + col;                     // (read only where cv: beyond D lies padding, or the next row)

  // pass 0: the included rows, the sums the means come from, what makes the column or the set invalid
  double a0[N0];
#pragma unroll
  for (int k = 0; k < N0; ++k) a0[k] = 0.0;
  double xmin = __longlong_as_double(0x7FF0000000000000ll), xmax = -xmin;
  for (int r = w; r < rows; r += REG_WAVES) {
    if (S.include && S.include[r] == 0) continue;
    const float yf = S.target[r];
    const float xf = cv ? xc[(int64_t)r * S.pitch] : 0.f;
    bool bad = !isfinite(yf) || !isfinite(xf);
    if (KIND == NM_REG_LOGIT) bad = bad || (yf != 0.f && yf != 1.f);
    a0[0] += (double)yf;
    a0[1] += (double)xf;
#pragma unroll
    for (int k = 0; k < Q; ++k) {
      const float cf = S.cov[(int64_t)r * S.cov_pitch + k];
      bad = bad || !isfinite(cf);
      a0[2 + k] += (double)cf;
    }
    a0[P] += 1.0;
    a0[P + 1] += (yf == 1.f) ? 1.0 : 0.0;
    a0[P + 2] += bad ? 1.0 : 0.0;
    xmin = fmin(xmin, (double)xf);
    xmax = fmax(xmax, (double)xf);
  }
  a0[P + 3] = xmin; a0[P + 4] = xmax;
#pragma unroll
  for (int k = 0; k < N0; ++k) part[(w * N0 + k) * REG_TILE + lane] = a0[k];
  __syncthreads();
#pragma unroll
  for (int k = 0; k < N0; ++k) {
    double v = part[k * REG_TILE + lane];
#pragma unroll
    for (int q = 1; q < REG_WAVES; ++q) {
      const double u = part[(q * N0 + k) * REG_TILE + lane];
      v = k == P + 3 ? fmin(v, u) : k == P + 4 ? fmax(v, u) : v + u;
    }
    a0[k] = v;
  }
  __syncthreads();
  const double n = a0[P];
  bool valid = cv && a0[P + 2] == 0.0 && n > (double)P && a0[P + 3] < a0[P + 4];
  if (KIND == NM_REG_LOGIT) valid = valid && a0[P + 1] > 0.0 && a0[P + 1] < n;
  double m[P];
  m[0] = 0.0;
#pragma unroll
  for (int i = 1; i < P; ++i) m[i] = a0[i] / n;

  double beta[P], A[P][P], g[P], L[P][P], rss = 0.0;
#pragma unroll
  for (int i = 0; i < P; ++i) beta[i] = 0.0;
  int n_iter = 0;
  int state = valid ? 0 : 4;                       // 0 iterating, 1 converged: the Hessian at the end is due, 2 done, 3 failed (-1), 4 invalid (-2)
  if (KIND == NM_REG_OLS) {
    reg_pass<Q, 0>(S, xc, cv, w, lane, m, beta, A, g, rss, part);
    if (state == 0) {
      if (reg_chol<P>(A, L)) {
#pragma unroll
        for (int i = 0; i < P; ++i) beta[i] = g[i];
        reg_forward<P>(L, beta);
        reg_backward<P>(L, beta);
        state = 2;
      } else {
        state = 4;
      }
    }
    reg_pass<Q, 2>(S, xc, cv, w, lane, m, beta, A, g, rss, part);
  } else {
    while (__syncthreads_or(state <= 1)) {
      reg_pass<Q, 1>(S, xc, cv, w, lane, m, beta, A, g, rss, part);
      if (state > 1) continue;
      const bool pd = reg_chol<P>(A, L);
      if (!pd) {
        state = n_iter == 0 ? 4 : 3;               // at zero the Hessian is a quarter of the Gram matrix: a singular design
      } else if (state == 1) {
        state = 2;
      } else {
        reg_forward<P>(L, g);
        reg_backward<P>(L, g);
        double big = 0.0;
#pragma unroll
        for (int i = 0; i < P; ++i) { beta[i] += g[i]; big = fmax(big, fabs(g[i])); }
        ++n_iter;
        state = big <= NM_REG_TOL ? 1 : (n_iter >= NM_REG_MAX_ITER || big != big) ? 3 : 0;
      }
    }
  }
  if (w != 0 || !cv) return;
  o[6] = n;
  if (state != 2) {
    for (int k = 0; k < 6; ++k) o[k] = qnan;
    o[7] = state == 3 ? -1.0 : -2.0;
    return;
  }
  // var(coef) = |L^-1 e1|^2 and var(const) = |L^-1 (1, -m)|^2 (times s^2 for OLS)
  double u[P], v[P];
  u[0] = 0.0; u[1] = 1.0; v[0] = 1.0; v[1] = -m[1];
#pragma unroll
  for (int i = 2; i < P; ++i) { u[i] = 0.0; v[i] = -m[i]; }
  reg_forward<P>(L, u);
  reg_forward<P>(L, v);
  double vu = 0.0, vv = 0.0, b0 = beta[0];
#pragma unroll
  for (int i = 0; i < P; ++i) { vu += u[i] * u[i]; vv += v[i] * v[i]; }
#pragma unroll
  for (int i = 1; i < P; ++i) b0 -= m[i] * beta[i];
  const double df = n - (double)P;
  const double s2 = KIND == NM_REG_OLS ? rss / df : 1.0;
  const double se0 = sqrt(s2 * vv), se1 = sqrt(s2 * vu);
  o[0] = b0; o[1] = beta[1]; o[2] = se0; o[3] = se1;
  if (KIND == NM_REG_OLS) {
    o[4] = reg_student_t_two_sided(b0 / se0, df);
    o[5] = reg_student_t_two_sided(beta[1] / se1, df);
  } else {
    o[4] = erfc(fabs(b0 / se0) * 0.70710678118654752440);
    o[5] = erfc(fabs(beta[1] / se1) * 0.70710678118654752440);
  }
  o[7] = (double)n_iter;
}

template <int KIND>
int launch_column_regress(int n_cov, dim3 grid, void* stream, const nm_reg_set_t* sets, int D, int max_rows, int tiles, double* out) {
  switch (n_cov) {
    case 0: return launch_kernel(column_regress_kernel<0, KIND>, grid, dim3(MT), 0, stream, sets, D, max_rows, tiles, out);
    case 1: return launch_kernel(column_regress_kernel<1, KIND>, grid, dim3(MT), 0, stream, sets, D, max_rows, tiles, out);
    case 2: return launch_kernel(column_regress_kernel<2, KIND>, grid, dim3(MT), 0, stream, sets, D, max_rows, tiles, out);
    case 3: return launch_kernel(column_regress_kernel<3, KIND>, grid, dim3(MT), 0, stream, sets, D, max_rows, tiles, out);
    default: return launch_kernel(column_regress_kernel<4, KIND>, grid, dim3(MT), 0, stream, sets, D, max_rows, tiles, out);
  }
}

}  // namespace

extern "C" {

int nm_column_regress(const nm_reg_set_t* sets_dev, int n_sets, int D, int max_rows, int n_cov, int kind, double* out,
                      void* stream) {
  if (!sets_dev || !out) return NM_E_NULL;
  if (n_sets < 1 || D < 1 || max_rows < 1 || max_rows > MAXN || n_cov < 0 || n_cov > NM_REG_MAX_COV ||
      (kind != NM_REG_OLS && kind != NM_REG_LOGIT))
    return NM_E_METRICS;
  const int tiles = (D + REG_TILE - 1) / REG_TILE;
  if ((int64_t)n_sets * tiles > 0x7FFFFFFFll) return NM_E_METRICS;
  const dim3 grid(n_sets * tiles);
  return kind == NM_REG_OLS ? launch_column_regress<NM_REG_OLS>(n_cov, grid, stream, sets_dev, D, max_rows, tiles, out)
                            : launch_column_regress<NM_REG_LOGIT>(n_cov, grid, stream, sets_dev, D, max_rows, tiles, out);
}

double nm_student_t_two_sided(double t, double df) { return reg_student_t_two_sided(t, df); }


int nm_posthoc_metrics(const float* scores, const int32_t* labels, const int32_t* offsets, int n_sets, int max_set,
                       const double* thr_in, double* out, void* stream) {
  if (!scores || !labels || !offsets || !out) return NM_E_NULL;
  if (n_sets < 1 || max_set < 1 || max_set > MAXN) return NM_E_METRICS;
  return launch_kernel(posthoc_kernel, dim3(n_sets), dim3(MT), METRICS_SMEM, stream, scores, labels, offsets, thr_in, out);
}

int nm_confusion_metrics(const int32_t* pred, const int32_t* labels, const int32_t* offsets, int n_sets, double* out,
                         void* stream) {
  if (!pred || !labels || !offsets || !out) return NM_E_NULL;
  if (n_sets < 1) return NM_E_METRICS;
  return launch_kernel(confusion_kernel, dim3(n_sets), dim3(MT), 0, stream, pred, labels, offsets, out);
}

int nm_latent_stats(const float* mu, const int32_t* offsets, int n_sets, int Z, int pitch, float* mean_out, float* var_out,
                    void* stream) {
  if (!mu || !offsets || !mean_out || !var_out) return NM_E_NULL;
  if (Z < 1 || Z > NM_MAX_LATENT) return NM_E_LATENT;
  if (n_sets < 1 || pitch < Z) return NM_E_METRICS;
  return launch_kernel(latent_stats_kernel, dim3(n_sets), dim3(MT), 0, stream, mu, offsets, Z, pitch, mean_out, var_out);
}

int nm_latent_score(const float* mu, const float* logvar, const int32_t* offsets, int n_sets, int Z, int pitch, const float* mean,
                    const float* var, float* zsep_out, float* score_out, void* stream) {
  if (!mu || !logvar || !offsets || !mean || !var || (!zsep_out && !score_out)) return NM_E_NULL;
  if (Z < 1 || Z > NM_MAX_LATENT) return NM_E_LATENT;
  if (n_sets < 1 || pitch < Z) return NM_E_METRICS;
  return launch_kernel(latent_score_kernel, dim3(n_sets), dim3(MT), 0, stream, mu, logvar, offsets, Z, pitch, mean, var, zsep_out,
                       score_out);
}

int nm_roi_effect(const nm_roi_set_t* sets_dev, int n_sets, int D, int max_rows, double* out, void* stream) {
  if (!sets_dev || !out) return NM_E_NULL;
  if (n_sets < 1 || D < 1 || max_rows < 1 || max_rows > MAXN) return NM_E_METRICS;
  const int tiles = (D + ROI_TILE - 1) / ROI_TILE;
  if ((int64_t)n_sets * tiles > 0x7FFFFFFFll) return NM_E_METRICS;
  return launch_kernel(roi_effect_kernel, dim3(n_sets * tiles), dim3(MT), 0, stream, sets_dev, D, max_rows, tiles, out);
}

size_t nm_roi_significance_workspace(int n_sets, int D, int max_rows, int n_perm) {
  if (n_sets < 1 || D < 1 || max_rows < 1 || n_perm < 0) return 0;
  return sig_plan(n_sets, D, max_rows, n_perm).total;
}

int nm_roi_significance(const nm_roi_set_t* sets_dev, int n_sets, int D, int max_rows, int n_perm, uint64_t seed,
                        void* workspace, size_t workspace_bytes, double* out, int32_t* maxstat_out, void* stream) {
  if (!sets_dev || !out || !workspace) return NM_E_NULL;
  if (n_sets < 1 || D < 1 || D > SIG_MAX_D || max_rows < 1 || max_rows > MAXN || n_perm < 0 || n_perm > NM_ROI_MAX_PERM)
    return NM_E_METRICS;
  const SigPlan P = sig_plan(n_sets, D, max_rows, n_perm);
  if (workspace_bytes < P.total) return NM_E_METRICS;
  const int pblocks = (n_perm + MT - 1) / MT, dblocks = (D + MT - 1) / MT;
  if ((int64_t)n_sets * D > 0x7FFFFFFFll || (int64_t)n_sets * n_perm > 0x7FFFFFFFll ||
      (int64_t)n_sets * P.tiles * P.chunks > 0x7FFFFFFFll)
    return NM_E_METRICS;
  char* ws = static_cast<char*>(workspace);
  uint16_t* r2 = reinterpret_cast<uint16_t*>(ws + P.r2);
  int32_t* colS = reinterpret_cast<int32_t*>(ws + P.colS);
  double* coltie = reinterpret_cast<double*>(ws + P.coltie);
  int32_t* info = reinterpret_cast<int32_t*>(ws + P.info);
  uint32_t* lab = reinterpret_cast<uint32_t*>(ws + P.lab);
  int32_t* tmax = reinterpret_cast<int32_t*>(ws + P.tmax);
  int32_t* ccnt = reinterpret_cast<int32_t*>(ws + P.ccnt);
  int32_t* ms = reinterpret_cast<int32_t*>(ws + P.ms);
  int32_t* cnt = reinterpret_cast<int32_t*>(ws + P.cnt);
  const int sort_lds = pow2_at_least(max_rows) * 8;
  int e = launch_kernel(roi_rank_kernel, dim3(n_sets * D), dim3(MT), sort_lds, stream, sets_dev, D, max_rows, r2, colS, coltie, info);
  if (e) return e;
  if (n_perm > 0) {
    e = launch_kernel(roi_label_kernel, dim3(n_sets * n_perm), dim3(MT), sort_lds, stream, (const int32_t*)info, n_perm, P.W, seed, lab);
    if (e) return e;
    e = launch_kernel(roi_sum_kernel, dim3(n_sets * P.tiles * P.chunks), dim3(MT), 0, stream, (const int32_t*)info,
                      (const uint16_t*)r2, (const int32_t*)colS, (const double*)coltie, (const uint32_t*)lab, D, max_rows, n_perm,
                      P.W, P.tiles, P.chunks, tmax, ccnt);
    if (e) return e;
    e = launch_kernel(roi_max_kernel, dim3(n_sets * pblocks), dim3(MT), 0, stream, (const int32_t*)info, (const int32_t*)tmax,
                      n_perm, P.tiles, pblocks, ms, maxstat_out);
    if (e) return e;
  }
  e = launch_kernel(roi_count_kernel, dim3(n_sets * dblocks), dim3(MT), 0, stream, (const int32_t*)info, (const int32_t*)colS,
                    (const int32_t*)ccnt, (const int32_t*)ms, D, n_perm, P.chunks, dblocks, cnt);
  if (e) return e;
  const int npad = pow2_at_least(D);
  return launch_kernel(roi_close_kernel, dim3(n_sets), dim3(MT), npad * (8 + 2), stream, (const int32_t*)info, (const int32_t*)colS,
                       (const double*)coltie, (const int32_t*)cnt, D, npad, n_perm, out);
}

size_t nm_auc_bootstrap_workspace(int n_sets, int max_set, int n_boot, int n_pairs) {
  if (n_sets < 1 || max_set < 1 || max_set > MAXN || n_boot < 1 || n_boot > NM_BOOT_MAX || n_pairs < 0) return 0;
  return boot_plan(n_sets, max_set, n_boot).total;
}

int nm_auc_bootstrap(const float* scores, const int32_t* labels, const int32_t* offsets, const int32_t* streams, int n_sets,
                     int max_set, int n_boot, int lo_index, int hi_index, uint64_t seed, const int32_t* pairs, int n_pairs,
                     void* workspace, size_t workspace_bytes, double* out, double* pairs_out, int32_t* boot_out, void* stream) {
  if (!scores || !labels || !offsets || !workspace || !out) return NM_E_NULL;
  if (n_pairs > 0 && (!pairs || !pairs_out)) return NM_E_NULL;
  if (n_sets < 1 || max_set < 1 || max_set > MAXN || n_boot < 1 || n_boot > NM_BOOT_MAX || n_pairs < 0) return NM_E_METRICS;
  if (lo_index < 0 || lo_index > hi_index || hi_index >= n_boot) return NM_E_METRICS;
  const BootPlan P = boot_plan(n_sets, max_set, n_boot);
  if (workspace_bytes < P.total) return NM_E_METRICS;
  if ((int64_t)n_sets * P.chunks > 0x7FFFFFFFll || (int64_t)n_sets + n_pairs > 0x7FFFFFFFll) return NM_E_METRICS;
  char* ws = static_cast<char*>(workspace);
  int32_t* info = reinterpret_cast<int32_t*>(ws + P.info);
  uint16_t* grp = reinterpret_cast<uint16_t*>(ws + P.grp);
  int32_t* boot = boot_out ? boot_out : reinterpret_cast<int32_t*>(ws + P.boot);
  const int npad_set = pow2_at_least(max_set);
  int e = launch_kernel(boot_prepare_kernel, dim3(n_sets), dim3(MT), npad_set * (8 + 4), stream, scores, labels, offsets, streams,
                        max_set, npad_set, grp, info);
  if (e) return e;
  e = launch_kernel(boot_resample_kernel, dim3(n_sets * P.chunks), dim3(MT), P.resample_lds, stream, (const int32_t*)info,
                    (const uint16_t*)grp, max_set, P.grp_lds, P.hpitch, n_boot, P.chunks, seed, boot);
  if (e) return e;
  return launch_kernel(boot_close_kernel, dim3(n_sets + n_pairs), dim3(MT), n_boot * 4, stream, (const int32_t*)info,
                       (const int32_t*)boot, labels, offsets, pairs, n_sets, n_boot, lo_index, hi_index, out, pairs_out);
}

}  // extern "C"

#include "nm_normative.inc"
#include "nm_curve.inc"
#include "nm_centile.inc"
#include "nm_fit.inc"
