// nm_curve.inc -- operating points on the device (included at the end of nm_metrics.hip; include/nmhip.h has the
// definitions): nm_operating_points, two launches on one stream over a small workspace.
//
//   select  one workgroup per score set.  build_curve (nm_metrics.hip) leaves the set in LDS exactly as posthoc_kernel
//           has it: sorted (score, label) keys, the true-positive prefix sums and the K compacted distinct-score
//           boundaries.  Every rule of the table is then one strided loop -- over the K boundaries, or over the n values
//           of its grid with a binary search into the boundaries -- whose per-thread candidate (value, order) is merged
//           once: a butterfly inside the wave, the four waves through LDS.  The merge picks by a total order (better
//           value, then lower order), so its shape does not matter.  Counts stay integers until the last divisions; the
//           fp64 expressions are the reference's, one operation at a time (contraction is off).  The set's summary row
//           and its ROC on a grid come from the same LDS.  (threshold, objective, status) per rule go to the workspace.
//   apply   one workgroup per evaluation entry: the thresholds of its selection set in registers, one pass over the
//           evaluation set's scores with the TP and FP of every rule counted in registers, one block reduction.
// No atomics, every sum in a fixed order: two runs give the same bytes, and a set's rows do not depend on its place.
#pragma clang fp contract(off)

namespace {

constexpr int OP_SEL = 4;                          // doubles per (set, rule) in the workspace: threshold, objective, status, 0
struct OpRules { nm_op_rule_t r[NM_OP_MAX_RULES]; };
static_assert(sizeof(nm_op_rule_t) == 40, "nm_op_rule_t is mirrored by _lib.NmOpRule");
static_assert(sizeof(OpRules) <= 1024, "the rule table travels as a kernel argument");

__device__ __forceinline__ double op_nan() { return __longlong_as_double(0x7FF8000000000000ll); }
__device__ __forceinline__ double op_inf() { return __longlong_as_double(0x7FF0000000000000ll); }

// (v, o) <- the better of (v, o) and (v2, o2): o < 0 is no candidate; a better value wins, equal values go to the lower order
template <bool MINIMIZE>
__device__ __forceinline__ void op_pick(double& v, int& o, double v2, int o2) {
  const bool take = o2 >= 0 && (o < 0 || (MINIMIZE ? v2 < v : v2 > v) || (v2 == v && o2 < o));
  if (take) { v = v2; o = o2; }
}
// the workgroup's best candidate, to every thread; all threads call
template <bool MINIMIZE>
__device__ __forceinline__ void op_best(double& v, int& o, double* redV, int32_t* redI) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const double v2 = __shfl_xor(v, off, 64);
    const int o2 = __shfl_xor(o, off, 64);
    op_pick<MINIMIZE>(v, o, v2, o2);
  }
  __syncthreads();                                 // whoever still reads the slots of the reduction before is done
  if ((threadIdx.x & 63) == 0) { redV[threadIdx.x >> 6] = v; redI[threadIdx.x >> 6] = o; }
  __syncthreads();
  v = redV[0]; o = redI[0];
#pragma unroll
  for (int w = 1; w < MT / 64; ++w) op_pick<MINIMIZE>(v, o, redV[w], redI[w]);
}
// sums over the workgroup in a fixed shape (a + b == b + a bit for bit: every lane of the butterfly holds the same sum)
__device__ __forceinline__ void op_sums(long long& a, long long& b, double& c, double& d, long long* redA, double* redV) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    a += __shfl_xor(a, off, 64); b += __shfl_xor(b, off, 64);
    c += __shfl_xor(c, off, 64); d += __shfl_xor(d, off, 64);
  }
  __syncthreads();
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) { redA[w] = a; redA[4 + w] = b; redV[w] = c; redV[4 + w] = d; }
  __syncthreads();
  a = redA[0] + redA[1] + redA[2] + redA[3];
  b = redA[4] + redA[5] + redA[6] + redA[7];
  c = ((redV[0] + redV[1]) + redV[2]) + redV[3];
  d = ((redV[4] + redV[5]) + redV[6]) + redV[7];
}

__global__ __launch_bounds__(MT) void op_select_kernel(const float* __restrict__ scores, const int32_t* __restrict__ labels,
                                                       const int32_t* __restrict__ offsets, const OpRules R, int n_rules,
                                                       double at_spec, double at_sens, double max_fpr, double* __restrict__ sel,
                                                       double* __restrict__ summary, double* __restrict__ grid, int G) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  uint64_t* key = reinterpret_cast<uint64_t*>(smem);            // [MAXN]
  int32_t* cum = reinterpret_cast<int32_t*>(key + MAXN);        // [MAXN]
  int32_t* bnd = cum + MAXN;                                    // [MAXN]
  __shared__ int32_t part[MT];
  __shared__ double redV[8];
  __shared__ int32_t redI[4];
  __shared__ long long redA[8];
  static_assert(MT / 64 == 4, "the reductions merge four waves");

  const int s = blockIdx.x, t = threadIdx.x;
  const int base = offsets[s], n = offsets[s + 1] - base;
  double* sl = sel + (int64_t)s * n_rules * OP_SEL;
  const bool sized = n >= 1 && n <= MAXN;
  int K = 0, P = 0, Nn = 0;
  bool ok = sized;
  if (sized) {
    int nan;
    K = build_curve(scores, labels, base, n, key, cum, bnd, part, nan);
    P = cum[n - 1]; Nn = n - P;
    ok = !__syncthreads_or(nan) && P > 0 && Nn > 0;
  }
  if (!ok) {                                       // empty, too long, one class, a NaN score: no curve
    for (int r = t; r < n_rules; r += MT) { sl[r * OP_SEL] = op_nan(); sl[r * OP_SEL + 1] = op_nan(); sl[r * OP_SEL + 2] = -2.0; sl[r * OP_SEL + 3] = 0.0; }
    if (summary && t < NM_METRICS_STRIDE)
      summary[(int64_t)s * NM_METRICS_STRIDE + t] = (sized && t >= 6) ? (double)(t == 6 ? P : Nn) : op_nan();
    if (grid)
      for (int g = t; g < G; g += MT) grid[(int64_t)s * G + g] = op_nan();
    return;
  }
  // point j = 0..K-1 of the curve: counts and threshold at the j-th distinct score from the top
  auto tp_at = [&](int j) -> long long { return cum[bnd[j]]; };
  auto fp_at = [&](int j) -> long long { const int i = bnd[j]; return (long long)i + 1 - cum[i]; };
  auto thr_at = [&](int j) -> double { return (double)key_score((uint32_t)(key[bnd[j]] >> 32)); };
  // the last point whose threshold is >= theta (its counts are those of `score >= theta`), -1 if there is none
  auto point_ge = [&](double theta) -> int {
    int lo = -1, hi = K;
    while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (thr_at(mid) >= theta) lo = mid; else hi = mid; }
    return lo;
  };
  // roc_curve's drop_intermediate: the ends and the corners of the curve
  auto kept = [&](int j, long long tp, long long fp) -> bool {
    if (j == 0 || j == K - 1) return true;
    const long long tp0 = tp_at(j - 1), fp0 = fp_at(j - 1), tp1 = tp_at(j + 1), fp1 = fp_at(j + 1);
    return (fp1 - 2 * fp + fp0 != 0) || (tp1 - 2 * tp + tp0 != 0);
  };
  const double dP = (double)P, dN = (double)Nn;

  for (int r = 0; r < n_rules; ++r) {
    const int kind = R.r[r].kind;
    double thr = op_nan(), obj = op_nan(), status = 0.0;
    if (kind == NM_OP_ROC) {                       // argmax(tpr - fpr) over the kept points, the origin (J = 0) first
      double bv = 0.0; int bo = -1;
      for (int j = t; j < K; j += MT) {
        const long long tp = tp_at(j), fp = fp_at(j);
        if (kept(j, tp, fp)) {
          const double J = (double)tp / dP - (double)fp / dN;
          if (J > bv) { bv = J; bo = j; }
        }
      }
      op_best<false>(bv, bo, redV, redI);
      thr = bo < 0 ? op_inf() : thr_at(bo);
      obj = bo < 0 ? 0.0 : bv;
    } else if (kind == NM_OP_F1 || kind == NM_OP_COST) {   // the linspace grid, first strict improvement
      const int ng = R.r[r].n;
      const double a = R.r[r].a, b = R.r[r].b, cfn = R.r[r].cost_fn, cfp = R.r[r].cost_fp;
      const double step = (b - a) / (double)(ng - 1);
      const bool f1 = kind == NM_OP_F1;
      const double init = f1 ? 0.0 : op_inf();
      double bv = init; int bo = -1;
      for (int i = t; i < ng; i += MT) {
        const double v = (i == ng - 1) ? b : (double)i * step + a;
        const int j = point_ge(v);
        const long long tp = j < 0 ? 0 : tp_at(j), fp = j < 0 ? 0 : fp_at(j);
        if (f1) {
          const double f = (double)(2 * tp) / (double)(P + tp + fp);
          if (f > bv) { bv = f; bo = i; }
        } else {
          const double c = (double)fp * cfp + (double)(P - tp) * cfn;
          if (c < bv) { bv = c; bo = i; }
        }
      }
      if (f1) op_best<false>(bv, bo, redV, redI); else op_best<true>(bv, bo, redV, redI);
      thr = bo < 0 ? 0.0 : ((bo == ng - 1) ? b : (double)bo * step + a);
      obj = bo < 0 ? init : bv;
    } else if (kind == NM_OP_PR || kind == NM_OP_F1MAX) {   // every distinct score, ascending: m = K - 1 - j
      const bool parity = kind == NM_OP_PR;
      double bv = 0.0; int bo = -1;
      for (int m = t; m < K; m += MT) {
        const int j = K - 1 - m;
        const long long tp = tp_at(j), fp = fp_at(j);
        double f;
        if (tp == 0) {
          f = parity ? op_inf() : 0.0;             // numpy's argmax stops at the first NaN: it beats every F1
        } else {
          const double p = (double)tp / (double)(tp + fp), rc = (double)tp / dP;
          f = 2.0 * (p * rc) / (p + rc);
        }
        if (bo < 0 || f > bv) { bv = f; bo = m; }
      }
      op_best<false>(bv, bo, redV, redI);
      const int j = K - 1 - bo;
      const bool hit_nan = parity && tp_at(j) == 0;
      thr = thr_at(j);
      obj = hit_nan ? op_nan() : bv;
      status = hit_nan ? 1.0 : 0.0;
    } else if (kind == NM_OP_EER) {                // nanargmin |fnr - fpr| over the kept points, the origin (1) first
      double bv = 1.0; int bo = -1;
      for (int j = t; j < K; j += MT) {
        const long long tp = tp_at(j), fp = fp_at(j);
        if (kept(j, tp, fp)) {
          const double d = fabs((1.0 - (double)tp / dP) - (double)fp / dN);
          if (d < bv) { bv = d; bo = j; }
        }
      }
      op_best<true>(bv, bo, redV, redI);
      thr = bo < 0 ? op_inf() : thr_at(bo);
      obj = bo < 0 ? 1.0 : bv;
    } else if (kind == NM_OP_SPEC) {               // the last point with tn >= ceil(a * n_neg): fp_j never falls with j
      const long long max_fp = (long long)Nn - (long long)ceil(R.r[r].a * dN);
      int lo = -1, hi = K;
      while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (fp_at(mid) <= max_fp) lo = mid; else hi = mid; }
      thr = lo < 0 ? op_inf() : thr_at(lo);
      obj = (double)(Nn - (lo < 0 ? 0 : fp_at(lo))) / dN;
    } else {
      status = -2.0;
    }
    if (t == 0) { sl[r * OP_SEL] = thr; sl[r * OP_SEL + 1] = obj; sl[r * OP_SEL + 2] = status; sl[r * OP_SEL + 3] = 0.0; }
  }

  if (summary) {
    long long a2 = 0, a2p = 0;                     // twice the trapezoid area in count units: all of it, up to max_fpr
    double ap = 0.0, frac = 0.0;                   // sum of (tp_j - tp_j-1) * precision_j; the one segment max_fpr cuts
    for (int j = t; j < K; j += MT) {
      const long long tp = tp_at(j), fp = fp_at(j);
      const long long tp0 = j > 0 ? tp_at(j - 1) : 0, fp0 = j > 0 ? fp_at(j - 1) : 0;
      const long long trap = (fp - fp0) * (tp + tp0);
      a2 += trap;
      ap += (double)(tp - tp0) * ((double)tp / (double)(tp + fp));
      const double x0 = (double)fp0 / dN, x1 = (double)fp / dN;
      if (x1 <= max_fpr) {
        a2p += trap;
      } else if (x0 < max_fpr) {
        const double y0 = (double)tp0 / dP, y1 = (double)tp / dP;
        const double ym = (max_fpr - x0) * ((y1 - y0) / (x1 - x0)) + y0;
        frac += (max_fpr - x0) * (y0 + ym) * 0.5;
      }
    }
    op_sums(a2, a2p, ap, frac, redA, redV);
    if (t == 0) {
      double* o = summary + (int64_t)s * NM_METRICS_STRIDE;
      const double auc = (double)a2 / (2.0 * dP * dN);
      const double part_auc = (double)a2p / (2.0 * dP * dN) + frac, min_area = 0.5 * max_fpr * max_fpr;
      // sensitivity at a fixed specificity: the last point with tn >= ceil(at_spec * n_neg); specificity at a fixed
      // sensitivity: the first point with tp >= ceil(at_sens * n_pos) (the last point has tp = n_pos)
      const long long max_fp = (long long)Nn - (long long)ceil(at_spec * dN), min_tp = (long long)ceil(at_sens * dP);
      int lo = -1, hi = K;
      while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (fp_at(mid) <= max_fp) lo = mid; else hi = mid; }
      const int js = lo;
      lo = -1; hi = K - 1;
      while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (tp_at(mid) >= min_tp) hi = mid; else lo = mid; }
      o[0] = auc;
      o[1] = ap / dP;
      o[2] = max_fpr == 1.0 ? auc : 0.5 * (1.0 + (part_auc - min_area) / (max_fpr - min_area));
      o[3] = js < 0 ? 0.0 : (double)tp_at(js) / dP;
      o[4] = (double)(Nn - fp_at(hi)) / dN;
      o[5] = (double)K; o[6] = dP; o[7] = dN;
    }
  }
  if (grid) {                                      // np.interp(linspace(0, 1, G), fpr, tpr) on the full curve, origin first
    const double gstep = 1.0 / (double)(G > 1 ? G - 1 : 1);
    for (int g = t; g < G; g += MT) {
      const double x = (g == G - 1 && G > 1) ? 1.0 : (double)g * gstep;
      int lo = -1, hi = K;                         // the last point with fpr <= x: the upper end of a vertical segment
      while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if ((double)fp_at(mid) / dN <= x) lo = mid; else hi = mid; }
      const double x0 = lo < 0 ? 0.0 : (double)fp_at(lo) / dN, y0 = lo < 0 ? 0.0 : (double)tp_at(lo) / dP;
      double y = y0;
      if (lo < K - 1 && x0 != x) {
        const double x1 = (double)fp_at(lo + 1) / dN, y1 = (double)tp_at(lo + 1) / dP;
        y = ((y1 - y0) / (x1 - x0)) * (x - x0) + y0;
      }
      grid[(int64_t)s * G + g] = y;
    }
  }
}

__global__ __launch_bounds__(MT) void op_apply_kernel(const float* __restrict__ scores, const int32_t* __restrict__ labels,
                                                      const int32_t* __restrict__ offsets, int n_sets, int n_rules,
                                                      const int32_t* __restrict__ select_of, const int32_t* __restrict__ eval_of,
                                                      const double* __restrict__ sel, double* __restrict__ out) {
  constexpr int NR = NM_OP_MAX_RULES;
  __shared__ int32_t red[2 * NR + 1][MT / 64];
  const int e = blockIdx.x, t = threadIdx.x;
  const int es = eval_of ? eval_of[e] : e, ss = select_of ? select_of[e] : e;
  double* o = out + (int64_t)e * n_rules * NM_METRICS_STRIDE;
  const bool named = es >= 0 && es < n_sets && ss >= 0 && ss < n_sets;
  const int base = named ? offsets[es] : 0, n = named ? offsets[es + 1] - base : 0;
  if (n <= 0) {                                    // an empty evaluation set (or an index that names no set)
    for (int k = t; k < n_rules * NM_METRICS_STRIDE; k += MT) o[k] = (k % NM_METRICS_STRIDE == 7) ? -2.0 : op_nan();
    return;
  }
  const double* sl = sel + (int64_t)ss * n_rules * OP_SEL;
  double thr[NR];
  int32_t tp[NR], fp[NR];
#pragma unroll
  for (int r = 0; r < NR; ++r) { thr[r] = r < n_rules ? sl[r * OP_SEL] : op_nan(); tp[r] = 0; fp[r] = 0; }
  int32_t pos = 0;
  for (int i = t; i < n; i += MT) {
    const double v = (double)scores[base + i];
    const int lab = labels[base + i] != 0;
    pos += lab;
#pragma unroll
    for (int r = 0; r < NR; ++r) {                 // (a NaN threshold, or a NaN score, predicts 0)
      const int hit = v >= thr[r];
      tp[r] += hit & lab;
      fp[r] += hit & (lab ^ 1);
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    pos += __shfl_xor(pos, off, 64);
#pragma unroll
    for (int r = 0; r < NR; ++r) { tp[r] += __shfl_xor(tp[r], off, 64); fp[r] += __shfl_xor(fp[r], off, 64); }
  }
  if ((t & 63) == 0) {
    const int w = t >> 6;
#pragma unroll
    for (int r = 0; r < NR; ++r) { red[2 * r][w] = tp[r]; red[2 * r + 1][w] = fp[r]; }
    red[2 * NR][w] = pos;
  }
  __syncthreads();
  if (t < n_rules) {
    const long long TP = (long long)red[2 * t][0] + red[2 * t][1] + red[2 * t][2] + red[2 * t][3];
    const long long FP = (long long)red[2 * t + 1][0] + red[2 * t + 1][1] + red[2 * t + 1][2] + red[2 * t + 1][3];
    const long long Pe = (long long)red[2 * NR][0] + red[2 * NR][1] + red[2 * NR][2] + red[2 * NR][3], Ne = n - Pe;
    double* row = o + t * NM_METRICS_STRIDE;
    const double status = sl[t * OP_SEL + 2];
    if (status == -2.0) {                          // the selection set has no curve
      for (int k = 0; k < NM_METRICS_STRIDE - 1; ++k) row[k] = op_nan();
      row[7] = -2.0;
    } else {
      const long long TN = Ne - FP;
      row[0] = sl[t * OP_SEL];
      row[1] = (double)(TP + TN) / (double)n;
      row[2] = Pe ? (double)TP / (double)Pe : op_nan();
      row[3] = Ne ? (double)TN / (double)Ne : op_nan();
      row[4] = (double)TP;
      row[5] = (double)FP;
      row[6] = sl[t * OP_SEL + 1];
      row[7] = status;
    }
  }
}

inline bool op_finite(double v) { return v - v == 0.0; }

}  // namespace

extern "C" {

size_t nm_operating_points_workspace(int n_sets, int n_rules) {
  if (n_sets < 1 || n_rules < 1 || n_rules > NM_OP_MAX_RULES) return 0;
  return (((size_t)n_sets * (size_t)n_rules * OP_SEL * sizeof(double)) + 255) & ~(size_t)255;
}

int nm_operating_points(const float* scores, const int32_t* labels, const int32_t* offsets, int n_sets, int max_set,
                        const nm_op_rule_t* rules, int n_rules, const int32_t* select_of, int n_eval, const int32_t* eval_of,
                        double at_spec, double at_sens, double max_fpr, void* workspace, size_t workspace_bytes,
                        double* rules_out, double* summary_out, double* grid_out, int G, void* stream) {
  if (!scores || !labels || !offsets || !rules || !workspace || !rules_out) return NM_E_NULL;
  if (G > 0 && !grid_out) return NM_E_NULL;
  if (n_sets < 1 || max_set < 1 || max_set > MAXN || n_rules < 1 || n_rules > NM_OP_MAX_RULES || n_eval < 1 || G < 0 ||
      G > NM_OP_MAX_GRID)
    return NM_E_METRICS;
  if (!(at_spec >= 0.0 && at_spec <= 1.0) || !(at_sens >= 0.0 && at_sens <= 1.0) || !(max_fpr > 0.0 && max_fpr <= 1.0))
    return NM_E_METRICS;
  OpRules R = {};
  for (int r = 0; r < n_rules; ++r) {
    const nm_op_rule_t& u = rules[r];
    if (u.kind < NM_OP_ROC || u.kind > NM_OP_SPEC) return NM_E_METRICS;
    if ((u.kind == NM_OP_F1 || u.kind == NM_OP_COST) &&
        (u.n < 2 || u.n > NM_OP_MAX_LINSPACE || !op_finite(u.a) || !op_finite(u.b))) return NM_E_METRICS;
    if (u.kind == NM_OP_COST && (!op_finite(u.cost_fn) || !op_finite(u.cost_fp))) return NM_E_METRICS;
    if (u.kind == NM_OP_SPEC && !(u.a >= 0.0 && u.a <= 1.0)) return NM_E_METRICS;
    R.r[r] = u;
  }
  if (workspace_bytes < nm_operating_points_workspace(n_sets, n_rules)) return NM_E_METRICS;
  double* sel = static_cast<double*>(workspace);
  int e = launch_kernel(op_select_kernel, dim3(n_sets), dim3(MT), METRICS_SMEM, stream, scores, labels, offsets, R, n_rules, at_spec,
                        at_sens, max_fpr, sel, summary_out, G > 0 ? grid_out : (double*)nullptr, G);
  if (e) return e;
  return launch_kernel(op_apply_kernel, dim3(n_eval), dim3(MT), 0, stream, scores, labels, offsets, n_sets, n_rules, select_of, eval_of,
                       (const double*)sel, rules_out);
}

}  // extern "C"
