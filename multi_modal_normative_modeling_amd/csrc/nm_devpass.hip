// nm_devpass.hip -- the ROI-wise deviation pass as its own kernel (libnmhip.so, third translation unit).
//
// The pass of multimodal_kfold_train_cvae_supervised_regression.py:163-192 (and utils_vae.py:147-152): per modality the
// unimodal encoder -> sampled z -> decoder, (x - x_hat)^2 per ROI and its row mean, for ALL subjects.  Forward only, one
// expert, nothing saved: the general forward-only step (nm_step_kernel<false, 3>) spends a 256-row tile's 178 k cycles
// mostly waiting -- eight dependent phases of one 8-wave workgroup, each behind a staged weight image and a barrier --
// with the CU's other half idle, because its LDS plan (P, Q as [256][136], S) takes 159 of 160 KB.
//
// Here a workgroup owns 128 rows (RT = 4) and 75 KB of LDS, so TWO workgroups share a CU and fill each other's waits:
//   P  [128][136] bf16  the running activation
//   W  [128][136] bf16  ONE weight image at a time (requested as soon as the layer before it has drained W; the other
//                        workgroup on the CU works meanwhile), or two first-layer stages together with P, or the two
//                        [64][136] output-chunk slots (their bias / logvar_out pieces go to the two vector slots), or --
//                        beside the 32-row heads image -- the sampled z as bf16 [128][32]
// 16-row MFMA tiles at or beyond the tile's valid rows are skipped in every phase (a 1064-row table costs 1064 rows
// rounded to 16, not 5 x 256; their export rows are zeroed, dv_zero_dead_rows), and the export epilogue makes one pass:
// residual, its square (stored), row sum.
// Arithmetic, draws (keyed by absolute row) and exports are those of the general kernel, row by row: the two agree bit for
// bit on out_sqerr / out_rowdev / out_loc (tests/test_gpu_devpass.py).  No loss log, no latent exports: launches that want
// those, a first hidden layer wider than 112 or a latent wider than 32 stay on nm_forward.  Models with several experts
// run on nm_devpass_multi_kernel, further down in this file; the joint latent statistics alone (no decoder) come from
// nm_latent_kernel, at its end.
#include "nm_core.inc"

// export stores: plain, not non-temporal ("written once, read by another kernel"), as the A/B decided: 458 us per pass
// non-temporal against 328 us plain (profiles/r04k_ab_devpass_export_stores.txt) -- a row's 256 bytes of a chunk leave
// as four 64-byte stores; plain stores merge in L2 into full lines before they go to memory, the streaming policy sent
// them on as partial lines.
constexpr int DV_RT = 4;
constexpr int DV_ROWS = DV_RT * 32;                                   // 128
constexpr int DV_P_BYTES = DV_ROWS * LDP * 2;                         // 34,816
constexpr int DV_W_BYTES = IMG_BYTES;                                 // 34,816
constexpr int DV_X_PIECES = (DV_ROWS * LDX * 2) >> 10;                // 18: a [128][72] x chunk
constexpr int DV_W0_PIECES = (DV_P_BYTES >> 10) - DV_X_PIECES;        // 16: what is left of a stage for the weight chunk
constexpr int DV_MAX_H0 = (DV_W0_PIECES << 10) / (LDX * 2) / 16 * 16; // 112 rows
constexpr int DV_Z_OFF = 64 * LDP * 2;                                // z [128][32] bf16 inside W, behind the (<= 64-row) heads image
constexpr int DV_MISC_FLOATS = 64 + 128 + 128 + 16 + 4;
constexpr int DV_SMEM = DV_P_BYTES + DV_W_BYTES + 2 * VEC_BYTES + DV_MISC_FLOATS * 4;
static_assert(2 * DV_SMEM <= 160 * 1024, "two workgroups per CU");
static_assert(2 * OIMG_BYTES <= DV_W_BYTES && DV_Z_OFF % 16 == 0 && DV_Z_OFF + DV_ROWS * 32 * 2 <= DV_W_BYTES, "W layout");

__device__ __forceinline__ void dv_carve(Ctx& c, unsigned char* smem) {
  c.wave_s = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  c.rsk = 1; c.rsq = 0; c.rloc0 = 0; c.gpart = nullptr; c.gp_stride = 0; c.ws0 = nullptr; c.xwg = 0; c.gwt = 0;
  c.P = reinterpret_cast<__bf16*>(smem);
  c.Q = c.P + DV_ROWS * LDP;                                         // = W
  c.stage = nullptr;                                                  // (no S in this plan)
  c.vec = reinterpret_cast<float*>(smem + DV_P_BYTES + DV_W_BYTES);
  c.red = c.vec + 2 * (VEC_BYTES / 4);
  c.colacc = c.red + 64;
  c.rowacc = c.colacc + 128;
  c.lse = nullptr; c.bgrad = nullptr;
  c.tlast = reinterpret_cast<unsigned long long*>(c.rowacc + 128);
  c.abort = reinterpret_cast<unsigned*>(c.tlast + 8);
}

// The export rows of a 128-row tile that the output phase leaves alone: the dead 16-row tiles of out_loc / out_sqerr (rows
// [live rounded up to 16, 128); a live 16-row tile's own rows past the table's end are stored as zeros by its wave) and every
// row of out_rowdev from `live` on.  They come back as zeros whatever the buffers held before the launch -- the export
// buffers hold whole 256-row tiles, and the general kernel stores the whole tile.  live = 0: a tile without a table row.
__device__ __forceinline__ void dv_zero_dead_rows(const nm_modality_t& md, int row0, int live) {
  const int xp = md.x_pitch, r16 = rup(live, 16);
  for (int e = threadIdx.x; e < (DV_ROWS - r16) * (xp >> 2); e += WG) {
    const int64_t gi = (int64_t)(row0 + r16) * xp + (int64_t)e * 4;
    if (md.out_loc) *(GAS f32x4*)(asg(md.out_loc) + gi) = f32x4{0.f, 0.f, 0.f, 0.f};
    if (md.out_sqerr) *(GAS f32x4*)(asg(md.out_sqerr) + gi) = f32x4{0.f, 0.f, 0.f, 0.f};
  }
  if (md.out_rowdev)
    for (int r = live + (int)threadIdx.x; r < DV_ROWS; r += WG) asg(md.out_rowdev)[row0 + r] = 0.f;
}

// One hidden layer, P -> P in place, image in W (requested by the phase before, its vector piece in slot `vs`): wait, GEMM
// over the live row tiles, then -- W drained -- request `nx` into W, then the activation epilogue.
__device__ __forceinline__ void dv_layer(const Ctx& cc, int vs, const Next& nx, int N, int K, bool act, int live) {
  constexpr int RT = DV_RT, WROWS = DV_RT * 16;
  Ctx c = cc;
  relaunder(c);
  const int ksteps = wpad(K) / 32, ntn = wpad(N) / 16;
  wait_vm(0);
  lds_barrier();
  f32x4 acc[2][RT];
  zero_acc(acc);
#pragma unroll
  for (int ks = 0; ks < 4; ++ks) {
    if (ks < ksteps) {
      bf16x8 wf[2];
#pragma unroll
      for (int t = 0; t < 2; ++t) wf[t] = lds_frag(c.Q, LDP, (c.wn + 4 * t) * 16 + c.c16, ks * 32 + 8 * c.g);
#pragma unroll
      for (int rt = 0; rt < RT; ++rt) {
        if (c.wm * WROWS + rt * 16 < live) {
          bf16x8 a = lds_frag(c.P, LDP, c.wm * WROWS + rt * 16 + c.c16, ks * 32 + 8 * c.g);
#pragma unroll
          for (int t = 0; t < 2; ++t) acc[t][rt] = mfma(wf[t], a, acc[t][rt]);
        }
      }
    }
  }
  lds_barrier();                       // every wave has finished reading P and W
  issue_next(c, nx);
  act_to_P(c, acc, c.vec + vs * (VEC_BYTES / 4), N, ntn, act);
}

__global__ __launch_bounds__(WG, 4) void nm_devpass_kernel(const nm_job_t* __restrict__ jobs, int tile0, int flags) {
  constexpr int RT = DV_RT, ROWS = DV_ROWS;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const nm_job_t* J = jobs + blockIdx.x;
  const int t128 = tile0 + (int)blockIdx.y;
  const int row0 = t128 * ROWS;
  if (row0 >= J->n_rows) {
    // the second half of a ragged last 256-row tile: its export rows come back as zeros, as from the general kernel
    if (row0 < (J->n_rows + TROWS - 1) / TROWS * TROWS) dv_zero_dead_rows(J->mod[0], row0, 0);
    return;
  }
  Ctx c;
  c.job = J;
  c.part = -1; c.nparts = 1; c.lstep = 0;
  c.slope = J->act_slope;
  dv_carve(c, smem);
  relaunder(c);
  c.flags = NM_F_EXPORT | (flags & NM_F_TRACE);
  c.t_last = 0;
  c.ws = nullptr;
  for (int i = c.tid; i < DV_SMEM / 4; i += WG) reinterpret_cast<uint32_t*>(smem)[i] = 0u;
  __syncthreads();
  if (c.flags & 64) c.tlast[c.wave_s] = clock64();
  c.row0 = row0;
  c.rloc0 = row0 % TROWS;                         // (the draw buffer holds whole 256-row batches)
  c.nrows = min(ROWS, J->n_rows - row0);
  c.inv_b = 1.0f / (float)c.nrows;
  const int live = c.nrows;
  const int step = row0 / TROWS;                  // the batch this tile belongs to = the general kernel's step index
  const nm_modality_t& md = J->mod[0];
  const int L = J->L, Z = J->Z, C = J->C, D = md.D;
  const int Zs = rup(Z, 16);
  const bool nl = J->non_linear != 0;
  const bool vec4 = (Z & 3) == 0;
  GAS char* const wsh = (GAS char*)J->wsh;
  char* const Wb = reinterpret_cast<char*>(c.Q);
  __bf16* const zlds = reinterpret_cast<__bf16*>(Wb + DV_Z_OFF);
  auto to_W = [&](const GAS char* blob, int vs, int rows, int K) {
    return Next{blob, Wb, IMG_BYTES >> 10, blob + cimg_bytes(rows, K), reinterpret_cast<char*>(c.vec) + vs * VEC_BYTES, rows, blob_kp(K)};
  };

  // ---- encoder ----
  const int nch = (md.Kx + XCH - 1) / XCH;
  const GAS char* after0 = wsh + (L > 1 ? md.enc_s[1] : md.heads_s);
  fwd_first_layer<RT>(c, (const GAS char*)asg(md.xb) + (int64_t)(row0 / TROWS) * nch * XIMG_TILE_BYTES + (int64_t)c.rloc0 * (LDX * 2),
                      md.Kx, wsh + md.enc_s[0], to_W(after0, 0, L > 1 ? J->H[1] : 2 * Zs, J->H[0]), J->H[0], nl, (gbf16)nullptr, true,
                      DV_W0_PIECES, live);
  int vs = 0;
  for (int e = 1; e < L; ++e) {
    const GAS char* nxt = wsh + (e + 1 < L ? md.enc_s[e + 1] : md.heads_s);
    dv_layer(c, vs, to_W(nxt, vs ^ 1, e + 1 < L ? J->H[e + 1] : 2 * Zs, J->H[e]), J->H[e], J->H[e - 1], nl, live);
    vs ^= 1;
  }
  tr(c, 1);
  // heads + the latent draw in their epilogue (z -> W behind the heads image; nothing requested meanwhile: W is in use)
  wait_vm(0);
  float kl_unused = 0.f;
  fwd_heads<RT>(c, 0, no_next(), Z, J->H[L - 1], (gf32)nullptr, (gf32)nullptr, Zs, 0, zlds, step, vec4, &kl_unused,
                c.vec + vs * (VEC_BYTES / 4));
  tr(c, 2);
  // ---- decoder ----
  relaunder(c);
  build_zc<RT>(c, c.P, md, (gcf32)nullptr, (gcf32)nullptr, Z, C, Zs, 0, (gcf32)nullptr, zlds);
  lds_barrier();                                   // z is consumed: W is free
  issue_next(c, to_W(wsh + md.dec_s[0], 0, J->H[L - 1], Z + C));
  tr(c, 4);
  vs = 0;
  const GAS char* oblob = wsh + md.out_s;
  const int nck = (D + OCH - 1) / OCH;
  // chunk ch: its [64][136] rows into half ch & 1 of W, its vectors into slot (ch + ob) & 1 -- ob such that chunk 0's vectors
  // do not land on the bias the last hidden layer's epilogue is still reading (L layers: that one sits in slot (L - 1) & 1)
  const int ob = L & 1;
  auto out_blob = [&](int ch) {
    return Next{oblob + (int64_t)ch * OBLOB_BYTES, Wb + (ch & 1) * OIMG_BYTES, OIMG_BYTES >> 10,
                oblob + (int64_t)ch * OBLOB_BYTES + OIMG_BYTES, reinterpret_cast<char*>(c.vec) + ((ch + ob) & 1) * VEC_BYTES, 0, 0};
  };
  for (int d = 0; d < L; ++d) {
    const int Kin = (d == 0) ? Z + C : J->H[L - d], Nout = J->H[L - 1 - d];
    const Next nx = (d + 1 < L) ? to_W(wsh + md.dec_s[d + 1], vs ^ 1, J->H[L - 2 - d], Nout) : out_blob(0);
    dv_layer(c, vs, nx, Nout, Kin, nl, live);
    vs ^= 1;
  }
  tr(c, 5);
  // ---- output layer in 64-ROI chunks: x_hat, (x - x_hat)^2, row sums ----
  // Wave grid of this phase: wave w owns rows [16 w, 16 w + 16) of the tile and ALL 64 columns of a chunk (four feature
  // tiles): a row's 256 bytes of a chunk are then stored by four consecutive instructions of ONE wave (64 bytes each),
  // which the memory system merges into full lines -- with the GEMM phases' 2 x 4 grid the two halves of every 128-byte
  // line came from two waves at different times, and the pass was bound by partial-line writes.  A row's sum needs no
  // cross-wave step either.  Same MFMA and LDS-read counts as before (one P fragment and four weight fragments per k step).
  const int Hl = J->H[0];
  gcf32 xf = asg(md.x_f32);
  const int xp = md.x_pitch;
  const bool sigm = J->out_kind == 1;
  float rdev = 0.f;
  const int orow = c.wave * 16 + c.c16;            // this lane's row of the tile
  const bool wave_live = c.wave * 16 < live;       // (wave-uniform: a dead 16-row tile's wave only keeps the barriers)
  auto load_xin = [&](int chx, f32x4 (&xv)[4]) {
#pragma unroll
    for (int ft = 0; ft < 4; ++ft) {
      const int dcl = min(chx * OCH + ft * 16 + 4 * c.g, xp - 4);
      xv[ft] = *(const GAS f32x4*)(xf + (int64_t)(row0 + orow) * xp + dcl);
    }
  };
  int stores_prev = 0;                             // export stores this wave issued in the previous chunk (wave-uniform)
  auto chunk = [&](const int ch, f32x4 (&xin)[4], f32x4 (&xnx)[4]) {
    relaunder(c);
    const int d0 = ch * OCH;
    const __bf16* Wc = reinterpret_cast<const __bf16*>(Wb + (ch & 1) * OIMG_BYTES);
    const float* vb = c.vec + ((ch + ob) & 1) * (VEC_BYTES / 4);       // bias[64], then logvar_out[64]
    // chunk ch's rows, vectors and inputs (requested a chunk ago) have landed; the previous chunk's export stores, issued
    // after them, may stay in flight
    wait_vm(ch > 0 ? stores_prev : 0);
    lds_barrier();                                  // ... for every wave; the previous chunk is finished everywhere
    if (ch + 1 < nck) { issue_next(c, out_blob(ch + 1)); if (wave_live) load_xin(ch + 1, xnx); }
    stores_prev = 0;
    if (!wave_live) return;
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
    tr(c, 6);
    const bool rv = orow < c.nrows;
    const bool full = live == ROWS && d0 + OCH <= D && !sigm;          // no row / column masks needed (wave-uniform)
#pragma unroll
    for (int ft = 0; ft < 4; ++ft) {
      const int dg0 = d0 + ft * 16 + 4 * c.g;
      const f32x4 bo = *reinterpret_cast<const f32x4*>(vb + ft * 16 + 4 * c.g);
      f32x4 lo, sq;
      if (full) {
        lo = acc[ft] + bo;
        const f32x4 diff = lo - xin[ft];
        sq = diff * diff;
      } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          float xh = acc[ft][i] + bo[i];
          if (sigm) xh = 1.0f / (1.0f + expf(-xh));
          const bool dv = rv && dg0 + i < D;
          const float diff = xh - xin[ft][i];
          lo[i] = dv ? xh : 0.f;
          sq[i] = dv ? diff * diff : 0.f;
        }
      }
      rdev += ((sq[0] + sq[1]) + sq[2]) + sq[3];
      // (whole tiles are stored, zeros on the rows past the table's end -- the export buffers hold whole 256-row tiles)
      if (d0 + ft * 16 < xp) {                      // wave-uniform
        if (dg0 < xp) {
          const int64_t gi = (int64_t)(row0 + orow) * xp + dg0;
          if (md.out_loc) *(GAS f32x4*)(asg(md.out_loc) + gi) = lo;
          if (md.out_sqerr) *(GAS f32x4*)(asg(md.out_sqerr) + gi) = sq;
        }
        stores_prev += (md.out_loc ? 1 : 0) + (md.out_sqerr ? 1 : 0);
      }
    }
    tr(c, 7);
  };
  {
    f32x4 xa[4], xb[4];
    if (wave_live) load_xin(0, xa);
    for (int ch = 0; ch < nck; ch += 2) {
      chunk(ch, xa, xb);
      if (ch + 1 < nck) chunk(ch + 1, xb, xa);
    }
  }
  if (md.out_rowdev && wave_live) {                 // the row's four column groups sit in the lanes c16, c16 + 16, + 32, + 48
    float v = rdev;
    v += __shfl_xor(v, 16, 64);
    v += __shfl_xor(v, 32, 64);
    if (c.g == 0 && orow < c.nrows) asg(md.out_rowdev)[row0 + orow] = v / (float)D;
  }
  if (live < ROWS) dv_zero_dead_rows(md, row0, live);   // (a ragged tile only: the rows no wave has stored)
  tr(c, 8);
}

// ---------------------------------------------------------------------------------------------------------------------
// nm_devpass_multi_kernel -- the same pass for models with several experts (SE: 3, UCA: 4): pred_recon with the joint
// latent, then reconstruction_deviation_multimodal (multimodal_kfold_test_cvae_supervised.py:112-113).
//
// A workgroup owns 128 rows as above.  Per tile: every expert's encoder chain (first layer, dv_layer, heads), the fusion
// of the experts and the latent draw, then every decoder (z | c | 1, hidden layers, 64-ROI output chunks with the export
// epilogue of nm_devpass_kernel -- that kernel's source stays as it is, so the chunk loop is repeated here per decoder).
//
// Expert statistics: [M][128][Zs] fp32 x 2 is 128 KB at M = 4, Zs = 32 -- it does not fit beside P and W.  As in the
// general kernel, fwd_heads stores mu_m / logvar_m to the workspace tile of the 256-row batch and the fusion reads them
// back through the SAME fuse_fwd / softmax_alpha (fp contraction off), so the joint statistics agree bit for bit by
// construction.  The two workgroups of one batch share that batch's workspace tile on disjoint row halves (rloc0 = row0 %
// 256; a row's statistics are whole cache lines); neither touches the tile's hand-off words.  The traffic stays in L2.
//
// LDS: P, W, the two vector slots and the scalars as above, plus Z [128][32] bf16 (8 KB): the sampled z, which every
// decoder's z | c | 1 build reads (the covariates may differ per modality, so each decoder builds its own).  79.3 KB.
// z = mu_j + eps exp(logvar_j / 2) is formed in one register with the addition kept apart from the product (the general
// kernel adds two values it reloads from the workspace: no fused multiply-add there).
//
// A job nm_devpass_multi_ok refuses must not reach this kernel (the caller checks on the host, as for nm_devpass); its
// workgroups leave at once, exports untouched, because its shapes would not fit the LDS plan.
constexpr int DVM_Z_BYTES = DV_ROWS * 32 * 2;                         // 8,192
constexpr int DVM_SMEM = DV_SMEM + DVM_Z_BYTES;
static_assert(2 * DVM_SMEM <= 160 * 1024, "two workgroups per CU");
static_assert((DV_SMEM & 15) == 0, "z buffer alignment");

__host__ __device__ inline int dvm_refused(const nm_job_t* j) {
  const int Me = j->M_enc > 0 ? j->M_enc : j->M;
  if (j->wide || j->M < 2 || j->M > NM_MAX_EXP || Me != j->M) return NM_E_DEVPASS;
  if (j->n_private != 0 || j->tc_weight != 0.f || j->w_off >= 0 || j->out_kind != 0) return NM_E_DEVPASS;
  if (j->H[0] > DV_MAX_H0 || rup(j->Z, 16) > 32) return NM_E_DEVPASS;
  return 0;
}

// the sum the general kernel forms in build_zc from two reloaded values: never a fused multiply-add
__device__ __forceinline__ float dvm_add(float a, float b) {
#pragma clang fp contract(off)
  return a + b;
}

__global__ __launch_bounds__(WG, 4) void nm_devpass_multi_kernel(const nm_job_t* __restrict__ jobs, int tile0, int flags) {
  constexpr int RT = DV_RT, ROWS = DV_ROWS;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const nm_job_t* J = jobs + blockIdx.x;
  if (dvm_refused(J) || !J->workspace) return;
  const int M = J->M;
  const int t128 = tile0 + (int)blockIdx.y;
  const int row0 = t128 * ROWS;
  if (row0 >= J->n_rows) {
    // the second half of a ragged last 256-row tile: every modality's export rows come back as zeros
    if (row0 < (J->n_rows + TROWS - 1) / TROWS * TROWS)
      for (int m = 0; m < M; ++m) dv_zero_dead_rows(J->mod[m], row0, 0);
    return;
  }
  Ctx c;
  c.job = J;
  c.part = -1; c.nparts = 1; c.lstep = 0;
  c.slope = J->act_slope;
  dv_carve(c, smem);
  relaunder(c);
  c.flags = NM_F_EXPORT | (flags & NM_F_TRACE);
  c.t_last = 0;
  // the workspace tile of this tile's 256-row batch (tiles of the launch are counted from the batch tile0 falls in)
  c.ws = (GAS char*)J->workspace + (int64_t)(t128 / 2 - tile0 / 2) * J->workspace_stride;
  for (int i = c.tid; i < DVM_SMEM / 4; i += WG) reinterpret_cast<uint32_t*>(smem)[i] = 0u;
  __syncthreads();
  if (c.flags & 64) c.tlast[c.wave_s] = clock64();
  c.row0 = row0;
  c.rloc0 = row0 % TROWS;
  c.nrows = min(ROWS, J->n_rows - row0);
  c.inv_b = 1.0f / (float)c.nrows;
  const int live = c.nrows;
  const int step = row0 / TROWS;
  const int L = J->L, Z = J->Z, C = J->C;
  const int Zs = rup(Z, 16);
  const bool nl = J->non_linear != 0;
  const bool vec4 = (Z & 3) == 0;
  GAS char* const wsh = (GAS char*)J->wsh;
  char* const Wb = reinterpret_cast<char*>(c.Q);
  __bf16* const zlds = reinterpret_cast<__bf16*>(smem + DV_SMEM);
  const WsLayout wl = ws_layout(M, L, Z);
  // this workgroup's rows of the batch's expert statistics; expert m at + m * 256 * Zs
  gf32 ws_mu_m = (gf32)(c.ws + wl.mu_m) + c.rloc0 * Zs;
  gf32 ws_lv_m = (gf32)(c.ws + wl.lv_m) + c.rloc0 * Zs;
  auto to_W = [&](const GAS char* blob, int vs, int rows, int K) {
    return Next{blob, Wb, IMG_BYTES >> 10, blob + cimg_bytes(rows, K), reinterpret_cast<char*>(c.vec) + vs * VEC_BYTES, rows, blob_kp(K)};
  };

  // ---- encoders: every expert's chain, statistics to the workspace ----
  for (int m = 0; m < M; ++m) {
    relaunder(c);
    const nm_modality_t& md = J->mod[m];
    const int nch = (md.Kx + XCH - 1) / XCH;
    const GAS char* after0 = wsh + (L > 1 ? md.enc_s[1] : md.heads_s);
    fwd_first_layer<RT>(c, (const GAS char*)asg(md.xb) + (int64_t)(row0 / TROWS) * nch * XIMG_TILE_BYTES + (int64_t)c.rloc0 * (LDX * 2),
                        md.Kx, wsh + md.enc_s[0], to_W(after0, 0, L > 1 ? J->H[1] : 2 * Zs, J->H[0]), J->H[0], nl, (gbf16)nullptr, true,
                        DV_W0_PIECES, live);
    int vs = 0;
    for (int e = 1; e < L; ++e) {
      const GAS char* nxt = wsh + (e + 1 < L ? md.enc_s[e + 1] : md.heads_s);
      dv_layer(c, vs, to_W(nxt, vs ^ 1, e + 1 < L ? J->H[e + 1] : 2 * Zs, J->H[e]), J->H[e], J->H[e - 1], nl, live);
      vs ^= 1;
    }
    tr(c, 1);
    wait_vm(0);
    fwd_heads<RT>(c, 0, no_next(), Z, J->H[L - 1], ws_mu_m + (int64_t)m * TROWS * Zs, ws_lv_m + (int64_t)m * TROWS * Zs, Zs, 0,
                  (__bf16*)nullptr, step, vec4, (float*)nullptr, c.vec + vs * (VEC_BYTES / 4));
  }

  // ---- fusion + the latent draw: z -> LDS ----
  handoff_barrier();                               // the heads' stores are complete for every thread of the workgroup
  // W and P are free: the first decoder's image lands during the latent arithmetic
  issue_next(c, to_W(wsh + J->mod[0].dec_s[0], 0, J->H[L - 1], Z + C));
  {
    float al[NM_MAX_EXP] = {0.f, 0.f, 0.f, 0.f};
    if (J->combine == NM_COMBINE_GPOE) softmax_alpha(J, al);
    relaunder(c);
    if (vec4) {
      const int nq4 = (Z + 3) >> 2;
      const float rq4 = 1.0f / (float)nq4;
#pragma unroll 2
      for (int e = c.tid; e < ROWS * nq4; e += WG) {
        const int r = idiv(e, nq4, rq4), z0 = 4 * (e - r * nq4);
        f32x4 mu4[NM_MAX_EXP], lv4[NM_MAX_EXP];
#pragma unroll
        for (int m = 0; m < NM_MAX_EXP; ++m) {
          mu4[m] = f32x4{0.f, 0.f, 0.f, 0.f};
          lv4[m] = mu4[m];
          if (m < M) {
            mu4[m] = *(const GAS f32x4*)(ws_mu_m + ((int64_t)m * TROWS + r) * Zs + z0);
            lv4[m] = *(const GAS f32x4*)(ws_lv_m + ((int64_t)m * TROWS + r) * Zs + z0);
          }
        }
        float ep[4];
        if (J->eps) {
#pragma unroll
          for (int i = 0; i < 4; ++i) ep[i] = asg(J->eps)[((int64_t)(step % J->eps_cap) * TROWS + c.rloc0 + r) * Z + min(z0 + i, Z - 1)];
        } else {
          randn2_ctr(J->seed, (uint32_t)step, (uint32_t)(c.row0 + r), (uint32_t)(z0 >> 1), ep[0], ep[1]);
          randn2_ctr(J->seed, (uint32_t)step, (uint32_t)(c.row0 + r), (uint32_t)(z0 >> 1) + 1u, ep[2], ep[3]);
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) ep[i] = (z0 + i < Z) ? ep[i] : 0.f;
        bf16x4 zk;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          Lat Lt;
#pragma unroll
          for (int m = 0; m < NM_MAX_EXP; ++m) { Lt.mu[m] = mu4[m][i]; Lt.lv[m] = lv4[m][i]; }
          const Fuse f = fuse_fwd(J, Lt, al);
          const float es = ep[i] * fx_exp(0.5f * f.lv);
          zk[i] = (__bf16)dvm_add(f.mu, es);
        }
        *reinterpret_cast<bf16x4*>(zlds + r * 32 + z0) = zk;
      }
    } else {
      const float rZ = 1.0f / (float)Z;
#pragma unroll 2
      for (int e = c.tid; e < ROWS * Z; e += WG) {
        const int r = idiv(e, Z, rZ), z = e - r * Z;
        Lat Lt;
#pragma unroll
        for (int m = 0; m < NM_MAX_EXP; ++m) {
          Lt.mu[m] = (m < M) ? ws_mu_m[((int64_t)m * TROWS + r) * Zs + z] : 0.f;
          Lt.lv[m] = (m < M) ? ws_lv_m[((int64_t)m * TROWS + r) * Zs + z] : 0.f;
        }
        const Fuse f = fuse_fwd(J, Lt, al);
        const float ep = J->eps ? asg(J->eps)[((int64_t)(step % J->eps_cap) * TROWS + c.rloc0 + r) * Z + z]
                                : randn_ctr(J->seed, (uint32_t)step, (uint32_t)(c.row0 + r), (uint32_t)z);
        const float es = ep * fx_exp(0.5f * f.lv);
        zlds[r * 32 + z] = (__bf16)dvm_add(f.mu, es);
      }
    }
  }
  lds_barrier();                                   // z is complete (the decoder image requested above stays in flight)
  tr(c, 3);

  // ---- decoders ----
  const int Hl = J->H[0];
  const int ob = L & 1;                            // (see nm_devpass_kernel: chunk 0's vectors avoid the last hidden layer's bias)
  for (int m = 0; m < M; ++m) {
    relaunder(c);
    const nm_modality_t& md = J->mod[m];
    const int D = md.D;
    if (m > 0) {
      lds_barrier();                               // the previous decoder's last chunk is finished everywhere: P, W, vectors free
      issue_next(c, to_W(wsh + md.dec_s[0], 0, J->H[L - 1], Z + C));
    }
    build_zc<RT>(c, c.P, md, (gcf32)nullptr, (gcf32)nullptr, Z, C, Zs, 0, (gcf32)nullptr, zlds);
    tr(c, 4);
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
      dv_layer(c, vs, nx, Nout, Kin, nl, live);    // (its first barrier also publishes z | c | 1)
      vs ^= 1;
    }
    tr(c, 5);
    // output layer in 64-ROI chunks, wave w owns rows [16 w, 16 w + 16) and all 64 columns: see nm_devpass_kernel
    gcf32 xf = asg(md.x_f32);
    const int xp = md.x_pitch;
    float rdev = 0.f;
    const int orow = c.wave * 16 + c.c16;
    const bool wave_live = c.wave * 16 < live;
    auto load_xin = [&](int chx, f32x4 (&xv)[4]) {
#pragma unroll
      for (int ft = 0; ft < 4; ++ft) {
        const int dcl = min(chx * OCH + ft * 16 + 4 * c.g, xp - 4);
        xv[ft] = *(const GAS f32x4*)(xf + (int64_t)(row0 + orow) * xp + dcl);
      }
    };
    int stores_prev = 0;
    auto chunk = [&](const int ch, f32x4 (&xin)[4], f32x4 (&xnx)[4]) {
      relaunder(c);
      const int d0 = ch * OCH;
      const __bf16* Wc = reinterpret_cast<const __bf16*>(Wb + (ch & 1) * OIMG_BYTES);
      const float* vb = c.vec + ((ch + ob) & 1) * (VEC_BYTES / 4);
      wait_vm(ch > 0 ? stores_prev : 0);
      lds_barrier();
      if (ch + 1 < nck) { issue_next(c, out_blob(ch + 1)); if (wave_live) load_xin(ch + 1, xnx); }
      stores_prev = 0;
      if (!wave_live) return;
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
      tr(c, 6);
      const bool rv = orow < c.nrows;
      const bool full = live == ROWS && d0 + OCH <= D;                   // no row / column masks needed (wave-uniform)
#pragma unroll
      for (int ft = 0; ft < 4; ++ft) {
        const int dg0 = d0 + ft * 16 + 4 * c.g;
        const f32x4 bo = *reinterpret_cast<const f32x4*>(vb + ft * 16 + 4 * c.g);
        f32x4 lo, sq;
        if (full) {
          lo = acc[ft] + bo;
          const f32x4 diff = lo - xin[ft];
          sq = diff * diff;
        } else {
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const float xh = acc[ft][i] + bo[i];
            const bool dv = rv && dg0 + i < D;
            const float diff = xh - xin[ft][i];
            lo[i] = dv ? xh : 0.f;
            sq[i] = dv ? diff * diff : 0.f;
          }
        }
        rdev += ((sq[0] + sq[1]) + sq[2]) + sq[3];
        if (d0 + ft * 16 < xp) {                      // wave-uniform
          if (dg0 < xp) {
            const int64_t gi = (int64_t)(row0 + orow) * xp + dg0;
            if (md.out_loc) *(GAS f32x4*)(asg(md.out_loc) + gi) = lo;
            if (md.out_sqerr) *(GAS f32x4*)(asg(md.out_sqerr) + gi) = sq;
          }
          stores_prev += (md.out_loc ? 1 : 0) + (md.out_sqerr ? 1 : 0);
        }
      }
      tr(c, 7);
    };
    {
      f32x4 xa[4], xb[4];
      if (wave_live) load_xin(0, xa);
      for (int ch = 0; ch < nck; ch += 2) {
        chunk(ch, xa, xb);
        if (ch + 1 < nck) chunk(ch + 1, xb, xa);
      }
    }
    if (md.out_rowdev && wave_live) {
      float v = rdev;
      v += __shfl_xor(v, 16, 64);
      v += __shfl_xor(v, 32, 64);
      if (c.g == 0 && orow < c.nrows) asg(md.out_rowdev)[row0 + orow] = v / (float)D;
    }
    if (live < ROWS) dv_zero_dead_rows(md, row0, live);   // (a ragged tile only: the rows no wave has stored)
    tr(c, 8);
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// nm_devpass_subsets_kernel -- the pass above with the experts of every row fused n_subsets times, each time over another
// subset of them: encoders once per tile, then per entry of the job's nm_subset_t row the fusion under that entry's mask,
// the latent draw, and the decoders the entry exports (nm_devpass_multi_kernel's source stays as it is: its decoder loop is
// repeated here with the export pointers taken from the entry).
//
// Per row r and entry s: E = mask_s & present_s[r] (no present bytes: every expert).  The combiner is fuse_fwd's with the
// sums over E and |E| in the place of M (dvs_fuse / dvs_softmax below keep its operations in its order, fp contraction
// off: under the full mask they ARE fuse_fwd / softmax_alpha, which is what makes the full-mask entry equal
// nm_devpass_multi_kernel bit for bit); never the single-expert bypass.  The draw is the full pass's draw of that row.
// A row with E empty gets z = 0 and NaN exports; a row whose present byte lacks bit m gets NaN in out_sqerr[m] /
// out_rowdev[m] (x is a placeholder there), out_loc[m] stays the prediction.
//
// Geometry, LDS plan (P, W, vector slots, scalars, Z [128][32] bf16), workspace tile and dvm_refused domain are those of
// nm_devpass_multi_kernel; the LDS plan grows by the gPoE weights of every expert set, [16][4] fp32 (256 bytes), computed
// once per workgroup: with present bytes the set differs from row to row.
constexpr int DVS_AL_BYTES = (1 << NM_MAX_EXP) * NM_MAX_EXP * 4;      // 256
constexpr int DVS_SMEM = DVM_SMEM + DVS_AL_BYTES;
static_assert(2 * DVS_SMEM <= 160 * 1024, "two workgroups per CU");
static_assert((DVM_SMEM & 15) == 0, "alpha table alignment");
static_assert(NM_MAX_SUBSETS == (1 << NM_MAX_EXP) - 1, "every non-empty expert set");

// softmax_alpha over the experts of E alone (E = every expert: softmax_alpha itself, operation by operation)
__device__ __forceinline__ void dvs_softmax(const nm_job_t* J, unsigned E, float (&al)[NM_MAX_EXP]) {
#pragma clang fp contract(off)
  float mx = -INFINITY;
#pragma unroll
  for (int m = 0; m < NM_MAX_EXP; ++m)
    if ((E >> m) & 1u) mx = fmaxf(mx, asg(J->params)[J->mod[m].alpha]);
  float s = 0.f;
#pragma unroll
  for (int m = 0; m < NM_MAX_EXP; ++m) {
    al[m] = ((E >> m) & 1u) ? fx_exp(asg(J->params)[J->mod[m].alpha] - mx) : 0.f;
    s += al[m];
  }
  const float rs_ = fx_rcp(s);
#pragma unroll
  for (int m = 0; m < NM_MAX_EXP; ++m) al[m] *= rs_;
}
// fuse_fwd over the experts of E (non-empty) with nE = |E| in the place of M, without the single-expert bypass
__device__ __forceinline__ Fuse dvs_fuse(const nm_job_t* J, const Lat& L, const float (&al)[NM_MAX_EXP], unsigned E, float nE) {
#pragma clang fp contract(off)
  Fuse f;
  const int cb = J->combine;
  float S = 0.f, Smu = 0.f, sm = 0.f, sv = 0.f;
#pragma unroll
  for (int m = 0; m < NM_MAX_EXP; ++m) {
    if ((E >> m) & 1u) {
      float var = fx_exp(L.lv[m]);
      float w = (cb == NM_COMBINE_POE2V) ? fx_exp(-var) : ((cb == NM_COMBINE_GPOE) ? al[m] * fx_rcp(var) : fx_rcp(var));
      S += w; Smu += L.mu[m] * w;
      sm += L.mu[m]; sv += var;
    }
  }
  if (cb == NM_COMBINE_MOE) { f.mu = sm * fx_rcp(nE); f.var = sv * fx_rcp(nE); }
  else {
    f.var = fx_rcp(S); f.mu = Smu * f.var;
    if (cb == NM_COMBINE_MOPOE) { f.mu = (sm + f.mu) * fx_rcp(nE + 1.0f); f.var = (sv + f.var) * fx_rcp(nE + 1.0f); }
    if (cb == NM_COMBINE_POE2V) f.var = fx_log(fx_rcp(S));
  }
  if (J->var_floor > 0.f) f.var = fmaxf(f.var, J->var_floor);
  f.lv = fx_log(f.var);
  return f;
}

// dv_zero_dead_rows with the export pointers of one (entry, decoder)
__device__ __forceinline__ void dvs_zero_dead_rows(int tid, int xp, gf32 oloc, gf32 osq, gf32 ordv, int row0, int live) {
  const int r16 = rup(live, 16);
  for (int e = tid; e < (DV_ROWS - r16) * (xp >> 2); e += WG) {
    const int64_t gi = (int64_t)(row0 + r16) * xp + (int64_t)e * 4;
    if (oloc) *(GAS f32x4*)(oloc + gi) = f32x4{0.f, 0.f, 0.f, 0.f};
    if (osq) *(GAS f32x4*)(osq + gi) = f32x4{0.f, 0.f, 0.f, 0.f};
  }
  if (ordv)
    for (int r = live + tid; r < DV_ROWS; r += WG) ordv[row0 + r] = 0.f;
}

__global__ __launch_bounds__(WG, 4) void nm_devpass_subsets_kernel(const nm_job_t* __restrict__ jobs, const nm_subset_t* __restrict__ subsets,
                                                                     int n_subsets, int tile0, int flags) {
  constexpr int RT = DV_RT, ROWS = DV_ROWS;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const nm_job_t* J = jobs + blockIdx.x;
  if (dvm_refused(J) || !J->workspace || n_subsets < 1 || n_subsets > NM_MAX_SUBSETS) return;
  const nm_subset_t* const subs = subsets + (int64_t)blockIdx.x * n_subsets;
  const int M = J->M;
  const int t128 = tile0 + (int)blockIdx.y;
  const int row0 = t128 * ROWS;
  if (row0 >= J->n_rows) {
    // the second half of a ragged last 256-row tile: every entry's export rows come back as zeros
    if (row0 < (J->n_rows + TROWS - 1) / TROWS * TROWS)
      for (int s = 0; s < n_subsets; ++s)
        for (int m = 0; m < M; ++m)
          dvs_zero_dead_rows((int)threadIdx.x, J->mod[m].x_pitch, asg(subs[s].out_loc[m]), asg(subs[s].out_sqerr[m]), asg(subs[s].out_rowdev[m]), row0, 0);
    return;
  }
  Ctx c;
  c.job = J;
  c.part = -1; c.nparts = 1; c.lstep = 0;
  c.slope = J->act_slope;
  dv_carve(c, smem);
  relaunder(c);
  c.flags = NM_F_EXPORT | (flags & NM_F_TRACE);
  c.t_last = 0;
  c.ws = (GAS char*)J->workspace + (int64_t)(t128 / 2 - tile0 / 2) * J->workspace_stride;
  for (int i = c.tid; i < DVS_SMEM / 4; i += WG) reinterpret_cast<uint32_t*>(smem)[i] = 0u;
  __syncthreads();
  if (c.flags & 64) c.tlast[c.wave_s] = clock64();
  c.row0 = row0;
  c.rloc0 = row0 % TROWS;
  c.nrows = min(ROWS, J->n_rows - row0);
  c.inv_b = 1.0f / (float)c.nrows;
  const int live = c.nrows;
  const int step = row0 / TROWS;
  const int L = J->L, Z = J->Z, C = J->C;
  const int Zs = rup(Z, 16);
  const bool nl = J->non_linear != 0;
  const bool vec4 = (Z & 3) == 0;
  const unsigned all_m = (1u << M) - 1u;
  GAS char* const wsh = (GAS char*)J->wsh;
  char* const Wb = reinterpret_cast<char*>(c.Q);
  __bf16* const zlds = reinterpret_cast<__bf16*>(smem + DV_SMEM);
  float* const altab = reinterpret_cast<float*>(smem + DVM_SMEM);    // [16 expert sets][4]: gPoE weights (zeros otherwise)
  const WsLayout wl = ws_layout(M, L, Z);
  gf32 ws_mu_m = (gf32)(c.ws + wl.mu_m) + c.rloc0 * Zs;
  gf32 ws_lv_m = (gf32)(c.ws + wl.lv_m) + c.rloc0 * Zs;
  auto to_W = [&](const GAS char* blob, int vs, int rows, int K) {
    return Next{blob, Wb, IMG_BYTES >> 10, blob + cimg_bytes(rows, K), reinterpret_cast<char*>(c.vec) + vs * VEC_BYTES, rows, blob_kp(K)};
  };

  // ---- encoders: every expert's chain ONCE, statistics to the workspace ----
  for (int m = 0; m < M; ++m) {
    relaunder(c);
    const nm_modality_t& md = J->mod[m];
    const int nch = (md.Kx + XCH - 1) / XCH;
    const GAS char* after0 = wsh + (L > 1 ? md.enc_s[1] : md.heads_s);
    fwd_first_layer<RT>(c, (const GAS char*)asg(md.xb) + (int64_t)(row0 / TROWS) * nch * XIMG_TILE_BYTES + (int64_t)c.rloc0 * (LDX * 2),
                        md.Kx, wsh + md.enc_s[0], to_W(after0, 0, L > 1 ? J->H[1] : 2 * Zs, J->H[0]), J->H[0], nl, (gbf16)nullptr, true,
                        DV_W0_PIECES, live);
    int vs = 0;
    for (int e = 1; e < L; ++e) {
      const GAS char* nxt = wsh + (e + 1 < L ? md.enc_s[e + 1] : md.heads_s);
      dv_layer(c, vs, to_W(nxt, vs ^ 1, e + 1 < L ? J->H[e + 1] : 2 * Zs, J->H[e]), J->H[e], J->H[e - 1], nl, live);
      vs ^= 1;
    }
    tr(c, 1);
    wait_vm(0);
    fwd_heads<RT>(c, 0, no_next(), Z, J->H[L - 1], ws_mu_m + (int64_t)m * TROWS * Zs, ws_lv_m + (int64_t)m * TROWS * Zs, Zs, 0,
                  (__bf16*)nullptr, step, vec4, (float*)nullptr, c.vec + vs * (VEC_BYTES / 4));
  }
  // the gPoE weights of every expert set (thread t: set t; set 0 stays zeros), published by the barrier below
  if (J->combine == NM_COMBINE_GPOE && c.tid > 0 && c.tid <= (int)all_m) {
    float a4[NM_MAX_EXP];
    dvs_softmax(J, (unsigned)c.tid, a4);
#pragma unroll
    for (int m = 0; m < NM_MAX_EXP; ++m) altab[c.tid * NM_MAX_EXP + m] = a4[m];
  }
  handoff_barrier();                               // the heads' stores are complete for every thread of the workgroup

  // ---- the entries: fusion under the mask + the latent draw -> LDS, then the decoders the entry exports ----
  const int Hl = J->H[0];
  const int ob = L & 1;                            // (see nm_devpass_kernel: chunk 0's vectors avoid the last hidden layer's bias)
  for (int s = 0; s < n_subsets; ++s) {
    relaunder(c);
    const nm_subset_t& en = subs[s];
    const unsigned mask = en.mask & all_m;
    const GAS unsigned char* const pres = asg(en.present);
    int mf = -1;                                   // the first decoder this entry exports
    for (int m = M - 1; m >= 0; --m)
      if (en.out_loc[m] || en.out_sqerr[m] || en.out_rowdev[m]) mf = m;
    if (mf < 0) continue;                          // (workgroup-uniform)
    if (s > 0) lds_barrier();                      // the previous entry's last chunk is finished everywhere: P, W, vectors, Z free
    // W and P are free: the first decoder's image lands during the latent arithmetic
    issue_next(c, to_W(wsh + J->mod[mf].dec_s[0], 0, J->H[L - 1], Z + C));
    if (vec4) {
      const int nq4 = (Z + 3) >> 2;
      const float rq4 = 1.0f / (float)nq4;
#pragma unroll 1
      for (int e = c.tid; e < ROWS * nq4; e += WG) {
        const int r = idiv(e, nq4, rq4), z0 = 4 * (e - r * nq4);
        const unsigned E = (pres && r < live) ? (mask & (unsigned)pres[row0 + r]) : mask;
        const float nE = (float)__popc(E);
        float al[NM_MAX_EXP];
#pragma unroll
        for (int m = 0; m < NM_MAX_EXP; ++m) al[m] = altab[E * NM_MAX_EXP + m];
        f32x4 mu4[NM_MAX_EXP], lv4[NM_MAX_EXP];
#pragma unroll
        for (int m = 0; m < NM_MAX_EXP; ++m) {
          mu4[m] = f32x4{0.f, 0.f, 0.f, 0.f};
          lv4[m] = mu4[m];
          if (m < M) {
            mu4[m] = *(const GAS f32x4*)(ws_mu_m + ((int64_t)m * TROWS + r) * Zs + z0);
            lv4[m] = *(const GAS f32x4*)(ws_lv_m + ((int64_t)m * TROWS + r) * Zs + z0);
          }
        }
        float ep[4];
        if (J->eps) {
#pragma unroll
          for (int i = 0; i < 4; ++i) ep[i] = asg(J->eps)[((int64_t)(step % J->eps_cap) * TROWS + c.rloc0 + r) * Z + min(z0 + i, Z - 1)];
        } else {
          randn2_ctr(J->seed, (uint32_t)step, (uint32_t)(c.row0 + r), (uint32_t)(z0 >> 1), ep[0], ep[1]);
          randn2_ctr(J->seed, (uint32_t)step, (uint32_t)(c.row0 + r), (uint32_t)(z0 >> 1) + 1u, ep[2], ep[3]);
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) ep[i] = (z0 + i < Z) ? ep[i] : 0.f;
        bf16x4 zk;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          Lat Lt;
#pragma unroll
          for (int m = 0; m < NM_MAX_EXP; ++m) { Lt.mu[m] = mu4[m][i]; Lt.lv[m] = lv4[m][i]; }
          const Fuse f = dvs_fuse(J, Lt, al, E, nE);
          const float es = ep[i] * fx_exp(0.5f * f.lv);
          zk[i] = (__bf16)(E ? dvm_add(f.mu, es) : 0.f);
        }
        *reinterpret_cast<bf16x4*>(zlds + r * 32 + z0) = zk;
      }
    } else {
      const float rZ = 1.0f / (float)Z;
#pragma unroll 1
      for (int e = c.tid; e < ROWS * Z; e += WG) {
        const int r = idiv(e, Z, rZ), z = e - r * Z;
        const unsigned E = (pres && r < live) ? (mask & (unsigned)pres[row0 + r]) : mask;
        const float nE = (float)__popc(E);
        float al[NM_MAX_EXP];
#pragma unroll
        for (int m = 0; m < NM_MAX_EXP; ++m) al[m] = altab[E * NM_MAX_EXP + m];
        Lat Lt;
#pragma unroll
        for (int m = 0; m < NM_MAX_EXP; ++m) {
          Lt.mu[m] = (m < M) ? ws_mu_m[((int64_t)m * TROWS + r) * Zs + z] : 0.f;
          Lt.lv[m] = (m < M) ? ws_lv_m[((int64_t)m * TROWS + r) * Zs + z] : 0.f;
        }
        const Fuse f = dvs_fuse(J, Lt, al, E, nE);
        const float ep = J->eps ? asg(J->eps)[((int64_t)(step % J->eps_cap) * TROWS + c.rloc0 + r) * Z + z]
                                : randn_ctr(J->seed, (uint32_t)step, (uint32_t)(c.row0 + r), (uint32_t)z);
        const float es = ep * fx_exp(0.5f * f.lv);
        zlds[r * 32 + z] = (__bf16)(E ? dvm_add(f.mu, es) : 0.f);
      }
    }
    lds_barrier();                                 // z is complete (the decoder image requested above stays in flight)
    tr(c, 3);

    for (int m = mf; m < M; ++m) {
      relaunder(c);
      const gf32 oloc = asg(en.out_loc[m]), osq = asg(en.out_sqerr[m]), ordv = asg(en.out_rowdev[m]);
      if (!oloc && !osq && !ordv) continue;        // (workgroup-uniform) nothing of this decoder is wanted: skipped entirely
      const nm_modality_t& md = J->mod[m];
      const int D = md.D;
      if (m != mf) {
        lds_barrier();                             // the previous decoder's last chunk is finished everywhere: P, W, vectors free
        issue_next(c, to_W(wsh + md.dec_s[0], 0, J->H[L - 1], Z + C));
      }
      build_zc<RT>(c, c.P, md, (gcf32)nullptr, (gcf32)nullptr, Z, C, Zs, 0, (gcf32)nullptr, zlds);
      tr(c, 4);
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
        dv_layer(c, vs, nx, Nout, Kin, nl, live);    // (its first barrier also publishes z | c | 1)
        vs ^= 1;
      }
      tr(c, 5);
      // output layer in 64-ROI chunks, wave w owns rows [16 w, 16 w + 16) and all 64 columns: see nm_devpass_kernel
      gcf32 xf = asg(md.x_f32);
      const int xp = md.x_pitch;
      float rdev = 0.f;
      const int orow = c.wave * 16 + c.c16;
      const bool wave_live = c.wave * 16 < live;
      const bool rv = orow < c.nrows;
      // this lane's row: its observed experts (read once), whether anything was fused, whether x of this modality is real
      const unsigned prow = (pres && rv) ? (unsigned)pres[row0 + orow] : all_m;
      const bool none = (mask & prow) == 0u;
      const bool xmiss = none || ((prow >> m) & 1u) == 0u;
      const float qnan = __builtin_nanf("");
      auto load_xin = [&](int chx, f32x4 (&xv)[4]) {
#pragma unroll
        for (int ft = 0; ft < 4; ++ft) {
          const int dcl = min(chx * OCH + ft * 16 + 4 * c.g, xp - 4);
          xv[ft] = *(const GAS f32x4*)(xf + (int64_t)(row0 + orow) * xp + dcl);
        }
      };
      int stores_prev = 0;
      auto chunk = [&](const int ch, f32x4 (&xin)[4], f32x4 (&xnx)[4]) {
        relaunder(c);
        const int d0 = ch * OCH;
        const __bf16* Wc = reinterpret_cast<const __bf16*>(Wb + (ch & 1) * OIMG_BYTES);
        const float* vb = c.vec + ((ch + ob) & 1) * (VEC_BYTES / 4);
        wait_vm(ch > 0 ? stores_prev : 0);
        lds_barrier();
        if (ch + 1 < nck) { issue_next(c, out_blob(ch + 1)); if (wave_live) load_xin(ch + 1, xnx); }
        stores_prev = 0;
        if (!wave_live) return;
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
        tr(c, 6);
        const bool full = live == ROWS && d0 + OCH <= D && !pres;         // no row / column / presence masks needed (wave-uniform)
#pragma unroll
        for (int ft = 0; ft < 4; ++ft) {
          const int dg0 = d0 + ft * 16 + 4 * c.g;
          const f32x4 bo = *reinterpret_cast<const f32x4*>(vb + ft * 16 + 4 * c.g);
          f32x4 lo, sq;
          if (full) {
            lo = acc[ft] + bo;
            const f32x4 diff = lo - xin[ft];
            sq = diff * diff;
          } else {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
              const float xh = acc[ft][i] + bo[i];
              const bool dv = rv && dg0 + i < D;
              const float diff = xh - xin[ft][i];
              lo[i] = dv ? (none ? qnan : xh) : 0.f;
              sq[i] = dv ? (xmiss ? qnan : diff * diff) : 0.f;
            }
          }
          rdev += ((sq[0] + sq[1]) + sq[2]) + sq[3];
          if (d0 + ft * 16 < xp) {                      // wave-uniform
            if (dg0 < xp) {
              const int64_t gi = (int64_t)(row0 + orow) * xp + dg0;
              if (oloc) *(GAS f32x4*)(oloc + gi) = lo;
              if (osq) *(GAS f32x4*)(osq + gi) = sq;
            }
            stores_prev += (oloc ? 1 : 0) + (osq ? 1 : 0);
          }
        }
        tr(c, 7);
      };
      {
        f32x4 xa[4], xb[4];
        if (wave_live) load_xin(0, xa);
        for (int ch = 0; ch < nck; ch += 2) {
          chunk(ch, xa, xb);
          if (ch + 1 < nck) chunk(ch + 1, xb, xa);
        }
      }
      if (ordv && wave_live) {
        float v = rdev;
        v += __shfl_xor(v, 16, 64);
        v += __shfl_xor(v, 32, 64);
        if (c.g == 0 && orow < c.nrows) ordv[row0 + orow] = v / (float)D;
      }
      // (a ragged tile only: the rows no wave has stored; the laundered thread index keeps the loop's addresses from being
      //  hoisted out of the entry loop and held in registers across it)
      if (live < ROWS) { relaunder(c); dvs_zero_dead_rows(c.tid, xp, oloc, osq, ordv, row0, live); }
      tr(c, 8);
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// nm_latent_kernel -- the encoder half of the pass above and nothing else: the joint posterior (mu, logvar) of every row,
// what cVAE.pred_latent returns (cVAE.py:539-545) and latent_deviation / separate_latent_deviation score against the
// training cohort (utils_vae.py:155-161).  No latent draw, no z | c | 1, no decoder, no output chunks.
//
// A workgroup owns 128 rows, two workgroups share a CU (LDS: P, W, the two vector slots and the scalars of nm_devpass_kernel,
// 75 KB; no z buffer).  Per tile: every expert's encoder chain (first layer, dv_layer, heads), then the fusion.
//   several experts: the heads store mu_m / logvar_m to this tile's rows of the batch's workspace tile, and the fusion reads
//     them back through fuse_fwd / softmax_alpha exactly as nm_devpass_multi_kernel and the general kernel do;
//   one expert (SM models, cVAE): the heads' accumulators go through the same fuse_fwd (its single-expert bypass, or the
//     one-expert product with the prior where the job has the bypass off) straight to the exports: no workspace tile.
// out_mu / out_logvar agree bit for bit with the general kernel's exports on the table's rows; the rows of the launch's
// 128-row tiles past the table's end -- the empty half of a ragged 256-row batch included -- come back as zeros.
// A job lat_refused refuses must not reach this kernel; its workgroups leave at once, exports untouched.
__host__ __device__ inline int lat_refused(const nm_job_t* j) {
  const int Me = j->M_enc > 0 ? j->M_enc : j->M;
  if (j->wide || j->M < 1 || j->M > NM_MAX_EXP || Me != j->M) return NM_E_DEVPASS;
  if (j->n_private != 0 || j->tc_weight != 0.f || j->w_off >= 0 || j->out_kind != 0) return NM_E_DEVPASS;
  if (j->H[0] > DV_MAX_H0 || rup(j->Z, 16) > 32) return NM_E_DEVPASS;
  return 0;
}

// One expert: the heads GEMM of fwd_heads (same fragments, same order of accumulation), its epilogue the fusion of that
// one expert and the export.  Lane (c16, g) of a unit holds row r, latent columns f0 .. f0 + 3.
__device__ __forceinline__ void lat_heads_export(const Ctx& cc, int Z, int K, int Zs, bool vec4, const float (&alpha)[NM_MAX_EXP],
                                                 const float* bias) {
  constexpr int RT = DV_RT, WROWS = DV_RT * 16;
  Ctx c = cc;
  relaunder(c);
  const nm_job_t* J = c.job;
  const int ksteps = wpad(K) / 32;
  const int nzt = Zs / 16;
  const __bf16* Wt = c.Q;
  gf32 omu = asg(J->out_mu), olv = asg(J->out_logvar);
  wait_vm(0);
  lds_barrier();
  for (int u = c.wn; u < nzt * RT; u += NWN) {
    const int ft = u / RT, rt = u - ft * RT;
    const int f0 = ft * 16 + 4 * c.g;
    f32x4 am = {0.f, 0.f, 0.f, 0.f}, al = am;
    for (int ks = 0; ks < ksteps; ++ks) {
      const bf16x8 fm = lds_frag(Wt, LDP, ft * 16 + c.c16, ks * 32 + 8 * c.g);
      const bf16x8 fl = lds_frag(Wt, LDP, Zs + ft * 16 + c.c16, ks * 32 + 8 * c.g);
      const bf16x8 a = lds_frag(c.P, LDP, c.wm * WROWS + rt * 16 + c.c16, ks * 32 + 8 * c.g);
      am = mfma(fm, a, am);
      al = mfma(fl, a, al);
    }
    const int r = c.wm * WROWS + rt * 16 + c.c16;
    am += *reinterpret_cast<const f32x4*>(bias + f0);
    al += *reinterpret_cast<const f32x4*>(bias + Zs + f0);
    const bool rv = r < c.nrows;
    f32x4 jm, jl;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      Lat Lt;
#pragma unroll
      for (int m = 0; m < NM_MAX_EXP; ++m) { Lt.mu[m] = 0.f; Lt.lv[m] = 0.f; }
      Lt.mu[0] = am[i]; Lt.lv[0] = al[i];
      const Fuse f = fuse_fwd(J, Lt, alpha);
      jm[i] = rv ? f.mu : 0.f;
      jl[i] = rv ? f.lv : 0.f;
    }
    const int64_t gr = (int64_t)(c.row0 + r) * Z + f0;
    if (vec4) {
      if (f0 < Z) {
        if (omu) *(GAS f32x4*)(omu + gr) = jm;
        if (olv) *(GAS f32x4*)(olv + gr) = jl;
      }
    } else {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        if (f0 + i < Z) {
          if (omu) omu[gr + i] = jm[i];
          if (olv) olv[gr + i] = jl[i];
        }
      }
    }
  }
  lds_barrier();
  tr(c, 2);
}

__global__ __launch_bounds__(WG, 4) void nm_latent_kernel(const nm_job_t* __restrict__ jobs, int tile0, int flags) {
  constexpr int RT = DV_RT, ROWS = DV_ROWS;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const nm_job_t* J = jobs + blockIdx.x;
  const int M = J->M;
  if (lat_refused(J) || (M > 1 && !J->workspace)) return;
  const int Z = J->Z;
  const int t128 = tile0 + (int)blockIdx.y;
  const int row0 = t128 * ROWS;
  gf32 omu = asg(J->out_mu), olv = asg(J->out_logvar);
  if (row0 >= J->n_rows) {
    // the second half of a ragged last 256-row tile: its export rows come back as zeros ([128][Z] floats: whole 16-byte words)
    if (row0 < (J->n_rows + TROWS - 1) / TROWS * TROWS) {
      for (int e = threadIdx.x; e < ROWS * Z / 4; e += WG) {
        const int64_t gi = (int64_t)row0 * Z + (int64_t)e * 4;
        if (omu) *(GAS f32x4*)(omu + gi) = f32x4{0.f, 0.f, 0.f, 0.f};
        if (olv) *(GAS f32x4*)(olv + gi) = f32x4{0.f, 0.f, 0.f, 0.f};
      }
    }
    return;
  }
  Ctx c;
  c.job = J;
  c.part = -1; c.nparts = 1; c.lstep = 0;
  c.slope = J->act_slope;
  dv_carve(c, smem);
  relaunder(c);
  c.flags = NM_F_EXPORT | (flags & NM_F_TRACE);
  c.t_last = 0;
  // several experts: the workspace tile of this tile's 256-row batch (counted from the batch tile0 falls in)
  c.ws = M > 1 ? (GAS char*)J->workspace + (int64_t)(t128 / 2 - tile0 / 2) * J->workspace_stride : nullptr;
  for (int i = c.tid; i < DV_SMEM / 4; i += WG) reinterpret_cast<uint32_t*>(smem)[i] = 0u;
  __syncthreads();
  if (c.flags & 64) c.tlast[c.wave_s] = clock64();
  c.row0 = row0;
  c.rloc0 = row0 % TROWS;
  c.nrows = min(ROWS, J->n_rows - row0);
  c.inv_b = 1.0f / (float)c.nrows;
  const int live = c.nrows;
  const int L = J->L;
  const int Zs = rup(Z, 16);
  const bool nl = J->non_linear != 0;
  const bool vec4 = (Z & 3) == 0;
  GAS char* const wsh = (GAS char*)J->wsh;
  char* const Wb = reinterpret_cast<char*>(c.Q);
  const WsLayout wl = ws_layout(M, L, Z);
  gf32 ws_mu_m = (gf32)(c.ws + wl.mu_m) + c.rloc0 * Zs;
  gf32 ws_lv_m = (gf32)(c.ws + wl.lv_m) + c.rloc0 * Zs;
  auto to_W = [&](const GAS char* blob, int vs, int rows, int K) {
    return Next{blob, Wb, IMG_BYTES >> 10, blob + cimg_bytes(rows, K), reinterpret_cast<char*>(c.vec) + vs * VEC_BYTES, rows, blob_kp(K)};
  };
  float al[NM_MAX_EXP] = {0.f, 0.f, 0.f, 0.f};
  if (J->combine == NM_COMBINE_GPOE && !(M == 1 && J->single_bypass)) softmax_alpha(J, al);

  // ---- encoders: every expert's chain ----
  for (int m = 0; m < M; ++m) {
    relaunder(c);
    const nm_modality_t& md = J->mod[m];
    const int nch = (md.Kx + XCH - 1) / XCH;
    const GAS char* after0 = wsh + (L > 1 ? md.enc_s[1] : md.heads_s);
    fwd_first_layer<RT>(c, (const GAS char*)asg(md.xb) + (int64_t)(row0 / TROWS) * nch * XIMG_TILE_BYTES + (int64_t)c.rloc0 * (LDX * 2),
                        md.Kx, wsh + md.enc_s[0], to_W(after0, 0, L > 1 ? J->H[1] : 2 * Zs, J->H[0]), J->H[0], nl, (gbf16)nullptr, true,
                        DV_W0_PIECES, live);
    int vs = 0;
    for (int e = 1; e < L; ++e) {
      const GAS char* nxt = wsh + (e + 1 < L ? md.enc_s[e + 1] : md.heads_s);
      dv_layer(c, vs, to_W(nxt, vs ^ 1, e + 1 < L ? J->H[e + 1] : 2 * Zs, J->H[e]), J->H[e], J->H[e - 1], nl, live);
      vs ^= 1;
    }
    tr(c, 1);
    if (M == 1) {
      lat_heads_export(c, Z, J->H[L - 1], Zs, vec4, al, c.vec + vs * (VEC_BYTES / 4));
      return;
    }
    wait_vm(0);
    fwd_heads<RT>(c, 0, no_next(), Z, J->H[L - 1], ws_mu_m + (int64_t)m * TROWS * Zs, ws_lv_m + (int64_t)m * TROWS * Zs, Zs, 0,
                  (__bf16*)nullptr, 0, vec4, (float*)nullptr, c.vec + vs * (VEC_BYTES / 4));
  }

  // ---- fusion: the joint statistics to the exports ----
  handoff_barrier();                               // the heads' stores are complete for every thread of the workgroup
  relaunder(c);
  if (vec4) {
    const int nq4 = Z >> 2;
    const float rq4 = 1.0f / (float)nq4;
#pragma unroll 2
    for (int e = c.tid; e < ROWS * nq4; e += WG) {
      const int r = idiv(e, nq4, rq4), z0 = 4 * (e - r * nq4);
      f32x4 jm = {0.f, 0.f, 0.f, 0.f}, jl = jm;
      if (r < live) {
        f32x4 mu4[NM_MAX_EXP], lv4[NM_MAX_EXP];
#pragma unroll
        for (int m = 0; m < NM_MAX_EXP; ++m) {
          mu4[m] = f32x4{0.f, 0.f, 0.f, 0.f};
          lv4[m] = mu4[m];
          if (m < M) {
            mu4[m] = *(const GAS f32x4*)(ws_mu_m + ((int64_t)m * TROWS + r) * Zs + z0);
            lv4[m] = *(const GAS f32x4*)(ws_lv_m + ((int64_t)m * TROWS + r) * Zs + z0);
          }
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          Lat Lt;
#pragma unroll
          for (int m = 0; m < NM_MAX_EXP; ++m) { Lt.mu[m] = mu4[m][i]; Lt.lv[m] = lv4[m][i]; }
          const Fuse f = fuse_fwd(J, Lt, al);
          jm[i] = f.mu; jl[i] = f.lv;
        }
      }
      const int64_t gr = (int64_t)(row0 + r) * Z + z0;
      if (omu) *(GAS f32x4*)(omu + gr) = jm;
      if (olv) *(GAS f32x4*)(olv + gr) = jl;
    }
  } else {
    const float rZ = 1.0f / (float)Z;
#pragma unroll 2
    for (int e = c.tid; e < ROWS * Z; e += WG) {
      const int r = idiv(e, Z, rZ), z = e - r * Z;
      float jm = 0.f, jl = 0.f;
      if (r < live) {
        Lat Lt;
#pragma unroll
        for (int m = 0; m < NM_MAX_EXP; ++m) {
          Lt.mu[m] = (m < M) ? ws_mu_m[((int64_t)m * TROWS + r) * Zs + z] : 0.f;
          Lt.lv[m] = (m < M) ? ws_lv_m[((int64_t)m * TROWS + r) * Zs + z] : 0.f;
        }
        const Fuse f = fuse_fwd(J, Lt, al);
        jm = f.mu; jl = f.lv;
      }
      const int64_t gr = (int64_t)(row0 + r) * Z + z;
      if (omu) omu[gr] = jm;
      if (olv) olv[gr] = jl;
    }
  }
  tr(c, 3);
}

// ---------------------------------------------------------------------------------------------------------------------
// nm_devpass_draws_kernel -- the posterior-predictive pass: nm_devpass_subsets_kernel's shape with the loop over DRAWS in
// the place of the loop over subsets, and the statistics of the S reconstructions folded in the output epilogue (nmhip.h
// states the definition).  Encoders once per tile, statistics to the workspace tile; then per draw s the fusion (the same
// fuse_fwd / softmax_alpha every time: the posterior does not depend on s), the draw under (seed_s | eps_s) and every
// decoder that is wanted.  The sources of the kernels above stay as they are: their decoder loop is repeated here with the
// fold in the place of the export stores.
//
// One expert: the heads' statistics go through the workspace like several experts' and through fuse_fwd with the job's
// single_bypass (as nm_latent_kernel does); with the bypass the draw is fwd_heads' expression (nm_devpass_kernel is the
// pass such a job otherwise runs on), without it the general kernel's separate addition (dvm_add) as for several experts.
//
// Accumulators: mean and M2 of an element live in pred_mean / pred_var between the draws.  The output phase's ownership
// (wave w: rows 16 w .. 16 w + 15, lane: four columns of a feature tile) does not depend on s, so an element is loaded and
// stored by ONE lane, with plain loads and stores; draw 0 stores without loading, the last draw finalises in registers.
// The chunk boundary takes a full wait (wait_vm(0)): the accumulator loads are vector-memory operations of their own, a
// count of the previous chunk's stores would no longer mean what it means in the kernels above.
//
// Geometry, LDS plan (P, W, vector slots, scalars, Z [128][32] bf16) and workspace tile: nm_devpass_multi_kernel's.
constexpr int DVD_SMEM = DVM_SMEM;
static_assert(2 * DVD_SMEM <= 160 * 1024, "two workgroups per CU");

__host__ __device__ inline int dvd_refused(const nm_job_t* j) { return lat_refused(j); }   // 1..NM_MAX_EXP experts, the compact shapes

// fwd_heads' in-register draw of a one-expert job (zdst path), written as it is written there
__device__ __forceinline__ float dvd_z_bypass(float mu, float ep, float lv) { return mu + ep * fx_exp(0.5f * lv); }

// one step of the fold (s >= 1): rs = 1 / (s + 1)
__device__ __forceinline__ void dvd_fold(float xh, float rs, float& mean, float& m2) {
#pragma clang fp contract(off)
  const float d = xh - mean;
  mean = mean + d * rs;
  m2 = m2 + d * (xh - mean);
}
// the exports of one element from its final (mean, M2): v = 1 / (S - 1) (S = 1: 0), cf = (S - 1) / S
__device__ __forceinline__ void dvd_final(float x, float mean, float m2, float v, float cf, float nv, float& var, float& msq, float& z) {
#pragma clang fp contract(off)
  var = m2 * v;
  const float e = x - mean;
  msq = e * e + var * cf;
  z = e / sqrtf(nv + var);
}
__device__ __forceinline__ float dvd_sum4(const f32x4& a) {
#pragma clang fp contract(off)
  return ((a[0] + a[1]) + a[2]) + a[3];
}
__device__ __forceinline__ float dvd_sumsq4(const f32x4& a) {
#pragma clang fp contract(off)
  return ((a[0] * a[0] + a[1] * a[1]) + a[2] * a[2]) + a[3] * a[3];
}

struct DvdOut { gf32 mean, var, msq, z, rdev, rz2; gcf32 nv; };
__device__ __forceinline__ DvdOut dvd_out(const nm_pred_t& p, int m) {
  DvdOut o;
  o.mean = asg(p.pred_mean[m]); o.var = asg(p.pred_var[m]);
  const bool on = o.mean && o.var;                  // (both accumulators, or the decoder is skipped)
  o.nv = on ? asg(p.noise_var[m]) : nullptr;
  o.msq = on ? asg(p.pred_msq[m]) : nullptr;
  o.z = (on && o.nv) ? asg(p.pred_z[m]) : nullptr;
  o.rdev = on ? asg(p.pred_rowdev[m]) : nullptr;
  o.rz2 = (on && o.nv) ? asg(p.pred_rowz2[m]) : nullptr;
  if (!on) { o.mean = nullptr; o.var = nullptr; }
  return o;
}
// dv_zero_dead_rows with the export pointers of one decoder's predictive exports
__device__ __forceinline__ void dvd_zero_dead_rows(int tid, int xp, const DvdOut& o, int row0, int live) {
  if (!o.mean) return;
  const int r16 = rup(live, 16);
  for (int e = tid; e < (DV_ROWS - r16) * (xp >> 2); e += WG) {
    const int64_t gi = (int64_t)(row0 + r16) * xp + (int64_t)e * 4;
    *(GAS f32x4*)(o.mean + gi) = f32x4{0.f, 0.f, 0.f, 0.f};
    *(GAS f32x4*)(o.var + gi) = f32x4{0.f, 0.f, 0.f, 0.f};
    if (o.msq) *(GAS f32x4*)(o.msq + gi) = f32x4{0.f, 0.f, 0.f, 0.f};
    if (o.z) *(GAS f32x4*)(o.z + gi) = f32x4{0.f, 0.f, 0.f, 0.f};
  }
  for (int r = live + tid; r < DV_ROWS; r += WG) {
    if (o.rdev) o.rdev[row0 + r] = 0.f;
    if (o.rz2) o.rz2[row0 + r] = 0.f;
  }
}

__global__ __launch_bounds__(WG, 4) void nm_devpass_draws_kernel(const nm_job_t* __restrict__ jobs, const nm_draw_t* __restrict__ draws,
                                                                   int n_draws, const nm_pred_t* __restrict__ preds, int tile0, int flags) {
  constexpr int RT = DV_RT, ROWS = DV_ROWS;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const nm_job_t* J = jobs + blockIdx.x;
  if (dvd_refused(J) || !J->workspace || n_draws < 1 || n_draws > NM_MAX_DRAWS) return;
  const nm_draw_t* const drs = draws + (int64_t)blockIdx.x * n_draws;
  const nm_pred_t& pr = preds[blockIdx.x];
  const int M = J->M;
  const int t128 = tile0 + (int)blockIdx.y;
  const int row0 = t128 * ROWS;
  if (row0 >= J->n_rows) {
    // the second half of a ragged last 256-row tile: every decoder's export rows come back as zeros
    if (row0 < (J->n_rows + TROWS - 1) / TROWS * TROWS)
      for (int m = 0; m < M; ++m) dvd_zero_dead_rows((int)threadIdx.x, J->mod[m].x_pitch, dvd_out(pr, m), row0, 0);
    return;
  }
  int mf = -1;                                     // the first decoder that is wanted
  for (int m = M - 1; m >= 0; --m)
    if (pr.pred_mean[m] && pr.pred_var[m]) mf = m;
  if (mf < 0) return;                              // (workgroup-uniform)
  Ctx c;
  c.job = J;
  c.part = -1; c.nparts = 1; c.lstep = 0;
  c.slope = J->act_slope;
  dv_carve(c, smem);
  relaunder(c);
  c.flags = NM_F_EXPORT | (flags & NM_F_TRACE);
  c.t_last = 0;
  c.ws = (GAS char*)J->workspace + (int64_t)(t128 / 2 - tile0 / 2) * J->workspace_stride;
  for (int i = c.tid; i < DVD_SMEM / 4; i += WG) reinterpret_cast<uint32_t*>(smem)[i] = 0u;
  __syncthreads();
  if (c.flags & 64) c.tlast[c.wave_s] = clock64();
  c.row0 = row0;
  c.rloc0 = row0 % TROWS;
  c.nrows = min(ROWS, J->n_rows - row0);
  c.inv_b = 1.0f / (float)c.nrows;
  const int live = c.nrows;
  const int step = row0 / TROWS;
  const int L = J->L, Z = J->Z, C = J->C;
  const int Zs = rup(Z, 16);
  const bool nl = J->non_linear != 0;
  const bool vec4 = (Z & 3) == 0;
  const bool byp = M == 1 && J->single_bypass != 0;
  GAS char* const wsh = (GAS char*)J->wsh;
  char* const Wb = reinterpret_cast<char*>(c.Q);
  __bf16* const zlds = reinterpret_cast<__bf16*>(smem + DV_SMEM);
  const WsLayout wl = ws_layout(M, L, Z);
  gf32 ws_mu_m = (gf32)(c.ws + wl.mu_m) + c.rloc0 * Zs;
  gf32 ws_lv_m = (gf32)(c.ws + wl.lv_m) + c.rloc0 * Zs;
  auto to_W = [&](const GAS char* blob, int vs, int rows, int K) {
    return Next{blob, Wb, IMG_BYTES >> 10, blob + cimg_bytes(rows, K), reinterpret_cast<char*>(c.vec) + vs * VEC_BYTES, rows, blob_kp(K)};
  };

  // ---- encoders: every expert's chain ONCE, statistics to the workspace ----
  for (int m = 0; m < M; ++m) {
    relaunder(c);
    const nm_modality_t& md = J->mod[m];
    const int nch = (md.Kx + XCH - 1) / XCH;
    const GAS char* after0 = wsh + (L > 1 ? md.enc_s[1] : md.heads_s);
    fwd_first_layer<RT>(c, (const GAS char*)asg(md.xb) + (int64_t)(row0 / TROWS) * nch * XIMG_TILE_BYTES + (int64_t)c.rloc0 * (LDX * 2),
                        md.Kx, wsh + md.enc_s[0], to_W(after0, 0, L > 1 ? J->H[1] : 2 * Zs, J->H[0]), J->H[0], nl, (gbf16)nullptr, true,
                        DV_W0_PIECES, live);
    int vs = 0;
    for (int e = 1; e < L; ++e) {
      const GAS char* nxt = wsh + (e + 1 < L ? md.enc_s[e + 1] : md.heads_s);
      dv_layer(c, vs, to_W(nxt, vs ^ 1, e + 1 < L ? J->H[e + 1] : 2 * Zs, J->H[e]), J->H[e], J->H[e - 1], nl, live);
      vs ^= 1;
    }
    tr(c, 1);
    wait_vm(0);
    fwd_heads<RT>(c, 0, no_next(), Z, J->H[L - 1], ws_mu_m + (int64_t)m * TROWS * Zs, ws_lv_m + (int64_t)m * TROWS * Zs, Zs, 0,
                  (__bf16*)nullptr, step, vec4, (float*)nullptr, c.vec + vs * (VEC_BYTES / 4));
  }
  handoff_barrier();                               // the heads' stores are complete for every thread of the workgroup

  // ---- the draws: fusion + draw s -> LDS, then every wanted decoder with the fold in its output epilogue ----
  const int Hl = J->H[0];
  const int ob = L & 1;                            // (see nm_devpass_kernel: chunk 0's vectors avoid the last hidden layer's bias)
  const float vS = n_draws > 1 ? 1.0f / (float)(n_draws - 1) : 0.f;
  const float cS = (float)(n_draws - 1) / (float)n_draws;
  for (int s = 0; s < n_draws; ++s) {
    relaunder(c);
    const uint64_t seed = drs[s].seed;
    const GAS float* const epsp = asg(drs[s].eps);
    const bool first = s == 0, last = s == n_draws - 1;
    const float rs = 1.0f / (float)(s + 1);
    if (s > 0) lds_barrier();                      // the previous draw's last chunk is finished everywhere: P, W, vectors, Z free
    // W and P are free: the first decoder's image lands during the latent arithmetic
    issue_next(c, to_W(wsh + J->mod[mf].dec_s[0], 0, J->H[L - 1], Z + C));
    {
      float al[NM_MAX_EXP] = {0.f, 0.f, 0.f, 0.f};
      if (J->combine == NM_COMBINE_GPOE && !byp) softmax_alpha(J, al);
      relaunder(c);
      if (vec4) {
        const int nq4 = (Z + 3) >> 2;
        const float rq4 = 1.0f / (float)nq4;
#pragma unroll 1
        for (int e = c.tid; e < ROWS * nq4; e += WG) {
          const int r = idiv(e, nq4, rq4), z0 = 4 * (e - r * nq4);
          f32x4 mu4[NM_MAX_EXP], lv4[NM_MAX_EXP];
#pragma unroll
          for (int m = 0; m < NM_MAX_EXP; ++m) {
            mu4[m] = f32x4{0.f, 0.f, 0.f, 0.f};
            lv4[m] = mu4[m];
            if (m < M) {
              mu4[m] = *(const GAS f32x4*)(ws_mu_m + ((int64_t)m * TROWS + r) * Zs + z0);
              lv4[m] = *(const GAS f32x4*)(ws_lv_m + ((int64_t)m * TROWS + r) * Zs + z0);
            }
          }
          float ep[4];
          if (epsp) {
#pragma unroll
            for (int i = 0; i < 4; ++i) ep[i] = epsp[((int64_t)(step % J->eps_cap) * TROWS + c.rloc0 + r) * Z + min(z0 + i, Z - 1)];
          } else {
            randn2_ctr(seed, (uint32_t)step, (uint32_t)(c.row0 + r), (uint32_t)(z0 >> 1), ep[0], ep[1]);
            randn2_ctr(seed, (uint32_t)step, (uint32_t)(c.row0 + r), (uint32_t)(z0 >> 1) + 1u, ep[2], ep[3]);
          }
#pragma unroll
          for (int i = 0; i < 4; ++i) ep[i] = (z0 + i < Z) ? ep[i] : 0.f;
          bf16x4 zk;
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            Lat Lt;
#pragma unroll
            for (int m = 0; m < NM_MAX_EXP; ++m) { Lt.mu[m] = mu4[m][i]; Lt.lv[m] = lv4[m][i]; }
            const Fuse f = fuse_fwd(J, Lt, al);
            if (byp) {
              zk[i] = (__bf16)((z0 + i < Z) ? dvd_z_bypass(f.mu, ep[i], f.lv) : 0.f);
            } else {
              const float es = ep[i] * fx_exp(0.5f * f.lv);
              zk[i] = (__bf16)dvm_add(f.mu, es);
            }
          }
          *reinterpret_cast<bf16x4*>(zlds + r * 32 + z0) = zk;
        }
      } else {
        const float rZ = 1.0f / (float)Z;
#pragma unroll 1
        for (int e = c.tid; e < ROWS * Z; e += WG) {
          const int r = idiv(e, Z, rZ), z = e - r * Z;
          Lat Lt;
#pragma unroll
          for (int m = 0; m < NM_MAX_EXP; ++m) {
            Lt.mu[m] = (m < M) ? ws_mu_m[((int64_t)m * TROWS + r) * Zs + z] : 0.f;
            Lt.lv[m] = (m < M) ? ws_lv_m[((int64_t)m * TROWS + r) * Zs + z] : 0.f;
          }
          const Fuse f = fuse_fwd(J, Lt, al);
          const float ep = epsp ? epsp[((int64_t)(step % J->eps_cap) * TROWS + c.rloc0 + r) * Z + z]
                                : randn_ctr(seed, (uint32_t)step, (uint32_t)(c.row0 + r), (uint32_t)z);
          if (byp) {
            zlds[r * 32 + z] = (__bf16)dvd_z_bypass(f.mu, ep, f.lv);
          } else {
            const float es = ep * fx_exp(0.5f * f.lv);
            zlds[r * 32 + z] = (__bf16)dvm_add(f.mu, es);
          }
        }
      }
    }
    lds_barrier();                                 // z is complete (the decoder image requested above stays in flight)
    tr(c, 3);

    for (int m = mf; m < M; ++m) {
      relaunder(c);
      const DvdOut o = dvd_out(pr, m);
      if (!o.mean) continue;                       // (workgroup-uniform) this decoder is not wanted: skipped entirely
      const nm_modality_t& md = J->mod[m];
      const int D = md.D;
      if (m != mf) {
        lds_barrier();                             // the previous decoder's last chunk is finished everywhere: P, W, vectors free
        issue_next(c, to_W(wsh + md.dec_s[0], 0, J->H[L - 1], Z + C));
      }
      build_zc<RT>(c, c.P, md, (gcf32)nullptr, (gcf32)nullptr, Z, C, Zs, 0, (gcf32)nullptr, zlds);
      tr(c, 4);
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
        dv_layer(c, vs, nx, Nout, Kin, nl, live);    // (its first barrier also publishes z | c | 1)
        vs ^= 1;
      }
      tr(c, 5);
      // output layer in 64-ROI chunks, wave w owns rows [16 w, 16 w + 16) and all 64 columns: see nm_devpass_kernel
      gcf32 xf = asg(md.x_f32);
      const int xp = md.x_pitch;
      float rdev = 0.f, rz2 = 0.f;
      const int orow = c.wave * 16 + c.c16;
      const bool wave_live = c.wave * 16 < live;
      const bool rv = orow < c.nrows;
      auto load_xin = [&](int chx, f32x4 (&xv)[4]) {
#pragma unroll
        for (int ft = 0; ft < 4; ++ft) {
          const int dcl = min(chx * OCH + ft * 16 + 4 * c.g, xp - 4);
          xv[ft] = *(const GAS f32x4*)(xf + (int64_t)(row0 + orow) * xp + dcl);
        }
      };
      auto chunk = [&](const int ch, f32x4 (&xin)[4], f32x4 (&xnx)[4]) {
        relaunder(c);
        const int d0 = ch * OCH;
        const __bf16* Wc = reinterpret_cast<const __bf16*>(Wb + (ch & 1) * OIMG_BYTES);
        const float* vb = c.vec + ((ch + ob) & 1) * (VEC_BYTES / 4);
        // chunk ch's rows, vectors and inputs have landed, and everything else this wave has in flight with them: the
        // accumulator loads and stores of the previous chunk are counted in the same queue (a full wait, not a count)
        wait_vm(0);
        lds_barrier();
        if (ch + 1 < nck) { issue_next(c, out_blob(ch + 1)); if (wave_live && last) load_xin(ch + 1, xnx); }
        if (!wave_live) return;
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
        tr(c, 6);
#pragma unroll
        for (int ft = 0; ft < 4; ++ft) {
          const int dg0 = d0 + ft * 16 + 4 * c.g;
          const f32x4 bo = *reinterpret_cast<const f32x4*>(vb + ft * 16 + 4 * c.g);
          if (d0 + ft * 16 < xp && dg0 < xp) {          // (the first: wave-uniform) whole tiles are stored, zeros past the table's end
            const int64_t gi = (int64_t)(row0 + orow) * xp + dg0;
            f32x4 mn, m2;
            if (first) {
#pragma unroll
              for (int i = 0; i < 4; ++i) {
                const float xh = acc[ft][i] + bo[i];
                mn[i] = (rv && dg0 + i < D) ? xh : 0.f;
                m2[i] = 0.f;
              }
            } else {
              const f32x4 pm = *(const GAS f32x4*)(o.mean + gi), p2 = *(const GAS f32x4*)(o.var + gi);
#pragma unroll
              for (int i = 0; i < 4; ++i) {
                const float xh = acc[ft][i] + bo[i];
                float a = pm[i], b = p2[i];
                dvd_fold(xh, rs, a, b);
                const bool dv = rv && dg0 + i < D;
                mn[i] = dv ? a : 0.f;
                m2[i] = dv ? b : 0.f;
              }
            }
            if (!last) {
              *(GAS f32x4*)(o.mean + gi) = mn;
              *(GAS f32x4*)(o.var + gi) = m2;
            } else {
              f32x4 nv4 = f32x4{1.f, 1.f, 1.f, 1.f};
              if (o.nv) nv4 = *(const GAS f32x4*)(o.nv + min(dg0, xp - 4));
              f32x4 va, sq, zz;
#pragma unroll
              for (int i = 0; i < 4; ++i) {
                float v1, q1, z1;
                dvd_final(xin[ft][i], mn[i], m2[i], vS, cS, nv4[i], v1, q1, z1);
                const bool dv = rv && dg0 + i < D;
                va[i] = dv ? v1 : 0.f;
                sq[i] = dv ? q1 : 0.f;
                zz[i] = (dv && o.nv) ? z1 : 0.f;
              }
              *(GAS f32x4*)(o.mean + gi) = mn;
              *(GAS f32x4*)(o.var + gi) = va;
              if (o.msq) *(GAS f32x4*)(o.msq + gi) = sq;
              if (o.z) *(GAS f32x4*)(o.z + gi) = zz;
              rdev += dvd_sum4(sq);
              rz2 += dvd_sumsq4(zz);
            }
          }
        }
        tr(c, 7);
      };
      {
        f32x4 xa[4], xb[4];
        if (wave_live && last) load_xin(0, xa);
        for (int ch = 0; ch < nck; ch += 2) {
          chunk(ch, xa, xb);
          if (ch + 1 < nck) chunk(ch + 1, xb, xa);
        }
      }
      if (last && wave_live) {                      // the row's four column groups sit in the lanes c16, c16 + 16, + 32, + 48
        float v = rdev, w = rz2;
        v += __shfl_xor(v, 16, 64);
        v += __shfl_xor(v, 32, 64);
        w += __shfl_xor(w, 16, 64);
        w += __shfl_xor(w, 32, 64);
        if (c.g == 0 && orow < c.nrows) {
          if (o.rdev) o.rdev[row0 + orow] = v / (float)D;
          if (o.rz2) o.rz2[row0 + orow] = w / (float)D;
        }
      }
      // (a ragged tile only, once: the rows no wave stores)
      if (last && live < ROWS) { relaunder(c); dvd_zero_dead_rows(c.tid, xp, o, row0, live); }
      tr(c, 8);
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// nm_decode_kernel -- the decoder half of nm_devpass_multi_kernel and nothing else: a table of latent rows z decoded under
// the rows' own covariates or under every row of a covariate grid (nmhip.h: nm_decode_t).  No encoder, no fusion, no draw,
// no workspace tile.  The sources of the kernels above stay as they are: their decoder loop and output-chunk epilogue are
// repeated here inside the loop over the grid's cells, the export pointers taken from the request.
//
// A workgroup owns 128 rows of the REQUEST (its own row count, not the job's tables'), two workgroups share a CU.  LDS: the
// plan of nm_devpass_multi_kernel (P, W, two vector slots, scalars, Z [128][32] bf16).  Per tile: z fp32 -> bf16 into Z once
// (the conversion build_zc and the draw code apply; zeros past the request's rows), then per cell g and wanted decoder m:
// z | c | 1 | 0 into P (dec_build_zc: the covariate block of the row itself, or row g of the grid for every row), the hidden
// layers through dv_layer, the 64-ROI chunks with nm_devpass_kernel's wave-per-16-rows epilogue.  Every value of a cell
// goes through the operations nm_devpass_multi_kernel applies to a row with that z and that covariate block, so with
// z = out_z and the tables' own cz / x the exports equal that kernel's (and the general kernel's) bit for bit, and cell g
// equals a per-row launch whose cz table repeats grid row g.
// A job dec_refused refuses, or a request whose counts are out of range, must not reach this kernel (the caller checks on
// the host); its workgroups leave at once, exports untouched.
__host__ __device__ inline int dec_refused(const nm_job_t* j) { return lat_refused(j); }     // the domain of the encoder half

// build_zc with the z columns from LDS and the covariate block from `cz` + r * cstride: cstride = Cz with cz at the tile's
// first row -- the table's own rows, build_zc's bytes -- or cstride = 0 -- ONE row for every row of the tile: the bytes
// build_zc produces from a table whose every row is that row.
__device__ __forceinline__ void dec_build_zc(const Ctx& c, __bf16* dst, const GAS uint16_t* cz, int cstride, int Z, int C,
                                             const __bf16* zsrc) {
  constexpr int ROWS = DV_ROWS;
  const int wz = wpad(Z + C);
  const float rz = 1.0f / (float)Z;
  {
    const int npc = (C + 1 + 7) >> 3;
    const float rnp = 1.0f / (float)npc;
    for (int p = c.tid; p < ROWS * npc; p += WG) {
      const int r = idiv(p, npc, rnp), col0 = 8 * (p - r * npc);
      const u32x4 v = *(const GAS u32x4*)(cz + (int64_t)r * cstride + col0);
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const int j = col0 + i;
        const uint16_t h = (uint16_t)(v[i >> 1] >> (16 * (i & 1)));
        if (j <= C) reinterpret_cast<uint16_t*>(dst)[r * LDP + Z + j] = h;
      }
    }
  }
  {                                                 // zero pad columns (Z + C, wz)
    const int nz = wz - (Z + C + 1);
    if (nz > 0) {
      const float rnz = 1.0f / (float)nz;
      for (int e = c.tid; e < ROWS * nz; e += WG) {
        const int r = idiv(e, nz, rnz);
        dst[r * LDP + Z + C + 1 + (e - r * nz)] = (__bf16)0.0f;
      }
    }
  }
#pragma unroll 4
  for (int e = c.tid; e < ROWS * Z; e += WG) {
    int r = idiv(e, Z, rz), k = e - r * Z;
    dst[r * LDP + k] = zsrc[r * 32 + k];
  }
}

__global__ __launch_bounds__(WG, 4) void nm_decode_kernel(const nm_job_t* __restrict__ jobs, const nm_decode_t* __restrict__ reqs,
                                                            int tile0, int flags) {
  constexpr int ROWS = DV_ROWS;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const nm_job_t* J = jobs + blockIdx.x;
  const nm_decode_t* const rq = reqs + blockIdx.x;
  if (dec_refused(J)) return;
  const int n_rows = rq->n_rows, ralloc = rq->rows_alloc, n_cells = rq->n_cells;
  if (n_rows < 0 || ralloc < n_rows || ralloc % TROWS != 0 || n_cells < 0 || n_cells > NM_MAX_CELLS || !rq->z) return;
  if (n_cells > 0 && !rq->cgrid) return;
  const int M = J->M;
  const int cells = n_cells > 0 ? n_cells : 1;
  const int t128 = tile0 + (int)blockIdx.y;
  const int row0 = t128 * ROWS;
  if (row0 >= n_rows) {
    // the second half of a ragged last 256-row tile: every cell's export rows come back as zeros (tiles beyond it -- the
    // grid is as tall as the launch's tallest request -- are not this request's)
    if (row0 < (n_rows + TROWS - 1) / TROWS * TROWS)
      for (int g = 0; g < cells; ++g)
        for (int m = 0; m < M; ++m) {
          const int xp = J->mod[m].x_pitch;
          const bool hx = rq->x[m] != nullptr;
          gf32 oloc = asg(rq->loc[m]), osq = hx ? asg(rq->sqerr[m]) : (gf32)nullptr, ordv = hx ? asg(rq->rowdev[m]) : (gf32)nullptr;
          if (oloc) oloc += (int64_t)g * ralloc * xp;
          if (osq) osq += (int64_t)g * ralloc * xp;
          if (ordv) ordv += (int64_t)g * ralloc;
          dvs_zero_dead_rows((int)threadIdx.x, xp, oloc, osq, ordv, row0, 0);
        }
    return;
  }
  Ctx c;
  c.job = J;
  c.part = -1; c.nparts = 1; c.lstep = 0;
  c.slope = J->act_slope;
  dv_carve(c, smem);
  relaunder(c);
  c.flags = NM_F_EXPORT | (flags & NM_F_TRACE);
  c.t_last = 0;
  c.ws = nullptr;
  for (int i = c.tid; i < DVM_SMEM / 4; i += WG) reinterpret_cast<uint32_t*>(smem)[i] = 0u;
  __syncthreads();
  if (c.flags & 64) c.tlast[c.wave_s] = clock64();
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
  auto to_W = [&](const GAS char* blob, int vs, int rows, int K) {
    return Next{blob, Wb, IMG_BYTES >> 10, blob + cimg_bytes(rows, K), reinterpret_cast<char*>(c.vec) + vs * VEC_BYTES, rows, blob_kp(K)};
  };
  // the first decoder that is wanted (workgroup-uniform; none: nothing to do but the tile's rows are nobody's either)
  int mf = 0;
  while (mf < M && !rq->loc[mf]) ++mf;
  if (mf == M) return;
  // W and P are free: the first decoder's image lands while z is converted
  issue_next(c, to_W(wsh + J->mod[mf].dec_s[0], 0, J->H[L - 1], Z + C));

  // ---- z: fp32 rows -> bf16 [128][32] in LDS, once per tile; rows past the request's end hold zeros ----
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
  tr(c, 3);

  // ---- per cell: every wanted decoder ----
  const int Hl = J->H[0];
  const int ob = L & 1;                            // (see nm_devpass_kernel: chunk 0's vectors avoid the last hidden layer's bias)
  for (int g = 0; g < cells; ++g) {
    for (int m = mf; m < M; ++m) {
      relaunder(c);
      const nm_modality_t& md = J->mod[m];
      const int D = md.D, xp = md.x_pitch;
      gcf32 xf = asg(rq->x[m]);
      gf32 oloc = asg(rq->loc[m]);
      if (!oloc) continue;                         // (workgroup-uniform) this decoder is not wanted: skipped entirely
      gf32 osq = xf ? asg(rq->sqerr[m]) : (gf32)nullptr, ordv = xf ? asg(rq->rowdev[m]) : (gf32)nullptr;
      oloc += (int64_t)g * ralloc * xp;
      if (osq) osq += (int64_t)g * ralloc * xp;
      if (ordv) ordv += (int64_t)g * ralloc;
      if (g != 0 || m != mf) {
        lds_barrier();                             // the previous decoder's last chunk is finished everywhere: P, W, vectors free
        issue_next(c, to_W(wsh + md.dec_s[0], 0, J->H[L - 1], Z + C));
      }
      if (n_cells > 0) dec_build_zc(c, c.P, asg(rq->cgrid) + (int64_t)g * md.Cz, 0, Z, C, zlds);
      else dec_build_zc(c, c.P, asg(rq->cz[m]) + (int64_t)row0 * md.Cz, md.Cz, Z, C, zlds);
      tr(c, 4);
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
        dv_layer(c, vs, nx, Nout, Kin, nl, live);    // (its first barrier also publishes z | c | 1)
        vs ^= 1;
      }
      tr(c, 5);
      // output layer in 64-ROI chunks, wave w owns rows [16 w, 16 w + 16) and all 64 columns: see nm_devpass_kernel
      float rdev = 0.f;
      const int orow = c.wave * 16 + c.c16;
      const bool wave_live = c.wave * 16 < live;
      const bool rv = orow < c.nrows;
      auto load_xin = [&](int chx, f32x4 (&xv)[4]) {
#pragma unroll
        for (int ft = 0; ft < 4; ++ft) {
          const int dcl = min(chx * OCH + ft * 16 + 4 * c.g, xp - 4);
          xv[ft] = *(const GAS f32x4*)(xf + (int64_t)(row0 + orow) * xp + dcl);
        }
      };
      int stores_prev = 0;
      auto chunk = [&](const int ch, f32x4 (&xin)[4], f32x4 (&xnx)[4]) {
        relaunder(c);
        const int d0 = ch * OCH;
        const __bf16* Wc = reinterpret_cast<const __bf16*>(Wb + (ch & 1) * OIMG_BYTES);
        const float* vb = c.vec + ((ch + ob) & 1) * (VEC_BYTES / 4);
        wait_vm(ch > 0 ? stores_prev : 0);
        lds_barrier();
        if (ch + 1 < nck) { issue_next(c, out_blob(ch + 1)); if (wave_live && xf) load_xin(ch + 1, xnx); }
        stores_prev = 0;
        if (!wave_live) return;
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
        tr(c, 6);
        const bool full = live == ROWS && d0 + OCH <= D;                   // no row / column masks needed (wave-uniform)
#pragma unroll
        for (int ft = 0; ft < 4; ++ft) {
          const int dg0 = d0 + ft * 16 + 4 * c.g;
          const f32x4 bo = *reinterpret_cast<const f32x4*>(vb + ft * 16 + 4 * c.g);
          f32x4 lo, sq;
          if (full) {
            lo = acc[ft] + bo;
            const f32x4 diff = lo - xin[ft];
            sq = diff * diff;
          } else {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
              const float xh = acc[ft][i] + bo[i];
              const bool dv = rv && dg0 + i < D;
              const float diff = xh - xin[ft][i];
              lo[i] = dv ? xh : 0.f;
              sq[i] = dv ? diff * diff : 0.f;
            }
          }
          rdev += ((sq[0] + sq[1]) + sq[2]) + sq[3];
          if (d0 + ft * 16 < xp) {                      // wave-uniform
            if (dg0 < xp) {
              const int64_t gi = (int64_t)(row0 + orow) * xp + dg0;
              *(GAS f32x4*)(oloc + gi) = lo;
              if (osq) *(GAS f32x4*)(osq + gi) = sq;
            }
            stores_prev += 1 + (osq ? 1 : 0);
          }
        }
        tr(c, 7);
      };
      {
        f32x4 xa[4], xb[4];
#pragma unroll
        for (int ft = 0; ft < 4; ++ft) { xa[ft] = f32x4{0.f, 0.f, 0.f, 0.f}; xb[ft] = xa[ft]; }
        if (wave_live && xf) load_xin(0, xa);
        for (int ch = 0; ch < nck; ch += 2) {
          chunk(ch, xa, xb);
          if (ch + 1 < nck) chunk(ch + 1, xb, xa);
        }
      }
      if (ordv && wave_live) {
        float v = rdev;
        v += __shfl_xor(v, 16, 64);
        v += __shfl_xor(v, 32, 64);
        if (c.g == 0 && orow < c.nrows) ordv[row0 + orow] = v / (float)D;
      }
      // (a ragged tile only: the rows no wave has stored; the laundered thread index keeps the loop's addresses from being
      //  hoisted out of the cell loop and held in registers across it)
      if (live < ROWS) { relaunder(c); dvs_zero_dead_rows(c.tid, xp, oloc, osq, ordv, row0, live); }
      tr(c, 8);
    }
  }
}

}  // namespace

extern "C" {

/* 0: the job's deviation pass can run on the compact kernel (one expert with the single-expert bypass, no private latent /
 * learnable weights / total correlation, first hidden width <= 112, latent <= 32, Gaussian output); NM_E_DEVPASS otherwise. */
int nm_devpass_ok(const nm_job_t* j) {
  if (!j) return NM_E_NULL;
  const int Me = j->M_enc > 0 ? j->M_enc : j->M;
  if (j->wide || j->M != 1 || Me != 1 || !j->single_bypass || j->n_private != 0 || j->tc_weight != 0.f || j->w_off >= 0) return NM_E_DEVPASS;
  if (j->H[0] > DV_MAX_H0 || rup(j->Z, 16) > 32 || j->out_kind != 0) return NM_E_DEVPASS;
  return 0;
}

/* The ROI-wise deviation pass (multimodal_kfold_train_cvae_supervised_regression.py:163-192) over table rows
 * [tile0 * 128, (tile0 + n_tiles) * 128): out_sqerr / out_rowdev / out_loc of modality 0, nothing else (no loss log, no
 * latent exports).  Every job must pass nm_devpass_ok. */
int nm_devpass(const nm_job_t* jobs_dev, int n_jobs, int tile0, int n_tiles, int flags, void* stream) {
  if (int bad = check_launch_geometry(jobs_dev, n_jobs, n_tiles, 1, tile0, 0)) return bad;
  return launch_kernel(nm_devpass_kernel, dim3(n_jobs, n_tiles), dim3(WG), DV_SMEM, stream, jobs_dev, tile0, flags & NM_F_TRACE);
}

/* 0: the job's multi-expert deviation pass can run on the compact kernel (not wide; 2..NM_MAX_EXP modalities, every one with
 * an encoder; no private latent / learnable weights / total correlation; Gaussian output; first hidden width <= 112, latent
 * <= 32 after rounding to 16); NM_E_DEVPASS otherwise.  single_bypass plays no part: it only acts on one-expert models. */
int nm_devpass_multi_ok(const nm_job_t* j) {
  if (!j) return NM_E_NULL;
  return dvm_refused(j);
}

/* pred_recon with the joint latent + reconstruction_deviation_multimodal (multimodal_kfold_test_cvae_supervised.py:112-113)
 * over table rows [tile0 * 128, (tile0 + n_tiles) * 128): out_loc / out_sqerr / out_rowdev of EVERY modality, nothing else.
 * Every job must pass nm_devpass_multi_ok -- checked by the caller on the host, as for nm_devpass (the descriptors are in
 * device memory here); the kernel makes a refused job's workgroups leave at once, its exports untouched.  Every job needs
 * one workspace tile per 256-row batch the launch touches: (tile0 + n_tiles + 1) / 2 - tile0 / 2 of them. */
int nm_devpass_multi(const nm_job_t* jobs_dev, int n_jobs, int tile0, int n_tiles, int flags, void* stream) {
  if (int bad = check_launch_geometry(jobs_dev, n_jobs, n_tiles, 1, tile0, 0)) return bad;
  return launch_kernel(nm_devpass_multi_kernel, dim3(n_jobs, n_tiles), dim3(WG), DVM_SMEM, stream, jobs_dev, tile0, flags & NM_F_TRACE);
}

/* The predicate of nm_devpass_multi_ok: the subset pass runs the same encoders and decoders in the same LDS plan. */
int nm_devpass_subsets_ok(const nm_job_t* j) {
  if (!j) return NM_E_NULL;
  return dvm_refused(j);
}

/* The modality-subset pass over table rows [tile0 * 128, (tile0 + n_tiles) * 128): encoders once per tile, then per entry of
 * subsets_dev[job][0 .. n_subsets) the fusion under the entry's mask, the draw and the decoders the entry exports (nmhip.h).
 * Status is decided here, on the host, before the device is asked anything -- the table and the descriptors live in device
 * memory: the per-entry rules (mask != 0, no bit >= M) are the caller's.  Workspace tiles as for nm_devpass_multi. */
int nm_devpass_subsets(const nm_job_t* jobs_dev, int n_jobs, const nm_subset_t* subsets_dev, int n_subsets, int tile0, int n_tiles,
                       int flags, void* stream) {
  if (!jobs_dev || !subsets_dev) return NM_E_NULL;
  if (n_subsets < 1 || n_subsets > NM_MAX_SUBSETS) return NM_E_GEOMETRY;
  if (int bad = check_launch_geometry(jobs_dev, n_jobs, n_tiles, 1, tile0, 0)) return bad;
  return launch_kernel(nm_devpass_subsets_kernel, dim3(n_jobs, n_tiles), dim3(WG), DVS_SMEM, stream, jobs_dev, subsets_dev, n_subsets,
                       tile0, flags & NM_F_TRACE);
}

/* 0: the job can run the posterior-predictive pass: what nm_devpass_multi_ok admits and one-expert jobs (bypass on or off)
 * within the same shape limits; NM_E_DEVPASS otherwise. */
int nm_devpass_draws_ok(const nm_job_t* j) {
  if (!j) return NM_E_NULL;
  return dvd_refused(j);
}

/* The posterior-predictive pass over table rows [tile0 * 128, (tile0 + n_tiles) * 128): encoders once per tile, then n_draws
 * times the fusion, the draw of draws_dev[job][s] and every decoder pred_dev[job] wants, folded into mean / variance /
 * mean squared error / z per ROI (nmhip.h).  Status is decided here, on the host, before the device is asked anything -- the
 * tables and the descriptors live in device memory: the per-job rules (pred_mean with pred_var, pred_z only with noise_var)
 * are the caller's.  Workspace tiles as for nm_devpass_multi, one-expert jobs included. */
int nm_devpass_draws(const nm_job_t* jobs_dev, int n_jobs, const nm_draw_t* draws_dev, int n_draws, const nm_pred_t* pred_dev,
                     int tile0, int n_tiles, int flags, void* stream) {
  if (!jobs_dev || !draws_dev || !pred_dev) return NM_E_NULL;
  if (n_draws < 1 || n_draws > NM_MAX_DRAWS) return NM_E_GEOMETRY;
  if (int bad = check_launch_geometry(jobs_dev, n_jobs, n_tiles, 1, tile0, 0)) return bad;
  return launch_kernel(nm_devpass_draws_kernel, dim3(n_jobs, n_tiles), dim3(WG), DVD_SMEM, stream, jobs_dev, draws_dev, n_draws,
                       pred_dev, tile0, flags & NM_F_TRACE);
}

/* 0: the job's joint latent statistics can come from the encoder-only kernel (not wide; 1..NM_MAX_EXP modalities, every one
 * with an encoder; no private latent / learnable weights / total correlation; Gaussian output; first hidden width <= 112,
 * latent <= 32 after rounding to 16); NM_E_DEVPASS otherwise.  One-expert jobs pass with the bypass on or off. */
int nm_latent_pass_ok(const nm_job_t* j) {
  if (!j) return NM_E_NULL;
  return lat_refused(j);
}

/* The joint posterior of every row (cVAE.pred_latent, cVAE.py:539-545) over table rows [tile0 * 128, (tile0 + n_tiles) * 128):
 * out_mu / out_logvar, nothing else (out_z and the per-modality exports stay as they are).  Every job must pass
 * nm_latent_pass_ok -- checked by the caller on the host; the kernel makes a refused job's workgroups leave at once.  A job
 * with several experts needs one workspace tile per 256-row batch the launch touches, as for nm_devpass_multi. */
int nm_latent_pass(const nm_job_t* jobs_dev, int n_jobs, int tile0, int n_tiles, int flags, void* stream) {
  if (int bad = check_launch_geometry(jobs_dev, n_jobs, n_tiles, 1, tile0, 0)) return bad;
  return launch_kernel(nm_latent_kernel, dim3(n_jobs, n_tiles), dim3(WG), DV_SMEM, stream, jobs_dev, tile0, flags & NM_F_TRACE);
}

/* 0: the job's decoders can run on the decoder-only kernel: exactly what nm_latent_pass_ok admits, so the two halves cover
 * the same models; NM_E_DEVPASS otherwise. */
int nm_decode_pass_ok(const nm_job_t* j) {
  if (!j) return NM_E_NULL;
  return dec_refused(j);
}

/* The decoder half alone over rows [tile0 * 128, (tile0 + n_tiles) * 128) of every job's request (nmhip.h: nm_decode_t): z
 * decoded under the rows' own covariates or under every row of a covariate grid, loc / sqerr / rowdev per cell.  Status is
 * decided here, on the host, before the device is asked anything -- the descriptors and the requests live in device memory:
 * the request's own rules (n_cells, rows_alloc, sqerr / rowdev only with x) are the caller's.  No workspace tile. */
int nm_decode_pass(const nm_job_t* jobs_dev, int n_jobs, const nm_decode_t* req_dev, int tile0, int n_tiles, int flags, void* stream) {
  if (!jobs_dev || !req_dev) return NM_E_NULL;
  if (int bad = check_launch_geometry(jobs_dev, n_jobs, n_tiles, 1, tile0, 0)) return bad;
  return launch_kernel(nm_decode_kernel, dim3(n_jobs, n_tiles), dim3(WG), DVM_SMEM, stream, jobs_dev, req_dev, tile0, flags & NM_F_TRACE);
}

/* NM_F_TRACE read-out of nm_devpass ([8 waves][64 tags] interval cycles of workgroup (0, 0), as nm_trace_read) */
int nm_trace_read_dv(unsigned long long* out512, int reset) {
  return read_counters(out512, nm_trace_cycles, reset);
}

}  // extern "C"

#include "nm_iw.inc"
#include "nm_chart.inc"
#include "nm_e2e.inc"
#include "nm_fi.inc"
