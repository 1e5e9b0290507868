// ---------------------------------------------------------------------------------------------------------------------
// nm_fi_kernel -- the evaluation pass of cVAE_multimodal_regression (cVAE.py:2249-2253, 2317-2323) in one launch: per (job,
// 128-row tile) every expert's encoder chain ONCE, then per draw s the fusion, the latent (the job's own draw, entry s of the
// draw table, or the joint mean), every decoder, and the regressor on the residuals x - x_hat -- which never leave the CU:
// an output chunk's residual goes to LDS as bf16 [128][72], rounded as the reg_resid export of the general kernel rounds it,
// and is multiplied with the matching W1 chunk image of the shadow (job.reg_s) right there.  One row of eight numbers per
// subject (nmhip.h: nm_fi_t, NM_FI_ROW_COLUMNS): mean, spread, minimum and maximum of the S predictions, the error against
// the target, the mean deviation of draw 0, the analytic KL, a status word.  The sources of the kernels above stay as they
// are (this file is included at the end of nm_devpass.hip): the encoder loop, the fusion and the decoder loop are repeated.
//
// The head, operation by operation what nm_forward (export) + nm_head_regression compute:
//   layer 1   chunks in the order of fwd_first_layer (modality by modality, chunk by chunk, two K steps of 32 per chunk),
//             fp32 accumulators that start at zero and live in REGISTERS across the decoders of a draw (acc[2][4] per lane:
//             the wave grid of every hidden layer); b1 is added in the activation epilogue (act_to_P, slope 0), where
//             fwd_first_layer adds it
//   layer 2   reg_head_body's: bias in the accumulator, W2 fragments from the fp32 master, ReLU into P
//   layer 3   one row per thread, the fmaf chain over the 64 columns of h2 starting from b3
//
// LDS plan: nm_devpass_multi_kernel's P, W, two vector slots, scalars and Z [128][32] bf16 (81,232 bytes, padded to
// 81,920 so that the copies below land on 1-KiB pieces), the W1 chunk image [128][72] bf16 (18,432), the residual chunk
// [128][72] bf16 (18,432), b1 (512) and the row scratch [6][128] fp32 (3,072): 122,368 bytes.  The siblings' two-per-CU
// budget is 81,920: the several-expert plan leaves 688 bytes of it, W is full with the two output-chunk slots while a
// chunk's residual is formed, P holds the decoder's last activation, which every chunk reads -- so neither the residual nor
// the W1 image can borrow them, and ONE workgroup runs per CU (8 waves, built for 2 waves per SIMD).  The first-layer
// accumulators take registers, not LDS.  No hand-issued loads beyond those of the shared phases; the chunk boundaries take
// a full wait (wait_vm(0)): LDS-DMA copies, input loads and export stores share one queue.
//
// A job fi_refused refuses must not reach this kernel (the caller asks nm_fi_pass_ok on the host); its workgroups leave
// at once, exports untouched.
namespace {

constexpr int FI_ROW = NM_FI_ROW_COLUMNS;
constexpr int FI_W1_OFF = 81920;                                      // W1 chunk image
constexpr int FI_R_OFF = FI_W1_OFF + DV_ROWS * LDX * 2;               // residual chunk
constexpr int FI_B1_OFF = FI_R_OFF + DV_ROWS * LDX * 2;               // b1 [128] fp32
constexpr int FI_TAB_OFF = FI_B1_OFF + 128 * 4;
constexpr int FI_T_DEV = 0, FI_T_KL = NM_MAX_EXP, FI_T_BAD = NM_MAX_EXP + 1;
constexpr int FI_TAB_COLS = FI_T_BAD + 1;                             // 6
constexpr int FI_SMEM = FI_TAB_OFF + FI_TAB_COLS * DV_ROWS * 4;
constexpr int FI_N1 = 128, FI_N2 = 64;                                // the regressor's hidden widths (cVAE.py:2249-2253)
static_assert(DVM_SMEM <= FI_W1_OFF && (FI_W1_OFF & 1023) == 0 && DV_ROWS * LDX * 2 == W0IMG_BYTES, "W1 image: whole 1-KiB pieces");
static_assert(FI_SMEM == 122368 && FI_SMEM <= 160 * 1024, "one workgroup per CU");
static_assert(2 * FI_SMEM > 160 * 1024 && DVM_SMEM + 2 * W0IMG_BYTES > 81920, "why not two: see the header comment");
static_assert(FI_ROW == 8 && sizeof(nm_fi_t) == 24, "row layout, request layout (mirrored in _lib.py)");

__host__ __device__ inline int fi_refused(const nm_job_t* j) {
  if (j->wide) return NM_E_DEVPASS;
  const int Me = j->M_enc > 0 ? j->M_enc : j->M;
  if (j->M < 1 || j->M > NM_MAX_EXP || Me != j->M) return NM_E_DEVPASS;
  if (j->reg_head != 1 || j->reg_s < 0) return NM_E_DEVPASS;
  for (int i = 0; i < 3; ++i)
    if (j->reg_w[i] < 0 || j->reg_b[i] < 0 || (j->reg_w[i] & 255) || (j->reg_b[i] & 3)) return NM_E_DEVPASS;
  if (j->n_private != 0 || j->tc_weight != 0.f || j->w_off >= 0 || j->out_kind != 0) return NM_E_DEVPASS;
  if (j->Z < 1 || rup(j->Z, 16) > 32) return NM_E_DEVPASS;
  if (j->L < 1 || j->L > NM_MAX_HID || j->H[0] > DV_MAX_H0) return NM_E_DEVPASS;
  for (int i = 0; i < j->L; ++i)
    if (j->H[i] < 1 || j->H[i] > NM_MAX_WIDTH) return NM_E_DEVPASS;
  if (j->cls_layers != 0 || j->cls_classes != 0) return NM_E_DEVPASS;
  if (j->combine == NM_COMBINE_GPOE && !(j->M == 1 && j->single_bypass))
    for (int m = 0; m < j->M; ++m)
      if (j->mod[m].alpha < 0) return NM_E_DEVPASS;
  return 0;
}

// rows [live, 128) of the tile: every buffer the pass writes comes back as zeros there
__device__ __forceinline__ void fi_zero_dead_rows(int tid, const nm_job_t* J, const nm_fi_t& rq, uint32_t want, int n_draws, int row0,
                                                  int live, bool latent_too) {
  for (int k = 0; k < J->M; ++k) {
    if (!((want >> k) & 1u)) continue;
    const nm_modality_t& md = J->mod[k];
    dvs_zero_dead_rows(tid, md.x_pitch, asg(md.out_loc), asg(md.out_sqerr), asg(md.out_rowdev), row0, live);
  }
  if (latent_too) {                                // (a tile without a table row: a live tile zeroes these in its fusion phase)
    const int Z = J->Z;
    for (int e = tid; e < DV_ROWS * Z; e += WG) {
      const int64_t gi = (int64_t)row0 * Z + e;
      if (J->out_mu) asg(J->out_mu)[gi] = 0.f;
      if (J->out_logvar) asg(J->out_logvar)[gi] = 0.f;
      if (J->out_z) asg(J->out_z)[gi] = 0.f;
    }
  }
  gf32 const rowtab = asg(rq.row);
  gf32 const fdr = asg(rq.fi_draws);
  for (int r = live + tid; r < DV_ROWS; r += WG) {
    if (J->out_fi_pred) asg(J->out_fi_pred)[row0 + r] = 0.f;
    if (rowtab) {
#pragma unroll
      for (int i = 0; i < FI_ROW; i += 4) *(GAS f32x4*)(rowtab + (int64_t)(row0 + r) * FI_ROW + i) = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    if (fdr)
      for (int s = 0; s < n_draws; ++s) fdr[(int64_t)(row0 + r) * n_draws + s] = 0.f;
  }
}

// one step of the fold over the draws (s >= 1): rs = 1 / (s + 1); nm_devpass_draws' fold of a reconstruction
__device__ __forceinline__ void fi_fold(float p, float rs, float& mean, float& m2) {
#pragma clang fp contract(off)
  const float d = p - mean;
  mean = mean + d * rs;
  m2 = m2 + d * (p - mean);
}
__device__ __forceinline__ float fi_sd(float m2, float v) {
#pragma clang fp contract(off)
  return sqrtf(m2 * v);
}
__device__ __forceinline__ float fi_dev(const float* tab, int r, int M, int& bad) {
#pragma clang fp contract(off)
  float d = 0.f;
  for (int m = 0; m < M; ++m) {
    const float v = tab[(FI_T_DEV + m) * DV_ROWS + r];
    d = m ? d + v : v;
    bad |= e2e_nonfinite(v);
  }
  return d / (float)M;
}
__device__ __forceinline__ float fi_sub(float a, float b) {
#pragma clang fp contract(off)
  return a - b;
}

__global__ __launch_bounds__(WG, 2) void nm_fi_kernel(const nm_job_t* __restrict__ jobs, const nm_draw_t* __restrict__ draws, int n_draws,
                                                        const nm_fi_t* __restrict__ reqs, int tile0, int flags) {
  constexpr int RT = DV_RT, ROWS = DV_ROWS, WROWS = DV_RT * 16;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const nm_job_t* J = jobs + blockIdx.x;
  if (fi_refused(J) || !J->workspace || n_draws < 1 || n_draws > NM_MAX_DRAWS) return;
  const nm_fi_t& rq = reqs[blockIdx.x];
  const nm_draw_t* const drs = draws ? draws + (int64_t)blockIdx.x * n_draws : nullptr;
  const int M = J->M;
  gf32 const rowtab = asg(rq.row);
  gf32 const fdr = asg(rq.fi_draws);
  const uint32_t want = (uint32_t)rq.want_mask & ((1u << M) - 1u);
  const int t128 = tile0 + (int)blockIdx.y;
  const int row0 = t128 * ROWS;
  if (row0 >= J->n_rows) {
    // the second half of a ragged last 256-row tile: the export rows come back as zeros
    if (row0 < (J->n_rows + TROWS - 1) / TROWS * TROWS) fi_zero_dead_rows((int)threadIdx.x, J, rq, want, n_draws, row0, 0, true);
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
  for (int i = c.tid; i < FI_SMEM / 4; i += WG) reinterpret_cast<uint32_t*>(smem)[i] = 0u;
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
  // a one-expert job with the bypass and no latent export: nm_forward makes the draw inside the heads' epilogue (fwd_heads)
  const bool byp_draw = byp && !(J->out_mu || J->out_logvar || J->out_z);
  const bool mean_z = rq.use_mean != 0;
  GAS char* const wsh = (GAS char*)J->wsh;
  char* const Wb = reinterpret_cast<char*>(c.Q);
  __bf16* const zlds = reinterpret_cast<__bf16*>(smem + DV_SMEM);
  char* const w1slot = reinterpret_cast<char*>(smem + FI_W1_OFF);
  __bf16* const Rc = reinterpret_cast<__bf16*>(smem + FI_R_OFF);                 // [128][LDX]
  float* const b1l = reinterpret_cast<float*>(smem + FI_B1_OFF);
  float* const tab = reinterpret_cast<float*>(smem + FI_TAB_OFF);                // [FI_TAB_COLS][128]
  const WsLayout wl = ws_layout(M, L, Z);
  gf32 ws_mu_m = (gf32)(c.ws + wl.mu_m) + c.rloc0 * Zs;
  gf32 ws_lv_m = (gf32)(c.ws + wl.lv_m) + c.rloc0 * Zs;
  auto to_W = [&](const GAS char* blob, int vs, int rows, int K) {
    return Next{blob, Wb, IMG_BYTES >> 10, blob + cimg_bytes(rows, K), reinterpret_cast<char*>(c.vec) + vs * VEC_BYTES, rows, blob_kp(K)};
  };
  // the regressor: W1 chunk images and b1 in the shadow, layers 2 and 3 in the fp32 master
  const int nq = head_chunk0(J, M);
  const GAS char* const wimg = wsh + J->reg_s;
  gcf32 prm = asg(J->params);
  gcf32 W2 = prm + J->reg_w[1], b2 = prm + J->reg_b[1], W3 = prm + J->reg_w[2];
  if (c.tid < FI_N1) b1l[c.tid] = ((const GAS float*)(wimg + (int64_t)nq * W0IMG_BYTES))[c.tid];

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

  const int Hl = J->H[0];
  const int ob = L & 1;                            // (see nm_devpass_kernel: chunk 0's vectors avoid the last hidden layer's bias)
  // the fold over the draws: thread r (< 128) owns row r
  float f_mean = 0.f, f_m2 = 0.f, f_min = 0.f, f_max = 0.f;
  int f_bad = 0;

  for (int s = 0; s < n_draws; ++s) {
    relaunder(c);
    const bool first = s == 0;
    const uint64_t seed = drs ? drs[s].seed : J->seed;
    const GAS float* const epsp = asg(drs ? drs[s].eps : J->eps);
    if (!first) lds_barrier();                     // the previous draw's head is finished everywhere: P, W, vectors, Z free

    // ---- fusion and the latent of draw s: z -> LDS; draw 0 also exports and folds the row's KL; four lanes per row ----
    {
      float al[NM_MAX_EXP] = {0.f, 0.f, 0.f, 0.f};
      if (J->combine == NM_COMBINE_GPOE && !byp) softmax_alpha(J, al);
      relaunder(c);
      const int r = c.tid >> 2, sub = c.tid & 3;
      const bool rv = r < c.nrows;
      const int64_t eprow = ((int64_t)(step % J->eps_cap) * TROWS + c.rloc0 + r) * Z;
      const int64_t grow = (int64_t)(c.row0 + r) * Z;
      float klp = 0.f;
      int bad = 0;
      if (vec4) {
        for (int z0 = 4 * sub; z0 < Z; z0 += 16) {
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
          float ep[4] = {0.f, 0.f, 0.f, 0.f};
          if (!mean_z) {
            if (epsp) {
#pragma unroll
              for (int i = 0; i < 4; ++i) ep[i] = epsp[eprow + z0 + i];
            } else {
              randn2_ctr(seed, (uint32_t)step, (uint32_t)(c.row0 + r), (uint32_t)(z0 >> 1), ep[0], ep[1]);
              randn2_ctr(seed, (uint32_t)step, (uint32_t)(c.row0 + r), (uint32_t)(z0 >> 1) + 1u, ep[2], ep[3]);
            }
          }
          f32x4 omu, olv, oz;
          bf16x4 zk;
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            Lat Lt;
#pragma unroll
            for (int m = 0; m < NM_MAX_EXP; ++m) { Lt.mu[m] = mu4[m][i]; Lt.lv[m] = lv4[m][i]; }
            const Fuse f = fuse_fwd(J, Lt, al);
            float zz;
            if (byp_draw) {
              zz = dvd_z_bypass(f.mu, ep[i], f.lv);
            } else {
              const float es = ep[i] * fx_exp(0.5f * f.lv);      // (the joint mean: an all-zero eps, as the two-launch route has it)
              zz = dvm_add(f.mu, es);
            }
            omu[i] = f.mu; olv[i] = f.lv; oz[i] = zz;
            klp += e2e_kl_term(f.mu, f.lv);
            bad |= e2e_nonfinite(f.mu) | e2e_nonfinite(f.lv);
            zk[i] = (__bf16)zz;
          }
          *reinterpret_cast<bf16x4*>(zlds + r * 32 + z0) = zk;
          if (first) {
            if (!rv) { omu = f32x4{0.f, 0.f, 0.f, 0.f}; olv = omu; oz = omu; }      // (rows past the table: zeros)
            if (J->out_mu) *(GAS f32x4*)(asg(J->out_mu) + grow + z0) = omu;
            if (J->out_logvar) *(GAS f32x4*)(asg(J->out_logvar) + grow + z0) = olv;
            if (J->out_z) *(GAS f32x4*)(asg(J->out_z) + grow + z0) = oz;
          }
        }
      } else {
        for (int z = sub; z < Z; z += 4) {
          Lat Lt;
#pragma unroll
          for (int m = 0; m < NM_MAX_EXP; ++m) {
            Lt.mu[m] = (m < M) ? ws_mu_m[((int64_t)m * TROWS + r) * Zs + z] : 0.f;
            Lt.lv[m] = (m < M) ? ws_lv_m[((int64_t)m * TROWS + r) * Zs + z] : 0.f;
          }
          const Fuse f = fuse_fwd(J, Lt, al);
          float ep = 0.f;
          if (!mean_z) ep = epsp ? epsp[eprow + z] : randn_ctr(seed, (uint32_t)step, (uint32_t)(c.row0 + r), (uint32_t)z);
          float zz;
          if (byp_draw) {
            zz = dvd_z_bypass(f.mu, ep, f.lv);
          } else {
            const float es = ep * fx_exp(0.5f * f.lv);
            zz = dvm_add(f.mu, es);
          }
          klp += e2e_kl_term(f.mu, f.lv);
          bad |= e2e_nonfinite(f.mu) | e2e_nonfinite(f.lv);
          zlds[r * 32 + z] = (__bf16)zz;
          if (first) {
            if (J->out_mu) asg(J->out_mu)[grow + z] = rv ? f.mu : 0.f;       // (rows past the table: zeros)
            if (J->out_logvar) asg(J->out_logvar)[grow + z] = rv ? f.lv : 0.f;
            if (J->out_z) asg(J->out_z)[grow + z] = rv ? zz : 0.f;
          }
        }
      }
      if (first) {
        // the row's KL and flag: the four lanes' shares, always in the same order
        klp += __shfl_xor(klp, 1, 64);
        klp += __shfl_xor(klp, 2, 64);
        bad |= __shfl_xor(bad, 1, 64);
        bad |= __shfl_xor(bad, 2, 64);
        if (sub == 0) {
          tab[FI_T_KL * ROWS + r] = rv ? -0.5f * klp : 0.f;
          tab[FI_T_BAD * ROWS + r] = (rv && bad) ? 1.0f : 0.f;
        }
      }
    }
    tr(c, 3);

    // ---- decoders: every one runs (the head needs its residual); exports of draw 0 where they are wanted ----
    f32x4 acc1[2][RT];                             // the regressor's first layer, across the decoders
    zero_acc(acc1);
    for (int m = 0; m < M; ++m) {
      relaunder(c);
      const nm_modality_t& md = J->mod[m];
      const bool wanted = first && ((want >> m) & 1u) != 0u;
      gf32 const oloc = wanted ? asg(md.out_loc) : (gf32)nullptr;
      gf32 const osq = wanted ? asg(md.out_sqerr) : (gf32)nullptr;
      gf32 const ordv = wanted ? asg(md.out_rowdev) : (gf32)nullptr;
      const int D = md.D;
      const int q0 = head_chunk0(J, m);
      lds_barrier();                               // z is complete / the previous decoder's last chunk is finished: P, W, vectors free
      issue_next(c, to_W(wsh + md.dec_s[0], 0, J->H[L - 1], Z + C));
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
      auto chunk = [&](const int ch, f32x4 (&xin)[4], f32x4 (&xnx)[4]) {
        relaunder(c);
        const int d0 = ch * OCH;
        const __bf16* Wc = reinterpret_cast<const __bf16*>(Wb + (ch & 1) * OIMG_BYTES);
        const float* vb = c.vec + ((ch + ob) & 1) * (VEC_BYTES / 4);
        // chunk ch's rows, vectors and inputs have landed; the previous chunk's head GEMM is finished everywhere (the
        // residual chunk and the W1 image are free)
        wait_vm(0);
        lds_barrier();
        dma_lin(c, wimg + (int64_t)(q0 + ch) * W0IMG_BYTES, w1slot, W0IMG_BYTES >> 10);
        if (ch + 1 < nck) { issue_next(c, out_blob(ch + 1)); if (wave_live) load_xin(ch + 1, xnx); }
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
          tr(c, 6);
          const bool rv = orow < c.nrows;
#pragma unroll
          for (int ft = 0; ft < 4; ++ft) {
            const int dg0 = d0 + ft * 16 + 4 * c.g;
            const f32x4 bo = *reinterpret_cast<const f32x4*>(vb + ft * 16 + 4 * c.g);
            f32x4 lo, sq;
            bf16x4 rk;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
              const float xh = acc[ft][i] + bo[i];
              const bool dv = rv && dg0 + i < D;
              const float diff = xh - xin[ft][i];
              lo[i] = dv ? xh : 0.f;
              sq[i] = dv ? diff * diff : 0.f;
              rk[i] = (__bf16)(dv ? fi_sub(xin[ft][i], xh) : 0.f);       // x - x_hat: the head's first-layer operand
            }
            *reinterpret_cast<bf16x4*>(Rc + orow * LDX + ft * 16 + 4 * c.g) = rk;
            rdev += ((sq[0] + sq[1]) + sq[2]) + sq[3];
            if (d0 + ft * 16 < xp && dg0 < xp) {          // (the first: wave-uniform)
              const int64_t gi = (int64_t)(row0 + orow) * xp + dg0;
              if (oloc) *(GAS f32x4*)(oloc + gi) = lo;
              if (osq) *(GAS f32x4*)(osq + gi) = sq;
            }
          }
          tr(c, 7);
        }
        // ---- the head's first layer on this chunk: every wave, its tiles of the (wm, wn) grid ----
        wait_vm(0);                                // the W1 image has landed
        lds_barrier();                             // ... for every wave, and the residual chunk is complete
        {
          const __bf16* Wq = reinterpret_cast<const __bf16*>(w1slot);
#pragma unroll
          for (int ks = 0; ks < 2; ++ks) {
            bf16x8 wf[2];
#pragma unroll
            for (int t = 0; t < 2; ++t) wf[t] = lds_frag(Wq, LDX, (c.wn + 4 * t) * 16 + c.c16, ks * 32 + 8 * c.g);
#pragma unroll
            for (int rt = 0; rt < RT; ++rt) {
              if (c.wm * WROWS + rt * 16 < live) {             // wave-uniform
                bf16x8 a = lds_frag(Rc, LDX, c.wm * WROWS + rt * 16 + c.c16, ks * 32 + 8 * c.g);
#pragma unroll
                for (int t = 0; t < 2; ++t) acc1[t][rt] = mfma(wf[t], a, acc1[t][rt]);
              }
            }
          }
        }
      };
      {
        f32x4 xa[4], xb[4];
        if (wave_live) load_xin(0, xa);
        for (int ch = 0; ch < nck; ch += 2) {
          chunk(ch, xa, xb);
          if (ch + 1 < nck) chunk(ch + 1, xb, xa);
        }
      }
      if (first && wave_live) {                     // the row's four column groups sit in the lanes c16, c16 + 16, + 32, + 48
        float v = rdev;
        v += __shfl_xor(v, 16, 64);
        v += __shfl_xor(v, 32, 64);
        const float dvr = v / (float)D;
        if (c.g == 0 && orow < c.nrows) {
          tab[(FI_T_DEV + m) * ROWS + orow] = dvr;
          if (ordv) ordv[row0 + orow] = dvr;
        }
      }
      // (a ragged tile only: the rows no wave has stored)
      if (first && live < ROWS) { relaunder(c); dvs_zero_dead_rows(c.tid, xp, oloc, osq, ordv, row0, live); }
      tr(c, 8);
    }

    // ---- the head: h1 = relu(acc1 + b1) -> P, layer 2, layer 3 (reg_head_body's forward over 128 rows) ----
    lds_barrier();                                 // the last chunk's GEMMs are finished everywhere: P is free
    relaunder(c);
    {
      Ctx hc = c;
      hc.slope = 0.f;                              // ReLU
      act_to_P(hc, acc1, b1l, FI_N1, wpad(FI_N1) / 16, true);
    }
    lds_barrier();
    tr(c, 21);
    {
      f32x4 acc[2][RT];
      bias_acc(c, acc, b2, FI_N2, 0);
      for (int ks = 0; ks < FI_N1 / 32; ++ks) {
        bf16x8 wf[2];
#pragma unroll
        for (int t = 0; t < 2; ++t) wf[t] = w_frag(W2, FI_N2, FI_N1, (c.wn + 4 * t) * 16 + c.c16, ks * 32 + 8 * c.g);
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) {
          bf16x8 a = lds_frag(c.P, LDP, c.wm * WROWS + rt * 16 + c.c16, ks * 32 + 8 * c.g);
#pragma unroll
          for (int t = 0; t < 2; ++t) acc[t][rt] = mfma(wf[t], a, acc[t][rt]);
        }
      }
      lds_barrier();
#pragma unroll
      for (int t = 0; t < 2; ++t) {                // relu_to_P (nmhip.hip)
        const int f0 = (c.wn + 4 * t) * 16 + 4 * c.g;
        if (f0 >= FI_N2) continue;
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) {
          const int r = c.wm * WROWS + rt * 16 + c.c16;
          bf16x4 pk;
#pragma unroll
          for (int i = 0; i < 4; ++i) pk[i] = (__bf16)fmaxf(acc[t][rt][i], 0.f);
          *reinterpret_cast<bf16x4*>(c.P + r * LDP + f0) = pk;
        }
      }
      lds_barrier();
    }
    relaunder(c);
    if (c.tid < ROWS) {
      const int r = c.tid;
      float p = prm[J->reg_b[2]];
      for (int n = 0; n < FI_N2; ++n) p = fmaf((float)c.P[r * LDP + n], (float)(__bf16)W3[wt_off(0, n, FI_N2 / 16)], p);
      if (r < c.nrows) {
        if (first) {
          f_mean = p; f_m2 = 0.f; f_min = p; f_max = p;
          if (J->out_fi_pred) asg(J->out_fi_pred)[row0 + r] = p;
        } else {
          fi_fold(p, 1.0f / (float)(s + 1), f_mean, f_m2);
          f_min = fminf(f_min, p);
          f_max = fmaxf(f_max, p);
        }
        f_bad |= e2e_nonfinite(p);
        if (fdr) fdr[(int64_t)(row0 + r) * n_draws + s] = p;
      }
    }
    tr(c, 22);
  }

  // ---- the row table: thread r owns row r; the rows past the table's end ----
  lds_barrier();                                   // every lane's words of the row scratch are in place
  relaunder(c);
  if (rowtab && c.tid < live) {
    const int r = c.tid;
    int bad = f_bad | (tab[FI_T_BAD * ROWS + r] != 0.f ? 1 : 0);
    const float dev = fi_dev(tab, r, M, bad);
    const float sd = n_draws > 1 ? fi_sd(f_m2, 1.0f / (float)(n_draws - 1)) : 0.f;
    float err = 0.f;
    int st = 0;
    if (J->fi_target) err = fi_sub(f_mean, asg(J->fi_target)[row0 + r]);
    else st = 2;
    st |= bad ? 1 : 0;
    gf32 orw = rowtab + (int64_t)(row0 + r) * FI_ROW;
    *(GAS f32x4*)orw = f32x4{f_mean, sd, f_min, f_max};
    *(GAS f32x4*)(orw + 4) = f32x4{err, dev, tab[FI_T_KL * ROWS + r], (float)st};
  }
  if (live < ROWS) fi_zero_dead_rows(c.tid, J, rq, 0u, n_draws, row0, live, false);
}

}  // namespace

extern "C" {

/* 0: the job's evaluation can run on nm_fi_pass (nmhip.h states the domain); NM_E_DEVPASS otherwise. */
int nm_fi_pass_ok(const nm_job_t* j) {
  if (!j) return NM_E_NULL;
  return fi_refused(j);
}

/* The regression model's evaluation pass over table rows [tile0 * 128, (tile0 + n_tiles) * 128).  Status is decided here, on
 * the host, before the device is asked anything -- the descriptors, the draw table and the requests live in device memory:
 * every job must pass nm_fi_pass_ok, asked by the caller while the descriptor is still on the host, and whether a request's
 * use_mean comes with n_draws == 1 is the caller's to check.  draws_dev may be NULL with n_draws == 1 (the job's own seed /
 * eps).  Workspace tiles as for nm_devpass_multi, one-expert jobs included. */
int nm_fi_pass(const nm_job_t* jobs_dev, int n_jobs, const nm_draw_t* draws_dev, int n_draws, const nm_fi_t* req_dev, int tile0,
               int n_tiles, int flags, void* stream) {
  if (!jobs_dev || !req_dev) return NM_E_NULL;
  if (n_draws < 1 || n_draws > NM_MAX_DRAWS) return NM_E_GEOMETRY;
  if (!draws_dev && n_draws != 1) return NM_E_NULL;
  if (int bad = check_launch_geometry(jobs_dev, n_jobs, n_tiles, 1, tile0, 0)) return bad;
  return launch_kernel(nm_fi_kernel, dim3(n_jobs, n_tiles), dim3(WG), FI_SMEM, stream, jobs_dev, draws_dev, n_draws, req_dev, tile0,
                       flags & NM_F_TRACE);
}

}  // extern "C"
