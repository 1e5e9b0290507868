// ---------------------------------------------------------------------------------------------------------------------
// nm_e2e_kernel -- the evaluation pass of cVAE_multimodal_endtoend (cVAE.py:2021-2207) in one launch: per (job, 128-row
// tile) every expert's encoder chain, the fusion, the latent (joint mean or the general kernel's draw), the classifier in
// eval mode, both decoder banks with nm_devpass_multi_kernel's export epilogue, and one row of eight numbers per subject
// (nmhip.h: nm_e2e_t, NM_E2E_ROW_COLUMNS) -- class probability, prediction, margin, the per-bank deviations the hinge
// loss trains and their contrast, the analytic KL, a status word.  The sources of the kernels above stay as they are (this
// file is included at the end of nm_devpass.hip): the encoder loop, the fusion and the decoder loop are repeated here.
//
// What differs from nm_devpass_multi_kernel:
//   experts / decoders   M_enc experts, M = 2 M_enc decoders (health bank k < M_enc, disease bank M_enc <= k < M)
//   latent               up to NM_MAX_LATENT = 64 columns: the heads image [2 Zs][LDP] fills W at Zs = 64, so z cannot sit
//                        behind it, and [128][64] bf16 is 16 KB.  z gets its own buffer with a fixed pitch of 64
//                        (e2e_build_zc: build_zc's LDS branch reads pitch 32).
//   classifier           cls_head_body's one-tile forward (nmhip.hip) with the running statistics, K order and
//                        bias-in-accumulator form kept: the input (bf16 of the joint mean or of z) is written into P by
//                        the fusion phase, the block's weights go through registers into W, the logits layer reads its
//                        fragments from the fp32 master.  Nothing is written to the parameters.
//   row table            what a row needs between the phases lives in LDS, column-major [14][128] fp32: the eight decoders'
//                        deviations, four logits, the KL and the non-finite flag of the latent statistics.  Each word has
//                        one writer; the row's owner (thread r of the workgroup) folds them after the last decoder.
//
// LDS plan: nm_devpass_kernel's P, W, two vector slots and scalars (DV_SMEM = 73,040 bytes), Z [128][64] bf16 (16,384) and
// the row scratch (7,168): 96,592 bytes.  Two such workgroups do not fit a CU's 160 KB (the siblings' two-per-CU plan
// needs <= 81,920 each and the z buffer alone takes 16 KB of the 8.9 KB that P and W leave), so ONE workgroup runs per CU;
// with 8 waves per CU the kernel is built for 2 waves per SIMD.  No hand-issued loads beyond those of the shared phases.
//
// A job e2e_refused refuses must not reach this kernel (the caller asks nm_e2e_pass_ok on the host); its workgroups leave
// at once, exports untouched.
namespace {

constexpr int E2E_ROW = NM_E2E_ROW_COLUMNS;
constexpr int E2E_ZP = NM_MAX_LATENT;                                 // pitch of z in LDS (elements)
constexpr int E2E_Z_BYTES = DV_ROWS * E2E_ZP * 2;                     // 16,384
constexpr int E2E_T_DEV = 0, E2E_T_LOGIT = NM_MAX_MOD, E2E_T_KL = NM_MAX_MOD + NM_MAX_CLASSES, E2E_T_BAD = E2E_T_KL + 1;
constexpr int E2E_TAB_COLS = E2E_T_BAD + 1;                           // 14
constexpr int E2E_TAB_BYTES = E2E_TAB_COLS * DV_ROWS * 4;             // 7,168
constexpr int E2E_SMEM = DV_SMEM + E2E_Z_BYTES + E2E_TAB_BYTES;
constexpr int E2E_MAX_CLS_WIDTH = 128;                                // the one-tile head
static_assert(E2E_SMEM == 96592 && E2E_SMEM <= 160 * 1024, "one workgroup per CU");
static_assert((DV_SMEM & 15) == 0 && (E2E_Z_BYTES & 15) == 0, "z buffer / row scratch alignment");
static_assert(E2E_ROW == 8 && NM_MAX_CLASSES == 4 && NM_MAX_MOD == 2 * NM_MAX_EXP, "row layout");
static_assert(2 * NM_MAX_LATENT <= IMG_ROWS && DV_MAX_H0 >= 110, "heads image, default first hidden width");

// gPoE reads params[mod[m].alpha] of every expert: a class that registers no alpha (the end-to-end model: offset -1) cannot
// be fused that way by ANY kernel -- the word in front of the parameter buffer need not be mapped
__host__ __device__ inline int e2e_alpha_missing(const nm_job_t* j) {
  const int Me = j->M_enc > 0 ? j->M_enc : j->M;
  if (j->combine != NM_COMBINE_GPOE || (Me == 1 && j->single_bypass)) return 0;
  for (int m = 0; m < Me && m < NM_MAX_EXP; ++m)
    if (j->mod[m].alpha < 0) return NM_E_OFFSETS;
  return 0;
}

__host__ __device__ inline int e2e_refused(const nm_job_t* j) {
  if (j->wide) return NM_E_DEVPASS;
  if (j->M_enc < 1 || j->M_enc > NM_MAX_EXP || j->M != 2 * j->M_enc) return NM_E_DEVPASS;
  if (j->n_private != 0 || j->tc_weight != 0.f || j->w_off >= 0 || j->out_kind != 0) return NM_E_DEVPASS;
  if (j->Z < 1 || j->Z > NM_MAX_LATENT || j->Z + j->C > NM_MAX_WIDTH) return NM_E_DEVPASS;
  if (j->L < 1 || j->L > NM_MAX_HID || j->H[0] > DV_MAX_H0) return NM_E_DEVPASS;
  for (int i = 0; i < j->L; ++i)
    if (j->H[i] < 1 || j->H[i] > NM_MAX_WIDTH) return NM_E_DEVPASS;
  if (j->cls_layers < 0 || j->cls_layers > NM_MAX_CLS || j->cls_classes < 2 || j->cls_classes > NM_MAX_CLASSES) return NM_E_DEVPASS;
  for (int i = 0; i < j->cls_layers; ++i)
    if (j->cls_width[i] < 1 || j->cls_width[i] > E2E_MAX_CLS_WIDTH) return NM_E_DEVPASS;
  if (e2e_alpha_missing(j)) return NM_E_DEVPASS;
  return 0;
}

// one latent column's share of -2 KL: 1 + lv - mu^2 - exp(lv), left to right
__device__ __forceinline__ float e2e_kl_term(float mu, float lv) {
#pragma clang fp contract(off)
  return ((1.0f + lv) - mu * mu) - expf(lv);
}
__device__ __forceinline__ int e2e_nonfinite(float v) { return (__float_as_uint(v) & 0x7f800000u) == 0x7f800000u ? 1 : 0; }

// build_zc with the z columns read from an LDS buffer of pitch E2E_ZP (build_zc's own LDS branch reads pitch 32)
__device__ __forceinline__ void e2e_build_zc(const Ctx& c, __bf16* dst, const nm_modality_t& md, int Z, int C, const __bf16* zsrc) {
  constexpr int ROWS = DV_ROWS;
  const int wz = wpad(Z + C);
  const float rz = 1.0f / (float)Z;
  const GAS uint16_t* cz = asg(md.cz);
  {
    const int npc = (C + 1 + 7) >> 3;
    const float rnp = 1.0f / (float)npc;
    for (int p = c.tid; p < ROWS * npc; p += WG) {
      const int r = idiv(p, npc, rnp), col0 = 8 * (p - r * npc);
      const u32x4 v = *(const GAS u32x4*)(cz + (int64_t)(c.row0 + r) * md.Cz + col0);
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
    const int r = idiv(e, Z, rz), k = e - r * Z;
    dst[r * LDP + k] = zsrc[r * E2E_ZP + k];
  }
}

// rows [live, 128) of the tile: the row table and every wanted decoder's exports come back as zeros
__device__ __forceinline__ void e2e_zero_dead_rows(int tid, const nm_job_t* J, uint32_t want, gf32 rowtab, int row0, int live) {
  for (int k = 0; k < J->M; ++k) {
    if (!((want >> k) & 1u)) continue;
    const nm_modality_t& md = J->mod[k];
    dvs_zero_dead_rows(tid, md.x_pitch, asg(md.out_loc), asg(md.out_sqerr), asg(md.out_rowdev), row0, live);
  }
  // (live = 0 only -- the empty half of a ragged batch: a live tile zeroes its own dead rows of these in its phases)
  if (live == 0) {
    const int Z = J->Z;
    for (int e = tid; e < DV_ROWS * Z; e += WG) {
      const int64_t gi = (int64_t)row0 * Z + e;
      if (J->out_mu) asg(J->out_mu)[gi] = 0.f;
      if (J->out_logvar) asg(J->out_logvar)[gi] = 0.f;
      if (J->out_z) asg(J->out_z)[gi] = 0.f;
    }
    if (J->out_logits)
      for (int e = tid; e < DV_ROWS * NM_MAX_CLASSES; e += WG) asg(J->out_logits)[(int64_t)row0 * NM_MAX_CLASSES + e] = 0.f;
  }
  if (rowtab)
    for (int r = live + tid; r < DV_ROWS; r += WG) {
#pragma unroll
      for (int i = 0; i < E2E_ROW; i += 4) *(GAS f32x4*)(rowtab + (int64_t)(row0 + r) * E2E_ROW + i) = f32x4{0.f, 0.f, 0.f, 0.f};
    }
}

// the row's eight numbers from its words of the row scratch (nmhip.h: the definition, in this order of operations)
__device__ __forceinline__ void e2e_row_fold(const float* tab, int r, int C, int Me, f32x4& lo, f32x4& hi) {
#pragma clang fp contract(off)
  constexpr int ROWS = DV_ROWS;
  float l[NM_MAX_CLASSES];
#pragma unroll
  for (int k = 0; k < NM_MAX_CLASSES; ++k) l[k] = tab[(E2E_T_LOGIT + k) * ROWS + r];
  float mx = l[0], top = l[0], mxd = l[1];
  int pred = 0;
#pragma unroll
  for (int k = 1; k < NM_MAX_CLASSES; ++k) {
    if (k < C) {
      mx = fmaxf(mx, l[k]);
      if (l[k] > top) { top = l[k]; pred = k; }
      if (k > 1) mxd = fmaxf(mxd, l[k]);
    }
  }
  float e[NM_MAX_CLASSES];
#pragma unroll
  for (int k = 0; k < NM_MAX_CLASSES; ++k) e[k] = k < C ? expf(l[k] - mx) : 0.f;
  float sd = e[1], sa = e[0] + e[1];
#pragma unroll
  for (int k = 2; k < NM_MAX_CLASSES; ++k)
    if (k < C) { sd = sd + e[k]; sa = sa + e[k]; }
  int st = tab[E2E_T_BAD * ROWS + r] != 0.f ? 1 : 0;
#pragma unroll
  for (int k = 0; k < NM_MAX_CLASSES; ++k) st |= k < C ? e2e_nonfinite(l[k]) : 0;
  float dh = 0.f, dd = 0.f;
  for (int m = 0; m < Me; ++m) {
    const float h = tab[(E2E_T_DEV + m) * ROWS + r], d = tab[(E2E_T_DEV + Me + m) * ROWS + r];
    dh = m ? dh + h : h;
    dd = m ? dd + d : d;
    st |= e2e_nonfinite(h) | e2e_nonfinite(d);
  }
  dh = dh / (float)Me;
  dd = dd / (float)Me;
  lo = f32x4{sd / sa, (float)pred, mxd - l[0], dh};
  hi = f32x4{dd, dh - dd, tab[E2E_T_KL * ROWS + r], st ? 1.0f : 0.0f};
}

__global__ __launch_bounds__(WG, 2) void nm_e2e_kernel(const nm_job_t* __restrict__ jobs, const nm_e2e_t* __restrict__ reqs, int tile0,
                                                         int flags) {
  constexpr int RT = DV_RT, ROWS = DV_ROWS, WROWS = DV_RT * 16;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const nm_job_t* J = jobs + blockIdx.x;
  if (e2e_refused(J) || !J->workspace) return;
  const nm_e2e_t& rq = reqs[blockIdx.x];
  const int Me = J->M_enc, M = J->M;
  gf32 const rowtab = asg(rq.row);
  const uint32_t want = (uint32_t)rq.want_mask & ((1u << M) - 1u);
  const int t128 = tile0 + (int)blockIdx.y;
  const int row0 = t128 * ROWS;
  if (row0 >= J->n_rows) {
    // the second half of a ragged last 256-row tile: the export rows come back as zeros
    if (row0 < (J->n_rows + TROWS - 1) / TROWS * TROWS) e2e_zero_dead_rows((int)threadIdx.x, J, want, rowtab, row0, 0);
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
  for (int i = c.tid; i < E2E_SMEM / 4; i += WG) reinterpret_cast<uint32_t*>(smem)[i] = 0u;
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
  float* const tab = reinterpret_cast<float*>(smem + DV_SMEM + E2E_Z_BYTES);      // [E2E_TAB_COLS][128]
  const WsLayout wl = ws_layout(M, L, Z);
  // this workgroup's rows of the batch's expert statistics; expert m at + m * 256 * Zs
  gf32 ws_mu_m = (gf32)(c.ws + wl.mu_m) + c.rloc0 * Zs;
  gf32 ws_lv_m = (gf32)(c.ws + wl.lv_m) + c.rloc0 * Zs;
  auto to_W = [&](const GAS char* blob, int vs, int rows, int K) {
    return Next{blob, Wb, IMG_BYTES >> 10, blob + cimg_bytes(rows, K), reinterpret_cast<char*>(c.vec) + vs * VEC_BYTES, rows, blob_kp(K)};
  };

  // ---- encoders: every expert's chain, statistics to the workspace ----
  for (int m = 0; m < Me; ++m) {
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

  // ---- fusion, the latent, the classifier's input: z -> LDS, bf16(mu or z) -> P; four lanes per row ----
  handoff_barrier();                               // the heads' stores are complete for every thread of the workgroup
  {
    float al[NM_MAX_EXP] = {0.f, 0.f, 0.f, 0.f};
    if (J->combine == NM_COMBINE_GPOE && !(Me == 1 && J->single_bypass)) softmax_alpha(J, al);
    relaunder(c);
    const int r = c.tid >> 2, sub = c.tid & 3;
    const bool rv = r < c.nrows;
    const bool mean_z = rq.use_mean != 0, cmu = J->cls_use_mu != 0;
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
          if (m < Me) {
            mu4[m] = *(const GAS f32x4*)(ws_mu_m + ((int64_t)m * TROWS + r) * Zs + z0);
            lv4[m] = *(const GAS f32x4*)(ws_lv_m + ((int64_t)m * TROWS + r) * Zs + z0);
          }
        }
        float ep[4] = {0.f, 0.f, 0.f, 0.f};
        if (!mean_z) {
          if (J->eps) {
#pragma unroll
            for (int i = 0; i < 4; ++i) ep[i] = asg(J->eps)[eprow + z0 + i];
          } else {
            randn2_ctr(J->seed, (uint32_t)step, (uint32_t)(c.row0 + r), (uint32_t)(z0 >> 1), ep[0], ep[1]);
            randn2_ctr(J->seed, (uint32_t)step, (uint32_t)(c.row0 + r), (uint32_t)(z0 >> 1) + 1u, ep[2], ep[3]);
          }
        }
        f32x4 omu, olv, oz;
        bf16x4 zk, ck;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          Lat Lt;
#pragma unroll
          for (int m = 0; m < NM_MAX_EXP; ++m) { Lt.mu[m] = mu4[m][i]; Lt.lv[m] = lv4[m][i]; }
          const Fuse f = fuse_fwd(J, Lt, al);
          const float es = ep[i] * fx_exp(0.5f * f.lv);
          const float zz = mean_z ? f.mu : dvm_add(f.mu, es);
          omu[i] = f.mu; olv[i] = f.lv; oz[i] = zz;
          klp += e2e_kl_term(f.mu, f.lv);
          bad |= e2e_nonfinite(f.mu) | e2e_nonfinite(f.lv);
          zk[i] = (__bf16)zz;
          ck[i] = (__bf16)(rv ? (cmu ? f.mu : zz) : 0.f);
        }
        *reinterpret_cast<bf16x4*>(zlds + r * E2E_ZP + z0) = zk;
        *reinterpret_cast<bf16x4*>(c.P + r * LDP + z0) = ck;
        if (!rv) { omu = f32x4{0.f, 0.f, 0.f, 0.f}; olv = omu; oz = omu; }      // (rows past the table: zeros)
        if (J->out_mu) *(GAS f32x4*)(asg(J->out_mu) + grow + z0) = omu;
        if (J->out_logvar) *(GAS f32x4*)(asg(J->out_logvar) + grow + z0) = olv;
        if (J->out_z) *(GAS f32x4*)(asg(J->out_z) + grow + z0) = oz;
      }
    } else {
      for (int z = sub; z < Z; z += 4) {
        Lat Lt;
#pragma unroll
        for (int m = 0; m < NM_MAX_EXP; ++m) {
          Lt.mu[m] = (m < Me) ? ws_mu_m[((int64_t)m * TROWS + r) * Zs + z] : 0.f;
          Lt.lv[m] = (m < Me) ? ws_lv_m[((int64_t)m * TROWS + r) * Zs + z] : 0.f;
        }
        const Fuse f = fuse_fwd(J, Lt, al);
        float ep = 0.f;
        if (!mean_z) ep = J->eps ? asg(J->eps)[eprow + z] : randn_ctr(J->seed, (uint32_t)step, (uint32_t)(c.row0 + r), (uint32_t)z);
        const float es = ep * fx_exp(0.5f * f.lv);
        const float zz = mean_z ? f.mu : dvm_add(f.mu, es);
        klp += e2e_kl_term(f.mu, f.lv);
        bad |= e2e_nonfinite(f.mu) | e2e_nonfinite(f.lv);
        zlds[r * E2E_ZP + z] = (__bf16)zz;
        c.P[r * LDP + z] = (__bf16)(rv ? (cmu ? f.mu : zz) : 0.f);
        if (J->out_mu) asg(J->out_mu)[grow + z] = rv ? f.mu : 0.f;         // (rows past the table: zeros)
        if (J->out_logvar) asg(J->out_logvar)[grow + z] = rv ? f.lv : 0.f;
        if (J->out_z) asg(J->out_z)[grow + z] = rv ? zz : 0.f;
      }
    }
    // the row's KL and flag: the four lanes' shares, always in the same order
    klp += __shfl_xor(klp, 1, 64);
    klp += __shfl_xor(klp, 2, 64);
    bad |= __shfl_xor(bad, 1, 64);
    bad |= __shfl_xor(bad, 2, 64);
    if (sub == 0) {
      tab[E2E_T_KL * ROWS + r] = rv ? -0.5f * klp : 0.f;
      tab[E2E_T_BAD * ROWS + r] = (rv && bad) ? 1.0f : 0.f;
    }
    // the classifier reads K rounded up to 32 columns: zeros behind the latent
    const int npad = rup(Z, 32) - Z;
    if (npad > 0) {
      const float rnp = 1.0f / (float)npad;
      for (int e = c.tid; e < ROWS * npad; e += WG) {
        const int rr = idiv(e, npad, rnp);
        c.P[rr * LDP + Z + (e - rr * npad)] = (__bf16)0.0f;
      }
    }
  }
  lds_barrier();                                   // z, the classifier's input and the row's KL are complete
  tr(c, 3);

  // ---- classifier, eval mode (cls_head_body's forward: K order and bias-in-accumulator form kept) ----
  {
    const int Lc = J->cls_layers, NC = J->cls_classes;
    gcf32 prm = asg(J->params);
    f32x4 acc[2][RT];
    for (int li = 0; li < Lc; ++li) {
      relaunder(c);
      const int K = li == 0 ? Z : J->cls_width[li - 1], N = J->cls_width[li], K32 = rup(K, 32);
      gcf32 Wl = prm + J->cls_w[li];
      WBlk<128> wb;
      wblk_load<128>(c, wb, Wl, N, K, 0, 0);
      float mean[2][4], rstd[2][4], gam[2][4], bet[2][4];
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int fc = min((c.wn + 4 * t) * 16 + 4 * c.g + i, N - 1);
          gam[t][i] = prm[J->cls_bn_w[li] + fc];
          bet[t][i] = prm[J->cls_bn_b[li] + fc];
          mean[t][i] = prm[J->cls_bn_mean[li] + fc];
          const float var = prm[J->cls_bn_var[li] + fc];
          rstd[t][i] = 1.0f / sqrtf(var + 1e-5f);
        }
      bias_acc(c, acc, prm + J->cls_b[li], N, 0);
      wblk_store<128>(c, wb, c.Q, LDP, N, K, 0, 0);
      lds_barrier();
      for (int ks = 0; ks < K32 / 32; ++ks) {
        bf16x8 wf[2];
#pragma unroll
        for (int t = 0; t < 2; ++t) wf[t] = lds_frag(c.Q, LDP, (c.wn + 4 * t) * 16 + c.c16, ks * 32 + 8 * c.g);
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) {
          bf16x8 a = lds_frag(c.P, LDP, c.wm * WROWS + rt * 16 + c.c16, ks * 32 + 8 * c.g);
#pragma unroll
          for (int t = 0; t < 2; ++t) acc[t][rt] = mfma(wf[t], a, acc[t][rt]);
        }
      }
      lds_barrier();                               // P and W fully read
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        const int f0 = (c.wn + 4 * t) * 16 + 4 * c.g;
        if (f0 >= rup(N, 32)) continue;
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) {
          const int r = c.wm * WROWS + rt * 16 + c.c16;
          f32x4 xh;
          bf16x4 pk;
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            xh[i] = (acc[t][rt][i] - mean[t][i]) * rstd[t][i];
            const float h = fmaxf(gam[t][i] * xh[i] + bet[t][i], 0.f);
            pk[i] = (__bf16)((f0 + i < N && r < c.nrows) ? h : 0.f);
          }
          *reinterpret_cast<bf16x4*>(c.P + r * LDP + f0) = pk;
        }
      }
      lds_barrier();
    }
    relaunder(c);
    const int Kl = Lc ? J->cls_width[Lc - 1] : Z, Kl32 = rup(Kl, 32);
    gcf32 Wo = prm + J->cls_w[Lc];
    bias_acc(c, acc, prm + J->cls_b[Lc], NC, 0);
    for (int ks = 0; ks < Kl32 / 32; ++ks) {
      bf16x8 wf[2];
#pragma unroll
      for (int t = 0; t < 2; ++t) wf[t] = w_frag(Wo, NC, Kl, (c.wn + 4 * t) * 16 + c.c16, ks * 32 + 8 * c.g);
#pragma unroll
      for (int rt = 0; rt < RT; ++rt) {
        bf16x8 a = lds_frag(c.P, LDP, c.wm * WROWS + rt * 16 + c.c16, ks * 32 + 8 * c.g);
#pragma unroll
        for (int t = 0; t < 2; ++t) acc[t][rt] = mfma(wf[t], a, acc[t][rt]);
      }
    }
    if (c.wn == 0 && c.g == 0) {                   // these lanes hold logits 0..3 of their rows
#pragma unroll
      for (int rt = 0; rt < RT; ++rt) {
        const int r = c.wm * WROWS + rt * 16 + c.c16;
        const bool rvl = r < c.nrows;
        f32x4 lg;
#pragma unroll
        for (int k = 0; k < NM_MAX_CLASSES; ++k) {
          lg[k] = (rvl && k < NC) ? acc[0][rt][k] : 0.f;                   // (rows past the table: zeros)
          tab[(E2E_T_LOGIT + k) * ROWS + r] = lg[k];
        }
        if (J->out_logits) *(GAS f32x4*)(asg(J->out_logits) + (int64_t)(c.row0 + r) * NM_MAX_CLASSES) = lg;
      }
    }
  }
  tr(c, 26);

  // ---- decoders: both banks ----
  const int Hl = J->H[0];
  const int ob = L & 1;                            // (see nm_devpass_kernel: chunk 0's vectors avoid the last hidden layer's bias)
  for (int m = 0; m < M; ++m) {
    relaunder(c);
    const nm_modality_t& md = J->mod[m];
    const bool wanted = ((want >> m) & 1u) != 0u;
    gf32 const oloc = wanted ? asg(md.out_loc) : (gf32)nullptr;
    gf32 const osq = wanted ? asg(md.out_sqerr) : (gf32)nullptr;
    gf32 const ordv = wanted ? asg(md.out_rowdev) : (gf32)nullptr;
    if (!rowtab && !oloc && !osq && !ordv) continue;          // nothing of this decoder is wanted
    const int D = md.D;
    lds_barrier();                                 // the classifier / the previous decoder is finished everywhere: P, W, vectors free
    issue_next(c, to_W(wsh + md.dec_s[0], 0, J->H[L - 1], Z + C));
    e2e_build_zc(c, c.P, md, Z, C, zlds);
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
    if (wave_live) {                                // the row's four column groups sit in the lanes c16, c16 + 16, + 32, + 48
      float v = rdev;
      v += __shfl_xor(v, 16, 64);
      v += __shfl_xor(v, 32, 64);
      const float dvr = v / (float)D;
      if (c.g == 0 && orow < c.nrows) {
        tab[(E2E_T_DEV + m) * ROWS + orow] = dvr;
        if (ordv) ordv[row0 + orow] = dvr;
      }
    }
    // (a ragged tile only: the rows no wave has stored)
    if (live < ROWS) { relaunder(c); dvs_zero_dead_rows(c.tid, xp, oloc, osq, ordv, row0, live); }
    tr(c, 8);
  }

  // ---- the row table: thread r owns row r ----
  if (!rowtab) return;
  lds_barrier();                                   // every lane's words of the row scratch are in place
  relaunder(c);
  if (c.tid < ROWS) {
    const int r = c.tid;
    f32x4 lo = {0.f, 0.f, 0.f, 0.f}, hi = lo;
    if (r < c.nrows) e2e_row_fold(tab, r, J->cls_classes, Me, lo, hi);
    gf32 orw = rowtab + (int64_t)(row0 + r) * E2E_ROW;
    *(GAS f32x4*)orw = lo;
    *(GAS f32x4*)(orw + 4) = hi;
  }
}

}  // namespace

extern "C" {

/* 0: the job's evaluation can run on nm_e2e_pass (nmhip.h states the domain); NM_E_DEVPASS otherwise. */
int nm_e2e_pass_ok(const nm_job_t* j) {
  if (!j) return NM_E_NULL;
  return e2e_refused(j);
}

/* NM_E_OFFSETS: the job asks for gPoE and an expert has no alpha offset (mod[m].alpha < 0) -- neither nm_e2e_pass nor the
 * two-launch route (nm_forward reads params[alpha] likewise) can evaluate it; 0 otherwise. */
int nm_e2e_alpha_ok(const nm_job_t* j) {
  if (!j) return NM_E_NULL;
  return e2e_alpha_missing(j);
}

/* The end-to-end model's evaluation pass over table rows [tile0 * 128, (tile0 + n_tiles) * 128).  Status is decided here, on
 * the host, before the device is asked anything -- the descriptors and the requests live in device memory: every job must
 * pass nm_e2e_pass_ok, asked by the caller while the descriptor is still on the host.  Workspace tiles as for
 * nm_devpass_multi. */
int nm_e2e_pass(const nm_job_t* jobs_dev, int n_jobs, const nm_e2e_t* req_dev, int tile0, int n_tiles, int flags, void* stream) {
  if (!jobs_dev || !req_dev) return NM_E_NULL;
  if (int bad = check_launch_geometry(jobs_dev, n_jobs, n_tiles, 1, tile0, 0)) return bad;
  return launch_kernel(nm_e2e_kernel, dim3(n_jobs, n_tiles), dim3(WG), E2E_SMEM, stream, jobs_dev, req_dev, tile0, flags & NM_F_TRACE);
}

}  // extern "C"
