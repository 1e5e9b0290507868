// ---------------------------------------------------------------------------------------------------------------------
// nm_devpass_iw_kernel -- the likelihood pass: nm_devpass_draws_kernel's shape with the importance weight of every draw in
// the place of the fold of the reconstructions (nmhip.h states the definition).  Encoders once per tile, statistics to
// the workspace tile; then per draw s the fusion, the draw under (seed_s | eps_s) and every wanted decoder, exactly as
// there.  The sources of the kernels above stay as they are (this file is included at the end of nm_devpass.hip): the
// draw loop and the decoder loop are repeated here with the likelihood sum in the place of the accumulator traffic.
//
// What a row needs lives in the registers of the lane that owns it in the output phase (g == 0, row orow = 16 wave +
// c16), across the decoder loop and the draw loop: no buffer holds state between the draws, no atomics, no [N, D] export.
//   latent term   a_s = -0.5 sum_k (z_k^2 - eps_k^2 - lv_k): lane (c16, g) of the row's wave recomputes the terms of the
//                 columns k = 8 g .. 8 g + 7 from the workspace statistics (fuse_fwd) and the draw (the generator call or
//                 the injected value the z phase uses), the owning lane takes them with 32 shuffles and adds them in
//                 ascending k.  No LDS beyond the draws kernel's plan.
//   likelihood    q_m = sum_d (x_d - x_hat_d)^2 / noise_var_d in the chunk epilogue (dvd_sum4 per four columns, the two
//                 __shfl_xor at the decoder's end: pred_rowz2's pattern), ll_m = ll_const[m] - 0.5 q_m.
//   fold          online log-sum-exp (mx, s1, s2) and running sums, in draw order, with the library's expf / logf.
// The chunk boundary keeps the draws kernel's full wait (wait_vm(0)): the x and noise_var loads are vector-memory
// operations of their own in the same queue as the weight images.
//
// Geometry, LDS plan and workspace tile: nm_devpass_draws_kernel's.  A job dvd_refused refuses, or a request whose row
// pointer is missing or whose mask is empty, must not reach this kernel (nm_iw_check on the host); its workgroups leave
// at once, exports untouched.
namespace {

constexpr int IW_ROW = NM_IW_ROW_COLUMNS;

__host__ __device__ inline int iw_refused(const nm_job_t* j) { return lat_refused(j); }

// the owning lane's view of 4 x 8 per-column terms held by the lanes (c16, g = 0..3): their sum in ascending column order
__device__ __forceinline__ float iw_gather_sum(const float (&t)[8], int c16) {
#pragma clang fp contract(off)
  float s = 0.f;
#pragma unroll
  for (int gg = 0; gg < 4; ++gg) {
#pragma unroll
    for (int i = 0; i < 8; ++i) s = s + __shfl(t[i], c16 + 16 * gg, 64);
  }
  return s;
}
__device__ __forceinline__ float iw_latent_term(float z, float ep, float lv) {
#pragma clang fp contract(off)
  return (z * z - ep * ep) - lv;
}
__device__ __forceinline__ float iw_kl_term(float mu, float lv) {
#pragma clang fp contract(off)
  return mu * mu + (expm1f(lv) - lv);             // exp(lv) - 1 without the cancellation near lv = 0
}
__device__ __forceinline__ float iw_q4(const f32x4& x, const f32x4& xh, const f32x4& nv, bool rv, int dg0, int D) {
#pragma clang fp contract(off)
  f32x4 t;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const float e = x[i] - xh[i];
    t[i] = (rv && dg0 + i < D) ? (e * e) / nv[i] : 0.f;
  }
  return dvd_sum4(t);
}
__device__ __forceinline__ float iw_ll(float llc, float q) {
#pragma clang fp contract(off)
  return llc - 0.5f * q;
}

// rows [live, 128) of the tile: the row export and every wanted decoder's recon_ll come back as zeros
__device__ __forceinline__ void iw_zero_dead_rows(int tid, const nm_iw_t& q, int M, int row0, int live) {
  gf32 orow = asg(q.row);
  for (int r = live + tid; r < DV_ROWS; r += WG) {
#pragma unroll
    for (int i = 0; i < IW_ROW; i += 4) *(GAS f32x4*)(orow + (int64_t)(row0 + r) * IW_ROW + i) = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int m = 0; m < M; ++m)
      if (((q.dec_mask >> m) & 1u) && q.recon_ll[m]) asg(q.recon_ll[m])[row0 + r] = 0.f;
  }
}

__global__ __launch_bounds__(WG, 4) void nm_devpass_iw_kernel(const nm_job_t* __restrict__ jobs, const nm_draw_t* __restrict__ draws,
                                                                int n_draws, const nm_iw_t* __restrict__ iws, int tile0, int flags) {
  constexpr int RT = DV_RT, ROWS = DV_ROWS;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const nm_job_t* J = jobs + blockIdx.x;
  if (iw_refused(J) || !J->workspace || n_draws < 1 || n_draws > NM_MAX_IW_DRAWS) return;
  const nm_draw_t* const drs = draws + (int64_t)blockIdx.x * n_draws;
  const nm_iw_t& iq = iws[blockIdx.x];
  const int M = J->M;
  const uint32_t dmask = iq.dec_mask & ((1u << M) - 1u);
  if (!iq.row || !dmask) return;
  const int t128 = tile0 + (int)blockIdx.y;
  const int row0 = t128 * ROWS;
  if (row0 >= J->n_rows) {
    // the second half of a ragged last 256-row tile: the export rows come back as zeros
    if (row0 < (J->n_rows + TROWS - 1) / TROWS * TROWS) iw_zero_dead_rows((int)threadIdx.x, iq, M, row0, 0);
    return;
  }
  const int mf = __builtin_ctz(dmask);             // the first decoder that is wanted
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

  const int Hl = J->H[0];
  const int ob = L & 1;                            // (see nm_devpass_kernel: chunk 0's vectors avoid the last hidden layer's bias)
  const int orow = c.wave * 16 + c.c16;            // the row this lane's output-phase values belong to
  const bool wave_live = c.wave * 16 < live;
  const bool rv = orow < c.nrows;
  const bool owner = c.g == 0 && rv;
  const int k0 = 8 * c.g;                          // this lane's latent columns of row orow: k0 .. k0 + 7

  // the fused statistics of column k0 + i of row orow, as the z phase computes them
  // (the lane's row and first column are laundered where they are used: what the compiler derives from them -- addresses,
  //  generator keys, clamped indices -- would otherwise be hoisted out of the draw loop and held across the decoders, whose
  //  layers need every register)
  auto fused = [&](int rr, int k, const float (&al)[NM_MAX_EXP]) {
    const uint32_t fo = (uint32_t)(rr * Zs + k);
    Lat Lt;
#pragma unroll
    for (int m = 0; m < NM_MAX_EXP; ++m) {
      Lt.mu[m] = (m < M) ? (ws_mu_m + m * TROWS * Zs)[fo] : 0.f;
      Lt.lv[m] = (m < M) ? (ws_lv_m + m * TROWS * Zs)[fo] : 0.f;
    }
    return fuse_fwd(J, Lt, al);
  };

  // ---- the analytic KL of the row, once (the posterior does not depend on the draw) ----
  float kl = 0.f;
  if (wave_live) {
    float al[NM_MAX_EXP] = {0.f, 0.f, 0.f, 0.f};
    if (J->combine == NM_COMBINE_GPOE && !byp) softmax_alpha(J, al);
    float t[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      t[i] = 0.f;
      if (k0 + i < Z) { const Fuse f = fused(orow, k0 + i, al); t[i] = iw_kl_term(f.mu, f.lv); }
    }
    kl = 0.5f * iw_gather_sum(t, c.c16);
  }

  // the fold's state: owned by lane (c16, g == 0), kept by every lane of the wave (the shuffles run wave-wide)
  float mx = 0.f, s1 = 0.f, s2 = 0.f, sum_lw = 0.f, sum_a = 0.f, sum_rec = 0.f, lw_max = 0.f, lw_min = 0.f;
  float sum_ll[NM_MAX_EXP] = {0.f, 0.f, 0.f, 0.f};

  // ---- the draws: fusion + draw s -> LDS, the row's latent term, then every wanted decoder with its likelihood sum ----
  for (int s = 0; s < n_draws; ++s) {
    relaunder(c);
    const uint64_t seed = drs[s].seed;
    const GAS float* const epsp = asg(drs[s].eps);
    if (s > 0) lds_barrier();                      // the previous draw's last chunk is finished everywhere: P, W, vectors, Z free
    // W and P are free: the first decoder's image lands during the latent arithmetic
    issue_next(c, to_W(wsh + J->mod[mf].dec_s[0], 0, J->H[L - 1], Z + C));
    float a_s = 0.f;
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
      // the latent term of row orow: the fp32 z of the z phase, recomputed by the row's own wave (its draw comes from the same
      // generator call -- the pair generator when Z is a multiple of 4, the scalar one otherwise -- or the same injected value)
      if (wave_live) {
        int rr = orow, kk = k0;
        asm volatile("" : "+v"(rr), "+v"(kk));
        float t[8];
#pragma unroll
        for (int i = 0; i < 8; i += 2) {
          float ep[2] = {0.f, 0.f};
          if (kk + i < Z) {
            if (epsp) {
#pragma unroll
              for (int u = 0; u < 2; ++u)
                ep[u] = epsp[((int64_t)(step % J->eps_cap) * TROWS + c.rloc0 + rr) * Z + min(kk + i + u, Z - 1)];
            } else if (vec4) {
              randn2_ctr(seed, (uint32_t)step, (uint32_t)(c.row0 + rr), (uint32_t)((kk + i) >> 1), ep[0], ep[1]);
            } else {
              ep[0] = randn_ctr(seed, (uint32_t)step, (uint32_t)(c.row0 + rr), (uint32_t)(kk + i));
              ep[1] = randn_ctr(seed, (uint32_t)step, (uint32_t)(c.row0 + rr), (uint32_t)(kk + i + 1));
            }
          }
#pragma unroll
          for (int u = 0; u < 2; ++u) {
            t[i + u] = 0.f;
            if (kk + i + u < Z) {
              const Fuse f = fused(rr, kk + i + u, al);
              float zf;
              if (byp) {
                zf = dvd_z_bypass(f.mu, ep[u], f.lv);
              } else {
                const float es = ep[u] * fx_exp(0.5f * f.lv);
                zf = dvm_add(f.mu, es);
              }
              t[i + u] = iw_latent_term(zf, ep[u], f.lv);
            }
          }
        }
        a_s = -0.5f * iw_gather_sum(t, c.c16);
      }
    }
    lds_barrier();                                 // z is complete (the decoder image requested above stays in flight)
    tr(c, 3);

    float rec = 0.f;                               // sum over the wanted decoders, ascending m, of ll_m of this draw
    for (int m = mf; m < M; ++m) {
      relaunder(c);
      if (!((dmask >> m) & 1u)) continue;          // (workgroup-uniform) this decoder is not wanted: skipped entirely
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
      gcf32 nvp = asg(iq.noise_var[m]);
      const int xp = md.x_pitch;
      float q = 0.f;
      auto load_xin = [&](int chx, f32x4 (&xv)[4]) {
#pragma unroll
        for (int ft = 0; ft < 4; ++ft) {
          const int dcl = min(chx * OCH + ft * 16 + 4 * c.g, xp - 4);
          xv[ft] = *(const GAS f32x4*)(xf + (int64_t)(row0 + orow) * xp + dcl);
        }
      };
      auto chunk = [&](const int ch) {
        relaunder(c);
        const int d0 = ch * OCH;
        const __bf16* Wc = reinterpret_cast<const __bf16*>(Wb + (ch & 1) * OIMG_BYTES);
        const float* vb = c.vec + ((ch + ob) & 1) * (VEC_BYTES / 4);
        // chunk ch's rows, vectors and inputs have landed, and everything else this wave has in flight with them (a full
        // wait, not a count: the x and noise_var loads share the queue)
        wait_vm(0);
        lds_barrier();
        if (ch + 1 < nck) issue_next(c, out_blob(ch + 1));
        if (!wave_live) return;
        f32x4 xin[4];                               // (x is needed in every draw: requested ahead of the MFMAs, used after them)
        load_xin(ch, xin);
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
          if (d0 + ft * 16 < xp && dg0 < xp) {          // (the first: wave-uniform)
            const f32x4 nv4 = *(const GAS f32x4*)(nvp + min(dg0, xp - 4));
            f32x4 xh;
#pragma unroll
            for (int i = 0; i < 4; ++i) xh[i] = acc[ft][i] + bo[i];
            q += iw_q4(xin[ft], xh, nv4, rv, dg0, D);
          }
        }
        tr(c, 7);
      };
      for (int ch = 0; ch < nck; ++ch) chunk(ch);
      if (wave_live) {                              // the row's four column groups sit in the lanes c16, c16 + 16, + 32, + 48
        q += __shfl_xor(q, 16, 64);
        q += __shfl_xor(q, 32, 64);
        const float ll = iw_ll(iq.ll_const[m], q);
        rec += ll;
#pragma unroll
        for (int mm = 0; mm < NM_MAX_EXP; ++mm)
          if (mm == m) sum_ll[mm] += ll;
      }
      tr(c, 8);
    }

    // ---- the fold of draw s, in the registers of the row's lanes ----
    {
      const float lw = rec + a_s;
      if (s == 0) {
        mx = lw; s1 = 1.0f; s2 = 1.0f; lw_max = lw; lw_min = lw;
      } else {
        if (lw > mx) {
          const float sc = expf(mx - lw);
          s1 = s1 * sc + 1.0f;
          s2 = s2 * (sc * sc) + 1.0f;
          mx = lw;
        } else {
          const float e = expf(lw - mx);
          s1 += e;
          s2 += e * e;
        }
        lw_max = fmaxf(lw_max, lw);
        lw_min = fminf(lw_min, lw);
      }
      sum_lw += lw;
      sum_a += a_s;
      sum_rec += rec;
    }
  }

  // ---- exports: eight values per row, and the per-decoder reconstruction term where asked ----
  if (owner) {
#pragma clang fp contract(off)
    const float fS = (float)n_draws;
    f32x4 lo, hi;
    lo[0] = (mx + logf(s1)) - logf(fS);
    lo[1] = sum_lw / fS;
    lo[2] = (s1 * s1) / s2;
    lo[3] = -(sum_a / fS);
    hi[0] = kl;
    hi[1] = sum_rec / fS;
    hi[2] = lw_max;
    hi[3] = lw_min;
    gf32 orw = asg(iq.row) + (int64_t)(row0 + orow) * IW_ROW;
    *(GAS f32x4*)orw = lo;
    *(GAS f32x4*)(orw + 4) = hi;
#pragma unroll
    for (int mm = 0; mm < NM_MAX_EXP; ++mm)
      if (mm < M && ((dmask >> mm) & 1u) && iq.recon_ll[mm]) asg(iq.recon_ll[mm])[row0 + orow] = sum_ll[mm] / fS;
  }
  // (a ragged tile only: the rows no lane owns)
  if (live < ROWS) { relaunder(c); iw_zero_dead_rows(c.tid, iq, M, row0, live); }
}

}  // namespace

extern "C" {

/* 0: the job can run the likelihood pass: the posterior-predictive pass's domain (nm_devpass_draws_ok); NM_E_DEVPASS
 * otherwise. */
int nm_devpass_iw_ok(const nm_job_t* j) {
  if (!j) return NM_E_NULL;
  return iw_refused(j);
}

/* One job's request against its descriptor, both on the host, before either is copied to the device: NM_E_NULL for a
 * missing pointer, a row export that is NULL or a wanted decoder without noise_var; NM_E_GEOMETRY for an empty decoder
 * mask or a bit at or above M; NM_E_DEVPASS for a job outside the pass's domain. */
int nm_iw_check(const nm_job_t* j, const nm_iw_t* q) {
  if (!j || !q) return NM_E_NULL;
  if (int bad = iw_refused(j)) return bad;
  if (!q->row) return NM_E_NULL;
  if (q->dec_mask == 0u || (q->dec_mask >> j->M) != 0u) return NM_E_GEOMETRY;
  for (int m = 0; m < j->M; ++m)
    if (((q->dec_mask >> m) & 1u) && !q->noise_var[m]) return NM_E_NULL;
  return NM_OK;
}

/* The likelihood pass over table rows [tile0 * 128, (tile0 + n_tiles) * 128): encoders once per tile, then n_draws times the
 * fusion, the draw of draws_dev[job][s] and every decoder of iw_dev[job]'s mask, the importance weights folded per row
 * (nmhip.h).  Status is decided here, on the host, before the device is asked anything -- the tables and the descriptors
 * live in device memory: the per-job rules are nm_iw_check's, asked by the caller of every request while it is still on
 * the host.  Workspace tiles as for nm_devpass_multi, one-expert jobs included. */
int nm_devpass_iw(const nm_job_t* jobs_dev, int n_jobs, const nm_draw_t* draws_dev, int n_draws, const nm_iw_t* iw_dev,
                  int tile0, int n_tiles, int flags, void* stream) {
  if (!jobs_dev || !draws_dev || !iw_dev) return NM_E_NULL;
  if (n_draws < 1 || n_draws > NM_MAX_IW_DRAWS) return NM_E_GEOMETRY;
  if (int bad = check_launch_geometry(jobs_dev, n_jobs, n_tiles, 1, tile0, 0)) return bad;
  return launch_kernel(nm_devpass_iw_kernel, dim3(n_jobs, n_tiles), dim3(WG), DVD_SMEM, stream, jobs_dev, draws_dev, n_draws,
                       iw_dev, tile0, flags & NM_F_TRACE);
}

}  // extern "C"
