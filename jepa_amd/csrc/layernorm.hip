// LayerNorm forward/backward (row per wave, fp32 statistics), what is left of it when it is folded into the consuming Linear, and
// the fused target path h = F.layer_norm(norm(x))[masks_pred] of the V-JEPA step.
//
// Reference behaviour restated (never copied):
//   nn.LayerNorm(eps=1e-6) in every Block / final norm   src/models/vision_transformer.py:252-281, modules.py:97,106
//   h = F.layer_norm(target_encoder(c)) ; apply_masks    app/vjepa/train.py:424-428
#include "common.hpp"
#include "options.hpp"
#include "internal.hpp"

#define LN_MAX_CHUNKS 4  // D <= 2048, D % 8 == 0: each lane owns up to 4 chunks of 8 columns

// the D every kernel here takes; -1 with the error set otherwise (`rule`: the entry points whose message has always stated the rule)
static int ln_check_D(const char* who, int64_t D, bool rule = false) {
  VJ_CHECK_ARG(D % 8 == 0 && D <= 512 * LN_MAX_CHUNKS, rule ? "%s: D=%ld unsupported (need D%%8==0, D<=%d)" : "%s: D=%ld unsupported", who,
               (long)D, 512 * LN_MAX_CHUNKS);
  return 0;
}
static inline int ln_grid(int64_t rows) { return rows_grid(rows, 256 * 8); }

// THE two-pass fp32 row statistics of every kernel here that normalises.  Lane l holds columns l*8 + i*512 .. +7 of the row in v[i];
// chunks at or past D are never touched.  ln_row_mean<true> also loads the row from xp into v, inside the same `c < D` as the sum (a load
// loop of its own costs the dead chunks a zero-fill); <false> takes v as it is.  ln_row_rstd: from the variance of the centred values, no
// E[x^2] - mean^2 cancellation.
template <bool LOAD>
__device__ __forceinline__ float ln_row_mean(const bf16_t* xp, float (&v)[LN_MAX_CHUNKS][8], int lane, int D, float invD) {
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < LN_MAX_CHUNKS; i++) {
    const int c = lane * 8 + i * 512;
    if (c < D) {
      if constexpr (LOAD) load8(xp + c, v[i]);
#pragma unroll
      for (int j = 0; j < 8; j++) s += v[i][j];
    }
  }
  return wave_sum(s) * invD;
}
__device__ __forceinline__ float ln_row_rstd(const float (&v)[LN_MAX_CHUNKS][8], float mean, int lane, int D, float invD, float eps) {
  float q = 0.f;
#pragma unroll
  for (int i = 0; i < LN_MAX_CHUNKS; i++) {
    if (lane * 8 + i * 512 < D) {
#pragma unroll
      for (int j = 0; j < 8; j++) {
        const float d = v[i][j] - mean;
        q += d * d;
      }
    }
  }
  return rsqrtf(wave_sum(q) * invD + eps);
}

// ---------------------------------------------------------------------------------------------
// layernorm_fwd: y = (x-mean)*rstd*gamma + beta  (bf16 in, bf16 out, fp32 math, biased variance)
// ---------------------------------------------------------------------------------------------
// gamma / beta are staged once per workgroup in LDS (fp32, in the order the lanes consume them: every lane's two
// float4 halves of a chunk sit 1 KB apart, so a wave's ds_read_b128 covers 1 KB contiguously): re-reading them from
// global memory for every row put 4x more bytes through the vector cache than the rows themselves (8 KB of affine
// parameters against 2 KB of x per row at D = 1024).
__global__ __launch_bounds__(256) void layernorm_fwd_kernel(const bf16_t* __restrict__ x,
                                                            const float* __restrict__ gamma,
                                                            const float* __restrict__ beta, bf16_t* __restrict__ y,
                                                            float* __restrict__ mean_out, float* __restrict__ rstd_out,
                                                            int64_t rows, int D, float eps) {
  __shared__ __attribute__((aligned(16))) float4 gbs[LN_MAX_CHUNKS][4][64];   // [chunk][gamma lo, gamma hi, beta lo, beta hi][lane]
  const int lane = threadIdx.x & 63;
  for (int q = threadIdx.x; q < LN_MAX_CHUNKS * 64; q += 256) {
    const int i = q >> 6, l = q & 63, c = l * 8 + i * 512;
    if (c < D) {
      gbs[i][0][l] = *(const float4*)(gamma + c);
      gbs[i][1][l] = *(const float4*)(gamma + c + 4);
      gbs[i][2][l] = *(const float4*)(beta + c);
      gbs[i][3][l] = *(const float4*)(beta + c + 4);
    }
  }
  __syncthreads();
  const int64_t wave = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int64_t nw = (int64_t)gridDim.x * 4;
  const float invD = 1.0f / (float)D;
  for (int64_t r = wave; r < rows; r += nw) {
    const bf16_t* xp = x + r * D;
    float v[LN_MAX_CHUNKS][8];
    const float mean = ln_row_mean<true>(xp, v, lane, D, invD);
    const float rstd = ln_row_rstd(v, mean, lane, D, invD, eps);
    bf16_t* yp = y + r * D;
#pragma unroll
    for (int i = 0; i < LN_MAX_CHUNKS; i++) {
      const int c = lane * 8 + i * 512;
      if (c < D) {
        const float4 g0 = gbs[i][0][lane], g1 = gbs[i][1][lane], b0 = gbs[i][2][lane], b1 = gbs[i][3][lane];
        const float gm[8] = {g0.x, g0.y, g0.z, g0.w, g1.x, g1.y, g1.z, g1.w};
        const float bt[8] = {b0.x, b0.y, b0.z, b0.w, b1.x, b1.y, b1.z, b1.w};
        float o[8];
#pragma unroll
        for (int j = 0; j < 8; j++) o[j] = (v[i][j] - mean) * rstd * gm[j] + bt[j];
        store8(yp + c, o);
      }
    }
    if (lane == 0 && mean_out) {
      mean_out[r] = mean;
      rstd_out[r] = rstd;
    }
  }
}

extern "C" int vj_layernorm_fwd(const void* x_bf16, const float* gamma, const float* beta, void* y_bf16, float* mean,
                                float* rstd, int64_t rows, int64_t D, float eps, hipStream_t stream) {
  if (ln_check_D("vj_layernorm_fwd", D, true)) return -1;
  VJ_CHECK_ARG((mean == nullptr) == (rstd == nullptr), "vj_layernorm_fwd: mean and rstd must both be given or both null");
  if (rows == 0) return 0;
  hipLaunchKernelGGL(layernorm_fwd_kernel, dim3(ln_grid(rows)), dim3(256), 0, stream, (const bf16_t*)x_bf16, gamma,
                     beta, (bf16_t*)y_bf16, mean, rstd, rows, (int)D, eps);
  VJ_LAUNCH_CHECK("vj_layernorm_fwd");
  return 0;
}

// ---------------------------------------------------------------------------------------------
// LayerNorm folded into the consuming Linear (round 5; vj_gemm_bf16_nt_lnfold, gemm.hip): what is left of the LayerNorm pass.
//   rowstats: rs[m] = {rstd_m, -mean_m * rstd_m} of the bf16 rows x -- the statistics of layernorm_fwd_kernel bit for bit (both run
//             ln_row_mean / ln_row_rstd; tests/test_norm_loss_optim_gpu.py compares them), but x is only READ: half the bytes
//             of the LayerNorm pass, and the GEMM that consumed its output now reads x directly.
//   fold_weights: Wf[n,:] = bf16(W[n,:] * gamma), c[n] = sum_k Wf[n,k] (of the ROUNDED values: the epilogue's acc - mean * c then
//             cancels exactly what the matrix pipe accumulated), bf[n] = b[n] + sum_k W[n,k] beta[k].  One wave per output row;
//             run once per optimizer step on the EMA target's fp32 weights.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void ln_rowstats_kernel(const bf16_t* __restrict__ x, float* __restrict__ rs, int64_t rows, int D,
                                                          float eps) {
  const int lane = threadIdx.x & 63;
  const int64_t wave = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int64_t nw = (int64_t)gridDim.x * 4;
  const float invD = 1.0f / (float)D;
  for (int64_t r = wave; r < rows; r += nw) {
    const bf16_t* xp = x + r * D;
    float v[LN_MAX_CHUNKS][8];
    const float mean = ln_row_mean<true>(xp, v, lane, D, invD);
    const float rstd = ln_row_rstd(v, mean, lane, D, invD, eps);
    if (lane == 0) *(float2*)(rs + 2 * r) = make_float2(rstd, -mean * rstd);
  }
}

extern "C" int vj_ln_rowstats(const void* x_bf16, float* rowstats, int64_t rows, int64_t D, float eps, hipStream_t stream) {
  if (ln_check_D("vj_ln_rowstats", D, true)) return -1;
  VJ_CHECK_ARG(rowstats != nullptr && ((uintptr_t)rowstats % 8 == 0), "vj_ln_rowstats: rowstats null or misaligned");
  if (rows == 0) return 0;
  hipLaunchKernelGGL(ln_rowstats_kernel, dim3(ln_grid(rows)), dim3(256), 0, stream, (const bf16_t*)x_bf16, rowstats, rows, (int)D, eps);
  VJ_LAUNCH_CHECK("vj_ln_rowstats");
  return 0;
}

__global__ __launch_bounds__(256) void ln_fold_weights_kernel(const float* __restrict__ W, const float* __restrict__ b,
                                                              const float* __restrict__ gamma, const float* __restrict__ beta,
                                                              bf16_t* __restrict__ Wf, float* __restrict__ cvec, float* __restrict__ bf,
                                                              int64_t N, int K) {
  const int lane = threadIdx.x & 63;
  const int64_t n = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (n >= N) return;
  const float* wp = W + n * K;
  bf16_t* op = Wf + n * K;
  float sc = 0.f, sb = 0.f;
  for (int k = lane * 4; k < K; k += 256) {   // K % 4 == 0
    const float4 w = *(const float4*)(wp + k);
    const float4 g = *(const float4*)(gamma + k);
    const float4 be = *(const float4*)(beta + k);
    u32x2_t o;
    o[0] = pack_bf2(w.x * g.x, w.y * g.y);
    o[1] = pack_bf2(w.z * g.z, w.w * g.w);
    *(u32x2_t*)(op + k) = o;
    sc += (bf_lo(o[0]) + bf_hi(o[0])) + (bf_lo(o[1]) + bf_hi(o[1]));
    sb += (w.x * be.x + w.y * be.y) + (w.z * be.z + w.w * be.w);
  }
  sc = wave_sum(sc);
  sb = wave_sum(sb);
  if (lane == 0) {
    cvec[n] = sc;
    bf[n] = (b ? b[n] : 0.f) + sb;
  }
}

// W [N,K] fp32 (row-major, contiguous), b [N] fp32 or null, gamma / beta [K] fp32 -> Wf [N,K] bf16, cvec [N], bf [N]
extern "C" int vj_ln_fold_weights(const float* W, const float* b, const float* gamma, const float* beta, void* Wf_bf16, float* cvec,
                                  float* bf, int64_t N, int64_t K, hipStream_t stream) {
  VJ_CHECK_ARG(W != nullptr && gamma != nullptr && beta != nullptr && Wf_bf16 != nullptr && cvec != nullptr && bf != nullptr,
               "vj_ln_fold_weights: null pointer");
  VJ_CHECK_ARG(K % 4 == 0 && K > 0 && N >= 0 && K < (1 << 30), "vj_ln_fold_weights: K=%ld must be a positive multiple of 4", (long)K);
  VJ_CHECK_ARG((((uintptr_t)W | (uintptr_t)gamma | (uintptr_t)beta) % 16 == 0) && ((uintptr_t)Wf_bf16 % 8 == 0),
               "vj_ln_fold_weights: W / gamma / beta must be 16-byte aligned, Wf 8-byte aligned");
  if (N == 0) return 0;
  hipLaunchKernelGGL(ln_fold_weights_kernel, dim3((unsigned)cdiv64(N, 4)), dim3(256), 0, stream, W, b, gamma, beta, (bf16_t*)Wf_bf16,
                     cvec, bf, N, (int)K);
  VJ_LAUNCH_CHECK("vj_ln_fold_weights");
  return 0;
}

// ---------------------------------------------------------------------------------------------
// layernorm_bwd: dx = rstd*(g - mean(g) - xhat*mean(g*xhat)) [+ dres], g = dy*gamma
// per-block partial dgamma/dbeta in fp32 -> part[blk][0:D]=dgamma, part[blk][D:2D]=dbeta
// CS: also the column sums of the OUTPUT dx (fp32, before the bf16 rounding) -> part[blk][2D:3D].  In a transformer block
// dx of norm2's backward is the dY of the proj Linear and dx of norm1's backward is the dY of the previous block's fc2, so
// their bias gradients (colsum of dY) come out of this pass for 16 more accumulator registers instead of costing a
// separate read of dY each (the transpose-free weight-gradient route has no transpose pass to fold them into).
// ---------------------------------------------------------------------------------------------
#define LN_BWD_MAX_BLOCKS 1024
template <int NCH, bool CS>
__global__ __launch_bounds__(256) void layernorm_bwd_kernel(const bf16_t* __restrict__ dy, const bf16_t* __restrict__ x,
                                                            const float* __restrict__ gamma,
                                                            const float* __restrict__ mean_in,
                                                            const float* __restrict__ rstd_in,
                                                            const bf16_t* __restrict__ dres, bf16_t* __restrict__ dx,
                                                            float* __restrict__ part, int64_t rows, int D) {
  constexpr int NSEG = CS ? 3 : 2;
  __shared__ float red[4][512 * NSEG];  // 4 waves x (512 dgamma | 512 dbeta [| 512 colsum dx]) staged per chunk pass
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const float invD = 1.0f / (float)D;
  float ag[NCH][8], ab[NCH][8], gam[NCH][8], as[CS ? NCH : 1][8];
#pragma unroll
  for (int i = 0; i < NCH; i++) {
    const int c = lane * 8 + i * 512;
#pragma unroll
    for (int j = 0; j < 8; j++) {
      ag[i][j] = ab[i][j] = 0.f;
      if constexpr (CS) as[i][j] = 0.f;
      gam[i][j] = (c < D) ? gamma[c + j] : 0.f;
    }
  }
  const int64_t rows_per = cdiv64(rows, gridDim.x);
  const int64_t rbeg = (int64_t)blockIdx.x * rows_per;
  const int64_t rend = (rbeg + rows_per < rows) ? rbeg + rows_per : rows;
  // Software prefetch, one row ahead (round 4): a wave used to load x | dy of its row, wait, reduce, THEN load the residual gradient, and
  // read the row's mean / rstd with a dependent scalar-sized load at the top of every iteration -- three exposed memory latencies per
  // row with ~10 waves per CU on the context-encoder launches (660 workgroups): 3.2 TB/s.  Now the raw 16-byte chunks of x, dy, dres
  // and the two statistics of row r + 4 are requested before row r is computed.  Same arithmetic in the same order: bit-identical.
  u32x4_t nx[NCH], nd[NCH], nr[NCH];
  float nmean = 0.f, nrstd = 0.f;
  auto request = [&](int64_t r) __attribute__((always_inline)) {
#pragma unroll
    for (int i = 0; i < NCH; i++) {
      const int c = lane * 8 + i * 512;
      if (c < D) {
        nx[i] = *(const u32x4_t*)(x + r * D + c);
        nd[i] = *(const u32x4_t*)(dy + r * D + c);
        if (dres) nr[i] = *(const u32x4_t*)(dres + r * D + c);
      }
    }
    nmean = mean_in[r];
    nrstd = rstd_in[r];
  };
#pragma unroll
  for (int i = 0; i < NCH; i++) nx[i] = nd[i] = nr[i] = (u32x4_t){0u, 0u, 0u, 0u};
  if (rbeg + wv < rend) request(rbeg + wv);
  for (int64_t r = rbeg + wv; r < rend; r += 4) {
    u32x4_t cx[NCH], cd[NCH], cr[NCH];
#pragma unroll
    for (int i = 0; i < NCH; i++) {
      cx[i] = nx[i];
      cd[i] = nd[i];
      cr[i] = nr[i];
    }
    const float mean = nmean, rstd = nrstd;
    if (r + 4 < rend) request(r + 4);
    // (the second pass recomputes xhat and g from the raw chunks -- the same operations on the same operands, hence the same bits --
    //  instead of keeping 16 floats per chunk alive across the two wave reductions: with the prefetch buffers that keeps the
    //  D = 1024 variant at three waves per SIMD, i.e. its 660 workgroups resident in one round)
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int i = 0; i < NCH; i++) {
      const int c = lane * 8 + i * 512;
      if (c < D) {
        float xv[8], dv[8];
        unpack8(cx[i], xv);
        unpack8(cd[i], dv);
#pragma unroll
        for (int j = 0; j < 8; j++) {
          const float xh = __fmul_rn(__fsub_rn(xv[j], mean), rstd);   // (rounded products: never contracted into the FMAs below,
          const float g = __fmul_rn(dv[j], gam[i][j]);                //  so both passes see the same xhat and g)
          s1 += g;
          s2 += g * xh;
          ag[i][j] += dv[j] * xh;
          ab[i][j] += dv[j];
        }
      }
    }
    const float c1 = wave_sum(s1) * invD, c2 = wave_sum(s2) * invD;
#pragma unroll
    for (int i = 0; i < NCH; i++) {
      const int c = lane * 8 + i * 512;
      if (c < D) {
        float o[8], xv[8], dv[8];
        unpack8(cx[i], xv);
        unpack8(cd[i], dv);
        if (dres) {
          unpack8(cr[i], o);
        } else {
#pragma unroll
          for (int j = 0; j < 8; j++) o[j] = 0.f;
        }
#pragma unroll
        for (int j = 0; j < 8; j++) {
          const float xh = __fmul_rn(__fsub_rn(xv[j], mean), rstd);   // (rounded products: never contracted into the FMAs below,
          const float g = __fmul_rn(dv[j], gam[i][j]);                //  so both passes see the same xhat and g)
          o[j] += rstd * (g - c1 - xh * c2);
        }
        if constexpr (CS) {
#pragma unroll
          for (int j = 0; j < 8; j++) as[i][j] += o[j];
        }
        store8(dx + r * D + c, o);
      }
    }
  }
  // cross-wave reduction of the column partials, one chunk pass at a time (512 columns x {dgamma,dbeta})
  float* pg = part + (int64_t)blockIdx.x * NSEG * D;
#pragma unroll
  for (int i = 0; i < NCH; i++) {
    if (i * 512 < D) {
      __syncthreads();
#pragma unroll
      for (int j = 0; j < 8; j++) {
        red[wv][lane * 8 + j] = ag[i][j];
        red[wv][512 + lane * 8 + j] = ab[i][j];
        if constexpr (CS) red[wv][1024 + lane * 8 + j] = as[i][j];
      }
      __syncthreads();
      for (int q = threadIdx.x; q < 512 * NSEG; q += 256) {
        const int col = (q & 511) + i * 512;
        if (col < D) {
          const float s = red[0][q] + red[1][q] + red[2][q] + red[3][q];
          pg[(q >> 9) * D + col] = s;
        }
      }
    }
  }
}

extern "C" int64_t vj_layernorm_bwd_ws_bytes(int64_t D) { return (int64_t)LN_BWD_MAX_BLOCKS * 3 * D * 4; }

// The backward kernel alone: dx is complete, the column partials part[nb][nseg * D] (nseg = 3 with `cs`: dgamma | dbeta |
// column sums of dx; else 2) are left in `ws` for the caller to reduce (the block chain reduces everything a block produced
// in ONE launch, chain.hip).  *nb_out = number of partial rows.
int vj_layernorm_bwd_partials(const void* dy_bf16, const void* x_bf16, const float* gamma, const float* mean, const float* rstd,
                              const void* dres_bf16, void* dx_bf16, bool cs, int64_t rows, int64_t D, void* ws,
                              int64_t ws_bytes, int64_t* nb_out, hipStream_t stream) {
  if (ln_check_D("vj_layernorm_bwd", D)) return -1;
  VJ_CHECK_ARG(ws_bytes >= vj_layernorm_bwd_ws_bytes(D), "vj_layernorm_bwd: workspace too small");
  *nb_out = 0;
  if (rows == 0) return 0;
  int64_t nb = cdiv64(rows, 16);  // >= 16 rows per workgroup so the column partials amortise
  if (nb > LN_BWD_MAX_BLOCKS) nb = LN_BWD_MAX_BLOCKS;
  if (nb < 1) nb = 1;
#define VJ_LNB(NCHV, CSV)                                                                                               \
  hipLaunchKernelGGL((layernorm_bwd_kernel<NCHV, CSV>), dim3((unsigned)nb), dim3(256), 0, stream, (const bf16_t*)dy_bf16, \
                     (const bf16_t*)x_bf16, gamma, mean, rstd, (const bf16_t*)dres_bf16, (bf16_t*)dx_bf16, (float*)ws,   \
                     rows, (int)D)
  if (cs) {
    if (D <= 512) VJ_LNB(1, true);
    else if (D <= 1024) VJ_LNB(2, true);
    else if (D <= 1536) VJ_LNB(3, true);
    else VJ_LNB(4, true);
  } else {
    if (D <= 512) VJ_LNB(1, false);
    else if (D <= 1024) VJ_LNB(2, false);
    else if (D <= 1536) VJ_LNB(3, false);
    else VJ_LNB(4, false);
  }
#undef VJ_LNB
  VJ_LAUNCH_CHECK("vj_layernorm_bwd");
  *nb_out = nb;
  return 0;
}

// dgamma/dbeta (and dxsum, nullable: column sums of dx) : out = alpha * sum + beta_acc * out   (beta_acc = 1 accumulates)
extern "C" int vj_layernorm_bwd_colsum(const void* dy_bf16, const void* x_bf16, const float* gamma, const float* mean,
                                       const float* rstd, const void* dres_bf16, void* dx_bf16, float* dgamma,
                                       float* dbeta, float* dxsum, float alpha, float beta_acc, int64_t rows, int64_t D,
                                       void* ws, int64_t ws_bytes, hipStream_t stream) {
  int64_t nb = 0;
  if (int rc = vj_layernorm_bwd_partials(dy_bf16, x_bf16, gamma, mean, rstd, dres_bf16, dx_bf16, dxsum != nullptr, rows, D, ws,
                                         ws_bytes, &nb, stream))
    return rc;
  if (nb == 0) return 0;
  float* outs[3] = {dgamma, dbeta, dxsum};
  return vj_reduce_partials_multi((const float*)ws, outs, dxsum != nullptr ? 3 : 2, nb, D, alpha, beta_acc, stream);   // ONE launch
}

extern "C" int vj_layernorm_bwd(const void* dy_bf16, const void* x_bf16, const float* gamma, const float* mean,
                                const float* rstd, const void* dres_bf16, void* dx_bf16, float* dgamma, float* dbeta,
                                float alpha, float beta_acc, int64_t rows, int64_t D, void* ws, int64_t ws_bytes,
                                hipStream_t stream) {
  return vj_layernorm_bwd_colsum(dy_bf16, x_bf16, gamma, mean, rstd, dres_bf16, dx_bf16, dgamma, dbeta, nullptr, alpha,
                                 beta_acc, rows, D, ws, ws_bytes, stream);
}

// ---------------------------------------------------------------------------------------------
// target_rows: h[b,k,:] = LN_noaffine_{eps2}( LN_{gamma,beta,eps1}( x[b, idx[b,k], :] ) )   fp32 out
// (final encoder norm + F.layer_norm + apply_masks fused; only the K predicted rows are ever normalised)
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void target_rows_kernel(const bf16_t* __restrict__ x, const float* __restrict__ gamma,
                                                          const float* __restrict__ beta,
                                                          const int64_t* __restrict__ idx, float* __restrict__ h,
                                                          int64_t B, int64_t N, int64_t K, int D, float eps1,
                                                          float eps2) {
  const int lane = threadIdx.x & 63;
  const int64_t wave = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int64_t nw = (int64_t)gridDim.x * 4;
  const float invD = 1.0f / (float)D;
  for (int64_t r = wave; r < B * K; r += nw) {
    const int64_t b = r / K;
    const bf16_t* xp = x + (b * N + idx[r]) * D;
    float v[LN_MAX_CHUNKS][8];
    float mean = ln_row_mean<true>(xp, v, lane, D, invD);
    float rstd = ln_row_rstd(v, mean, lane, D, invD, eps1);
#pragma unroll
    for (int i = 0; i < LN_MAX_CHUNKS; i++) {
      const int c = lane * 8 + i * 512;
      if (c < D) {
#pragma unroll
        for (int j = 0; j < 8; j++) v[i][j] = (v[i][j] - mean) * rstd * gamma[c + j] + beta[c + j];
      }
    }
    mean = ln_row_mean<false>(nullptr, v, lane, D, invD);
    rstd = ln_row_rstd(v, mean, lane, D, invD, eps2);
    float* hp = h + r * D;
#pragma unroll
    for (int i = 0; i < LN_MAX_CHUNKS; i++) {
      const int c = lane * 8 + i * 512;
      if (c < D) {
        float4 o0, o1;
        o0.x = (v[i][0] - mean) * rstd;
        o0.y = (v[i][1] - mean) * rstd;
        o0.z = (v[i][2] - mean) * rstd;
        o0.w = (v[i][3] - mean) * rstd;
        o1.x = (v[i][4] - mean) * rstd;
        o1.y = (v[i][5] - mean) * rstd;
        o1.z = (v[i][6] - mean) * rstd;
        o1.w = (v[i][7] - mean) * rstd;
        *(float4*)(hp + c) = o0;
        *(float4*)(hp + c + 4) = o1;
      }
    }
  }
}

extern "C" int vj_target_rows(const void* x_bf16, const float* gamma, const float* beta, const int64_t* idx,
                              float* h, int64_t B, int64_t N, int64_t K, int64_t D, float eps_norm, float eps_ln,
                              hipStream_t stream) {
  if (ln_check_D("vj_target_rows", D)) return -1;
  if (B * K == 0) return 0;
  hipLaunchKernelGGL(target_rows_kernel, dim3(ln_grid(B * K)), dim3(256), 0, stream, (const bf16_t*)x_bf16, gamma,
                     beta, idx, h, B, N, K, (int)D, eps_norm, eps_ln);
  VJ_LAUNCH_CHECK("vj_target_rows");
  return 0;
}
