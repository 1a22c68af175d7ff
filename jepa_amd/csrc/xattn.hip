// Cross-attention of a FEW learned query tokens against the token sequence of a frozen encoder, forward and backward,
// for gfx950: the attention inside the attentive probe that the reference trains on frozen V-JEPA features.
//   reference: CrossAttention.forward (src/models/utils/modules.py:140-157: q = Linear(query), kv = Linear(x) packed
//   [B,N,2,H,hd], F.scaled_dot_product_attention(q, k, v), default scale hd^-0.5; NOTE its `proj` is never applied) as used by
//   CrossAttentionBlock (modules.py:177-181: q + xattn(q, norm1(x))) inside AttentivePooler (attentive_pooler.py:96-102,
//   num_queries = 1 in AttentiveClassifier, attentive_pooler.py:120-130).
//
// One query row against N keys is a matrix-VECTOR product: 2 N hd flop for 4 N hd bytes of K and V -- HBM-bound by two
// orders of magnitude, so there is no MFMA here.  One workgroup per (batch, head[, query]) streams K then V once each
// (16-byte row chunks, eight consecutive lanes cover one 128-byte row of hd = 64), keeps the N scores / probabilities in LDS
// (fp32) and reduces in a fixed order (deterministic).  Algorithmic bytes: forward 4 N hd per (b, h, query); backward
// reads K and V twice and writes dK and dV once: 12 N hd.
// Those single-workgroup kernels hold N fp32 scores (forward) or two such arrays (backward) in LDS, so they serve N <= 38 264
// (forward) and N <= 19 132 (backward).  Above that the _ws entry points run split-key kernels instead: fixed chunks of XA_CHUNK
// keys, one workgroup per (b, h[, query], chunk), fp32 partials in a caller-provided workspace merged in ascending chunk order.
// Algorithmic bytes of the split forms: forward 4 N hd per (b, h, query) (+ hd + 2 fp32 per chunk); backward 10 N hd + 16 N per
// (b, h) -- pass 1 reads K and V and writes p_j and dP_j (fp32), pass 2 reads p_j, dP_j and K and writes dK and dV.
//   forward : s_j = (q . k_j) scale log2e ; p_j = 2^(s_j - max) ; y = sum_j p_j v_j / sum_j p_j ; out = residual + y ;
//             lse2 = max + log2(sum)
//   backward: p_j = 2^(s_j - lse2) ; dP_j = dy . v_j ; delta = sum_j p_j dP_j ; dS_j = p_j (dP_j - delta) ;
//             dq = scale sum_j dS_j k_j ; dk_j = scale dS_j q ; dv_j = p_j dy            (one query per (b, h))
#include "common.hpp"

#define XA_THREADS 256
#define XA_LOG2E 1.4426950408889634f

namespace {

// dynamic LDS layout of the single-workgroup kernels: [qv: 128][red: 8][part: (256 / nch) * hd <= 256 * 8 = 2048][sc: N][ds: N (backward only)]
// (the split-key kernels keep the same arrays, XA_CHUNK scores long, in static LDS)
#define XA_LDS_FIXED (128 + 8 + 2048)
// ... and they keep every score of a (b, h, query) there: 1 (forward) or 2 (backward) fp32 arrays of N
#define XA_LDS_MAX (160 * 1024 - 2048)

// what a workgroup works on: blockIdx.x = (b, h, query) -- (b, h) where NQ = 1 -- and the keys from j0 on
struct XaSlice {
  int b, h, iq;
  int64_t D, rs, koff, col;           // rs: stride of the packed [K | V] rows; koff: key j0 of this (b, h) in kv and dkv; col: this
                                      // head in a [B, D] tensor (dy, dq)
  const bf16_t *kbase, *vbase, *qp;
};
__device__ __forceinline__ XaSlice xa_slice(const bf16_t* q, int64_t q_bstride, const bf16_t* kv, int NQ, int N, int H, int hd,
                                            int j0 = 0) {
  XaSlice s;
  s.iq = blockIdx.x % NQ;
  const int bh = blockIdx.x / NQ;
  s.h = bh % H;
  s.b = bh / H;
  s.D = (int64_t)H * hd;
  s.rs = 2 * s.D;
  s.koff = ((int64_t)s.b * N + j0) * s.rs + (int64_t)s.h * hd;
  s.col = (int64_t)s.b * s.D + (int64_t)s.h * hd;
  s.kbase = kv + s.koff;
  s.vbase = s.kbase + s.D;
  s.qp = q + (int64_t)s.b * q_bstride + (int64_t)s.iq * s.D + (int64_t)s.h * hd;
  return s;
}

// this head's hd elements of a bf16 row into LDS as fp32, times `mul`.  No barrier here.
__device__ __forceinline__ void xa_stage(const bf16_t* p, int hd, float* dst, float mul = 1.f) {
  if ((int)threadIdx.x < hd) dst[threadIdx.x] = bf2f(p[threadIdx.x]) * mul;
}

__device__ __forceinline__ float xa_block_reduce(float v, float* red, bool is_max) {
  // wave reduction, then the four waves through LDS in a fixed order
  v = is_max ? wave_max(v) : wave_sum(v);
  const int w = threadIdx.x >> 6;
  __syncthreads();   // `red` may still be read from a previous call
  if ((threadIdx.x & 63) == 0) red[w] = v;
  __syncthreads();
  float r = red[0];
#pragma unroll
  for (int i = 1; i < XA_THREADS / 64; i++) r = is_max ? fmaxf(r, red[i]) : r + red[i];
  return r;
}

// a + the dot product of one 16-byte chunk of a bf16 row with the eight fp32 at v, in element order
__device__ __forceinline__ float xa_dot8(float a, const u32x4_t& w, const float* v) {
#pragma unroll
  for (int i = 0; i < 4; i++) a += bf_lo(w[i]) * v[2 * i] + bf_hi(w[i]) * v[2 * i + 1];
  return a;
}

// s_j for every key of this (b, h) into LDS; qv = this head's query row (fp32, LDS), pre-multiplied by scale * log2e
__device__ __forceinline__ void xa_scores(const bf16_t* __restrict__ kbase, int64_t rs, int N, int hd, const float* qv,
                                          float* sc) {
  const int nch = hd >> 3;
  for (int j = threadIdx.x; j < N; j += XA_THREADS) {
    const bf16_t* kp = kbase + (int64_t)j * rs;
    float a = 0.f;
    for (int c = 0; c < nch; c++) a = xa_dot8(a, *(const u32x4_t*)(kp + c * 8), qv + c * 8);
    sc[j] = a;
  }
}

// out[d] = sum_j wgt[j] * rows[j][d] for this head: thread = (row group rg, 8-column chunk c); partial sums through LDS
// (part[rg][hd], fixed summation order).  Returns the total for column d = threadIdx.x (valid for threadIdx.x < hd).
__device__ __forceinline__ float xa_weighted_rows(const bf16_t* __restrict__ base, int64_t rs, int N, int hd,
                                                  const float* wgt, float* part) {
  const int nch = hd >> 3, ngrp = XA_THREADS / nch;   // nch in {1..16}: 256 / nch row groups (hd = 80: 25 groups, 6 idle threads)
  const int c = threadIdx.x % nch, rg = threadIdx.x / nch;
  float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if (rg < ngrp) {
    for (int j = rg; j < N; j += ngrp) {
      const u32x4_t w = *(const u32x4_t*)(base + (int64_t)j * rs + c * 8);
      const float p = wgt[j];
#pragma unroll
      for (int i = 0; i < 4; i++) {
        acc[2 * i] += p * bf_lo(w[i]);
        acc[2 * i + 1] += p * bf_hi(w[i]);
      }
    }
  }
  __syncthreads();   // `part` may still be read from a previous call
  if (rg < ngrp) {
#pragma unroll
    for (int i = 0; i < 8; i++) part[rg * hd + c * 8 + i] = acc[i];
  }
  __syncthreads();
  float tot = 0.f;
  if ((int)threadIdx.x < hd)
    for (int g = 0; g < ngrp; g++) tot += part[g * hd + threadIdx.x];
  return tot;
}
// the soft-max of the n keys from kbase on: s_j into sc, the block max, p_j = 2^(s_j - max) left in sc, their block sum, and this
// thread's column of sum_j p_j v_j (valid for threadIdx.x < hd)
struct XaSoft {
  float mx, sum, y;
};
__device__ __forceinline__ XaSoft xa_softmax_rows(const XaSlice& s, int n, int hd, const float* qv, float* red, float* part,
                                                  float* sc) {
  XaSoft r;
  xa_scores(s.kbase, s.rs, n, hd, qv, sc);
  r.mx = -INFINITY;
  for (int j = threadIdx.x; j < n; j += XA_THREADS) r.mx = fmaxf(r.mx, sc[j]);   // own entries: no barrier needed yet
  r.mx = xa_block_reduce(r.mx, red, true);
  r.sum = 0.f;
  for (int j = threadIdx.x; j < n; j += XA_THREADS) {
    const float p = __builtin_amdgcn_exp2f(sc[j] - r.mx);
    sc[j] = p;
    r.sum += p;
  }
  r.sum = xa_block_reduce(r.sum, red, false);   // its barriers also publish every thread's p_j
  r.y = xa_weighted_rows(s.vbase, s.rs, n, hd, sc, part);
  return r;
}

// dk_j = scale dS_j q ; dv_j = p_j dy for the n keys from dkb on (dkb: this head's columns of the first key's dK row; dV lies D
// further): thread = (row group, 8-column chunk), 16-byte stores
__device__ __forceinline__ void xa_store_dkdv(bf16_t* __restrict__ dkb, int64_t rs, int64_t D, int n, int hd, const float* qraw,
                                              const float* dyv, float scale, const float* ds, const float* sc) {
  const int nch = hd >> 3, ngrp = XA_THREADS / nch;
  const int c = threadIdx.x % nch, rg = threadIdx.x / nch;
  if (rg < ngrp) {
    float q8[8], d8[8];
#pragma unroll
    for (int i = 0; i < 8; i++) {
      q8[i] = qraw[c * 8 + i] * scale;
      d8[i] = dyv[c * 8 + i];
    }
    dkb += c * 8;
    for (int j = rg; j < n; j += ngrp) {
      const float s = ds[j], p = sc[j];
      u32x4_t wk, wv;
#pragma unroll
      for (int i = 0; i < 4; i++) {
        wk[i] = pack_bf2(s * q8[2 * i], s * q8[2 * i + 1]);
        wv[i] = pack_bf2(p * d8[2 * i], p * d8[2 * i + 1]);
      }
      *(u32x4_t*)(dkb + (int64_t)j * rs) = wk;
      *(u32x4_t*)(dkb + (int64_t)j * rs + D) = wv;
    }
  }
}

__global__ __launch_bounds__(XA_THREADS) void xattn_fwd_kernel(const bf16_t* __restrict__ q, int64_t q_bstride,
                                                               const bf16_t* __restrict__ kv,
                                                               const bf16_t* __restrict__ resid, bf16_t* __restrict__ out,
                                                               float* __restrict__ lse2, int B, int NQ, int N, int H,
                                                               int hd, float scale) {
  extern __shared__ __attribute__((aligned(16))) float xs[];
  float* qv = xs;
  float* red = xs + 128;
  float* part = xs + 136;
  float* sc = xs + XA_LDS_FIXED;
  const XaSlice s = xa_slice(q, q_bstride, kv, NQ, N, H, hd);
  xa_stage(s.qp, hd, qv, scale * XA_LOG2E);
  __syncthreads();
  const XaSoft m = xa_softmax_rows(s, N, hd, qv, red, part, sc);
  if ((int)threadIdx.x < hd) {
    const int64_t o = ((int64_t)s.b * NQ + s.iq) * s.D + (int64_t)s.h * hd + threadIdx.x;
    float v = m.y / m.sum;
    // the block's residual (the un-projected query tokens, attentive_pooler.py:97-98 + modules.py:178-179) is
    // the same row for every sample
    if (resid) v += bf2f(resid[(int64_t)s.iq * s.D + (int64_t)s.h * hd + threadIdx.x]);
    out[o] = f2bf(v);
  }
  if (threadIdx.x == 0 && lse2) lse2[((int64_t)s.b * H + s.h) * NQ + s.iq] = m.mx + log2f(m.sum);
}

__global__ __launch_bounds__(XA_THREADS) void xattn_bwd_kernel(const bf16_t* __restrict__ q, int64_t q_bstride,
                                                               const bf16_t* __restrict__ kv,
                                                               const bf16_t* __restrict__ dy,
                                                               const float* __restrict__ lse2, bf16_t* __restrict__ dq,
                                                               bf16_t* __restrict__ dkv, int B, int N, int H, int hd,
                                                               float scale) {
  extern __shared__ __attribute__((aligned(16))) float xs[];
  float* qv = xs;            // q * scale * log2e
  float* red = xs + 128;
  float* part = xs + 136;
  float* sc = xs + XA_LDS_FIXED;   // p_j
  float* ds = sc + N;              // dP_j, then dS_j
  __shared__ float dyv[128], qraw[128];
  const XaSlice s = xa_slice(q, q_bstride, kv, 1, N, H, hd);
  xa_stage(s.qp, hd, qraw);
  xa_stage(s.qp, hd, qv, scale * XA_LOG2E);
  xa_stage(dy + s.col, hd, dyv);
  __syncthreads();
  xa_scores(s.kbase, s.rs, N, hd, qv, sc);    // s_j
  xa_scores(s.vbase, s.rs, N, hd, dyv, ds);   // dP_j = dy . v_j (same row-dot routine, dy as the vector)
  const float l2 = lse2[(int64_t)s.b * H + s.h];
  float dl = 0.f;
  for (int j = threadIdx.x; j < N; j += XA_THREADS) {
    const float p = __builtin_amdgcn_exp2f(sc[j] - l2);
    sc[j] = p;
    dl += p * ds[j];
  }
  dl = xa_block_reduce(dl, red, false);   // delta = sum_j p_j dP_j
  for (int j = threadIdx.x; j < N; j += XA_THREADS) ds[j] = sc[j] * (ds[j] - dl);
  __syncthreads();
  // dq = scale * sum_j dS_j k_j   (per sample; the caller sums it over the batch when the projected query is shared)
  const float dqv = xa_weighted_rows(s.kbase, s.rs, N, hd, ds, part);
  if ((int)threadIdx.x < hd) dq[s.col + threadIdx.x] = f2bf(dqv * scale);
  xa_store_dkdv(dkv + s.koff, s.rs, s.D, N, hd, qraw, dyv, scale, ds, sc);
}

// ---- split-key forms (vj_xattn_fwd_ws / vj_xattn_bwd_ws above the single-workgroup limits) ------------------------------
// A chunk of XA_CHUNK consecutive keys per workgroup (blockIdx.y).  The chunk is a compile-time constant, so the chunk count -- and
// with it every summation order -- depends on N alone, never on the device.  Partials go to the caller's workspace (fp32) and are
// merged in ascending chunk order; no atomics.
#define XA_CHUNK 2048

// forward partials, grid (B*H*NQ, chunks): over its keys, m_c = max s_j, l_c = sum_j 2^(s_j - m_c), y_c = sum_j 2^(s_j - m_c) v_j
__global__ __launch_bounds__(XA_THREADS) void xattn_fwd_split_kernel(const bf16_t* __restrict__ q, int64_t q_bstride,
                                                                     const bf16_t* __restrict__ kv, float* __restrict__ ws_y,
                                                                     float* __restrict__ ws_ml, int NQ, int N, int H, int hd,
                                                                     float scale, int nch) {
  __shared__ __attribute__((aligned(16))) float xs[XA_LDS_FIXED + XA_CHUNK];
  float* qv = xs;
  float* red = xs + 128;
  float* part = xs + 136;
  float* sc = xs + XA_LDS_FIXED;
  const int ch = blockIdx.y, j0 = ch * XA_CHUNK, n = min(XA_CHUNK, N - j0);
  const XaSlice s = xa_slice(q, q_bstride, kv, NQ, N, H, hd, j0);
  xa_stage(s.qp, hd, qv, scale * XA_LOG2E);
  __syncthreads();
  const XaSoft m = xa_softmax_rows(s, n, hd, qv, red, part, sc);
  const int64_t slot = (int64_t)blockIdx.x * nch + ch;
  if ((int)threadIdx.x < hd) ws_y[slot * hd + threadIdx.x] = m.y;
  if (threadIdx.x == 0) {
    ws_ml[2 * slot] = m.mx;
    ws_ml[2 * slot + 1] = m.sum;
  }
}

// forward combine, grid B*H*NQ: M = max m_c ; L = sum_c 2^(m_c - M) l_c ; out = resid + sum_c 2^(m_c - M) y_c / L ; lse2 = M + log2 L
__global__ __launch_bounds__(128) void xattn_fwd_combine_kernel(const float* __restrict__ ws_y, const float* __restrict__ ws_ml,
                                                                const bf16_t* __restrict__ resid, bf16_t* __restrict__ out,
                                                                float* __restrict__ lse2, int NQ, int H, int hd, int nch) {
  const int bhq = blockIdx.x, d = threadIdx.x;
  const int iq = bhq % NQ, bh = bhq / NQ;
  const int h = bh % H, b = bh / H;
  const float* ml = ws_ml + (int64_t)bhq * nch * 2;
  const float* yc = ws_y + (int64_t)bhq * nch * hd;
  float M = -INFINITY;
  for (int c = 0; c < nch; c++) M = fmaxf(M, ml[2 * c]);
  float L = 0.f, y = 0.f;
  for (int c = 0; c < nch; c++) {
    const float w = __builtin_amdgcn_exp2f(ml[2 * c] - M);
    L += w * ml[2 * c + 1];
    if (d < hd) y += w * yc[(int64_t)c * hd + d];
  }
  if (d < hd) {
    const int64_t D = (int64_t)H * hd;
    float v = y / L;
    if (resid) v += bf2f(resid[(int64_t)iq * D + (int64_t)h * hd + d]);
    out[((int64_t)b * NQ + iq) * D + (int64_t)h * hd + d] = f2bf(v);
  }
  if (d == 0 && lse2) lse2[(int64_t)bh * NQ + iq] = M + log2f(L);
}

// backward pass 1, grid (B*H, chunks): p_j = 2^(s_j - lse2) and dP_j = dy . v_j to the workspace, and the chunk's part of
// delta = sum_j p_j dP_j
__global__ __launch_bounds__(XA_THREADS) void xattn_bwd_split_p_kernel(const bf16_t* __restrict__ q, int64_t q_bstride,
                                                                       const bf16_t* __restrict__ kv,
                                                                       const bf16_t* __restrict__ dy,
                                                                       const float* __restrict__ lse2, float* __restrict__ ws_p,
                                                                       float* __restrict__ ws_dp, float* __restrict__ ws_delta,
                                                                       int N, int H, int hd, float scale, int nch) {
  __shared__ __attribute__((aligned(16))) float qv[128], dyv[128], red[8];
  const int bh = blockIdx.x, ch = blockIdx.y, j0 = ch * XA_CHUNK, n = min(XA_CHUNK, N - j0);
  const XaSlice s = xa_slice(q, q_bstride, kv, 1, N, H, hd, j0);
  xa_stage(s.qp, hd, qv, scale * XA_LOG2E);
  xa_stage(dy + s.col, hd, dyv);
  __syncthreads();
  const float l2 = lse2[bh];
  float* pp = ws_p + (int64_t)bh * N + j0;
  float* dpp = ws_dp + (int64_t)bh * N + j0;
  const int nc8 = hd >> 3;
  float dl = 0.f;
  for (int j = threadIdx.x; j < n; j += XA_THREADS) {
    const bf16_t* kp = s.kbase + (int64_t)j * s.rs;   // K and V of a key lie in one row: both dots in one pass over it
    float a = 0.f, e = 0.f;
    for (int c = 0; c < nc8; c++) {
      a = xa_dot8(a, *(const u32x4_t*)(kp + c * 8), qv + c * 8);
      e = xa_dot8(e, *(const u32x4_t*)(kp + s.D + c * 8), dyv + c * 8);
    }
    const float p = __builtin_amdgcn_exp2f(a - l2);
    pp[j] = p;
    dpp[j] = e;
    dl += p * e;
  }
  dl = xa_block_reduce(dl, red, false);
  if (threadIdx.x == 0) ws_delta[(int64_t)bh * nch + ch] = dl;
}

// backward pass 2, grid (B*H, chunks): delta = the chunk partials summed in ascending order (the same sum in every workgroup),
// dS_j = p_j (dP_j - delta), this chunk's dq partial sum_j dS_j k_j (unscaled) to the workspace, dk_j = scale dS_j q and
// dv_j = p_j dy stored directly (every key has one owner)
__global__ __launch_bounds__(XA_THREADS) void xattn_bwd_split_d_kernel(const bf16_t* __restrict__ q, int64_t q_bstride,
                                                                       const bf16_t* __restrict__ dy,
                                                                       const bf16_t* __restrict__ kv,
                                                                       const float* __restrict__ ws_p,
                                                                       const float* __restrict__ ws_dp,
                                                                       const float* __restrict__ ws_delta,
                                                                       float* __restrict__ ws_dq, bf16_t* __restrict__ dkv,
                                                                       int N, int H, int hd, float scale, int nch) {
  __shared__ __attribute__((aligned(16))) float part[2048], sc[XA_CHUNK], ds[XA_CHUNK], dyv[128], qraw[128];
  const int bh = blockIdx.x, ch = blockIdx.y, j0 = ch * XA_CHUNK, n = min(XA_CHUNK, N - j0);
  const XaSlice s = xa_slice(q, q_bstride, kv, 1, N, H, hd, j0);
  xa_stage(s.qp, hd, qraw);
  xa_stage(dy + s.col, hd, dyv);
  float delta = 0.f;
  for (int c = 0; c < nch; c++) delta += ws_delta[(int64_t)bh * nch + c];
  const float* pp = ws_p + (int64_t)bh * N + j0;
  const float* dpp = ws_dp + (int64_t)bh * N + j0;
  for (int j = threadIdx.x; j < n; j += XA_THREADS) {
    const float p = pp[j];
    sc[j] = p;
    ds[j] = p * (dpp[j] - delta);
  }
  __syncthreads();
  const float dqv = xa_weighted_rows(s.kbase, s.rs, n, hd, ds, part);
  if ((int)threadIdx.x < hd) ws_dq[((int64_t)bh * nch + ch) * hd + threadIdx.x] = dqv;
  xa_store_dkdv(dkv + s.koff, s.rs, s.D, n, hd, qraw, dyv, scale, ds, sc);
}

// dq = scale * sum_c dq_c (ascending chunk order), grid B*H
__global__ __launch_bounds__(128) void xattn_bwd_dq_kernel(const float* __restrict__ ws_dq, bf16_t* __restrict__ dq, int hd,
                                                           float scale, int nch) {
  const int bh = blockIdx.x, d = threadIdx.x;
  if (d >= hd) return;
  const float* pd = ws_dq + (int64_t)bh * nch * hd + d;
  float t = 0.f;
  for (int c = 0; c < nch; c++) t += pd[(int64_t)c * hd];
  dq[(int64_t)bh * hd + d] = f2bf(t * scale);   // dq [B, H*hd]: (b*H + h)*hd + d
}

inline int64_t xa_max_keys(int arrays) { return ((int64_t)XA_LDS_MAX / 4 - XA_LDS_FIXED) / arrays; }

// the single-workgroup kernels may use XA_LDS_MAX bytes of dynamic LDS: said once per device and kernel
inline void xa_allow_lds(VjPerDeviceOnce& once, const void* kernel) {
  once([kernel] { (void)hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, XA_LDS_MAX); });
}

// workspace of the split forms: every sub-array 256-byte aligned
struct XaSplit {
  int64_t nch, off[4], bytes;
};
inline int64_t xa_align(int64_t x) { return (x + 255) & ~(int64_t)255; }
XaSplit xa_split_layout(int64_t B, int64_t NQ, int64_t N, int64_t H, int64_t hd, int backward) {
  XaSplit s{};
  s.nch = (N + XA_CHUNK - 1) / XA_CHUNK;
  int64_t sz[4];
  if (!backward) {   // y partials [B*H*NQ][nch][hd], (m, l) [B*H*NQ][nch][2]
    sz[0] = B * H * NQ * s.nch * hd * 4;
    sz[1] = B * H * NQ * s.nch * 2 * 4;
    sz[2] = sz[3] = 0;
  } else {           // p [B*H][N], dP [B*H][N], delta partials [B*H][nch], dq partials [B*H][nch][hd]
    sz[0] = B * H * N * 4;
    sz[1] = B * H * N * 4;
    sz[2] = B * H * s.nch * 4;
    sz[3] = B * H * s.nch * hd * 4;
  }
  int64_t o = 0;
  for (int i = 0; i < 4; i++) {
    s.off[i] = o;
    o += xa_align(sz[i]);
  }
  s.bytes = o;
  return s;
}

// the dimension check of every entry point; vj_xattn_ws_bytes passes no name and gets the answer without a message
int xa_check_dims(const char* who, int64_t B, int64_t NQ, int64_t N, int64_t H, int64_t hd) {
  const bool dims = B >= 0 && NQ >= 1 && N >= 1 && H >= 1, head = hd % 8 == 0 && hd >= 8 && hd <= 128;
  if (!who) return dims && head ? 0 : -1;
  VJ_CHECK_ARG(dims, "%s: bad dims", who);
  VJ_CHECK_ARG(head, "%s: head_dim=%ld unsupported (need %%8==0, <=128)", who, (long)hd);
  return 0;
}

int xa_check(const char* who, int64_t B, int64_t NQ, int64_t N, int64_t H, int64_t hd, int64_t* lds_bytes, int arrays) {
  if (int rc = xa_check_dims(who, B, NQ, N, H, hd)) return rc;
  VJ_CHECK_ARG(B * H * NQ < (1ll << 31), "%s: grid too large", who);
  *lds_bytes = (XA_LDS_FIXED + arrays * N) * 4;
  VJ_CHECK_ARG(*lds_bytes <= XA_LDS_MAX, "%s: N=%ld keys do not fit the LDS score buffer (max %ld)", who, (long)N,
               (long)xa_max_keys(arrays));
  return 0;
}

int xa_check_split(const char* who, int64_t B, int64_t NQ, int64_t N, int64_t H, int64_t hd, const XaSplit& s, void* ws,
                   int64_t ws_bytes) {
  if (int rc = xa_check_dims(who, B, NQ, N, H, hd)) return rc;
  VJ_CHECK_ARG(N < (1ll << 31) && B * H * NQ * XA_THREADS <= 0xffffffffll && s.nch <= 65535, "%s: grid too large", who);
  if (B == 0) return 0;   // nothing to launch: vj_xattn_ws_bytes is 0, so no workspace is required
  VJ_CHECK_ARG(ws != nullptr && ws_bytes >= s.bytes, "%s: workspace of %ld bytes, need %ld (vj_xattn_ws_bytes)", who,
               (long)ws_bytes, (long)s.bytes);
  return 0;
}

}  // namespace

extern "C" int vj_xattn_fwd(const void* q, int64_t q_bstride, const void* kv, const void* resid, void* out, float* lse2,
                            int64_t B, int64_t NQ, int64_t N, int64_t H, int64_t hd, float scale, hipStream_t stream) {
  int64_t lds = 0;
  if (int rc = xa_check("vj_xattn_fwd", B, NQ, N, H, hd, &lds, 1)) return rc;
  if (B == 0) return 0;
  static VjPerDeviceOnce once;
  xa_allow_lds(once, (const void*)xattn_fwd_kernel);
  hipLaunchKernelGGL(xattn_fwd_kernel, dim3((unsigned)(B * H * NQ)), dim3(XA_THREADS), (size_t)lds, stream, (const bf16_t*)q,
                     q_bstride, (const bf16_t*)kv, (const bf16_t*)resid, (bf16_t*)out, lse2, (int)B, (int)NQ, (int)N, (int)H,
                     (int)hd, scale);
  VJ_LAUNCH_CHECK("vj_xattn_fwd");
  return 0;
}

extern "C" int vj_xattn_bwd(const void* q, int64_t q_bstride, const void* kv, const void* dy, const float* lse2, void* dq,
                            void* dkv, int64_t B, int64_t NQ, int64_t N, int64_t H, int64_t hd, float scale,
                            hipStream_t stream) {
  VJ_CHECK_ARG(NQ == 1, "vj_xattn_bwd: one query per sample (AttentiveClassifier, attentive_pooler.py:120); got %ld", (long)NQ);
  int64_t lds = 0;
  if (int rc = xa_check("vj_xattn_bwd", B, NQ, N, H, hd, &lds, 2)) return rc;
  if (B == 0) return 0;
  static VjPerDeviceOnce once;
  xa_allow_lds(once, (const void*)xattn_bwd_kernel);
  hipLaunchKernelGGL(xattn_bwd_kernel, dim3((unsigned)(B * H)), dim3(XA_THREADS), (size_t)lds, stream, (const bf16_t*)q, q_bstride,
                     (const bf16_t*)kv, (const bf16_t*)dy, lse2, (bf16_t*)dq, (bf16_t*)dkv, (int)B, (int)N, (int)H, (int)hd, scale);
  VJ_LAUNCH_CHECK("vj_xattn_bwd");
  return 0;
}

extern "C" int64_t vj_xattn_ws_bytes(int64_t B, int64_t NQ, int64_t N, int64_t H, int64_t hd, int backward) {
  if (xa_check_dims(nullptr, B, NQ, N, H, hd)) return -1;
  if (N <= xa_max_keys(backward ? 2 : 1)) return 0;   // the single-workgroup kernel runs: no workspace
  return xa_split_layout(B, NQ, N, H, hd, backward).bytes;
}

extern "C" int vj_xattn_fwd_ws(const void* q, int64_t q_bstride, const void* kv, const void* resid, void* out, float* lse2,
                               int64_t B, int64_t NQ, int64_t N, int64_t H, int64_t hd, float scale, void* ws, int64_t ws_bytes,
                               hipStream_t stream) {
  if (N <= xa_max_keys(1)) return vj_xattn_fwd(q, q_bstride, kv, resid, out, lse2, B, NQ, N, H, hd, scale, stream);
  const XaSplit s = xa_split_layout(B, NQ, N, H, hd, 0);
  if (int rc = xa_check_split("vj_xattn_fwd_ws", B, NQ, N, H, hd, s, ws, ws_bytes)) return rc;
  if (B == 0) return 0;
  float* ws_y = (float*)((char*)ws + s.off[0]);
  float* ws_ml = (float*)((char*)ws + s.off[1]);
  hipLaunchKernelGGL(xattn_fwd_split_kernel, dim3((unsigned)(B * H * NQ), (unsigned)s.nch), dim3(XA_THREADS), 0, stream,
                     (const bf16_t*)q, q_bstride, (const bf16_t*)kv, ws_y, ws_ml, (int)NQ, (int)N, (int)H, (int)hd, scale,
                     (int)s.nch);
  VJ_LAUNCH_CHECK("vj_xattn_fwd_ws");
  hipLaunchKernelGGL(xattn_fwd_combine_kernel, dim3((unsigned)(B * H * NQ)), dim3(128), 0, stream, (const float*)ws_y,
                     (const float*)ws_ml, (const bf16_t*)resid, (bf16_t*)out, lse2, (int)NQ, (int)H, (int)hd, (int)s.nch);
  VJ_LAUNCH_CHECK("vj_xattn_fwd_ws");
  return 0;
}

extern "C" int vj_xattn_bwd_ws(const void* q, int64_t q_bstride, const void* kv, const void* dy, const float* lse2, void* dq,
                               void* dkv, int64_t B, int64_t NQ, int64_t N, int64_t H, int64_t hd, float scale, void* ws,
                               int64_t ws_bytes, hipStream_t stream) {
  VJ_CHECK_ARG(NQ == 1, "vj_xattn_bwd_ws: one query per sample (AttentiveClassifier, attentive_pooler.py:120); got %ld", (long)NQ);
  if (N <= xa_max_keys(2)) return vj_xattn_bwd(q, q_bstride, kv, dy, lse2, dq, dkv, B, NQ, N, H, hd, scale, stream);
  const XaSplit s = xa_split_layout(B, NQ, N, H, hd, 1);
  if (int rc = xa_check_split("vj_xattn_bwd_ws", B, NQ, N, H, hd, s, ws, ws_bytes)) return rc;
  if (B == 0) return 0;
  float* ws_p = (float*)((char*)ws + s.off[0]);
  float* ws_dp = (float*)((char*)ws + s.off[1]);
  float* ws_delta = (float*)((char*)ws + s.off[2]);
  float* ws_dq = (float*)((char*)ws + s.off[3]);
  const dim3 grid((unsigned)(B * H), (unsigned)s.nch);
  hipLaunchKernelGGL(xattn_bwd_split_p_kernel, grid, dim3(XA_THREADS), 0, stream, (const bf16_t*)q, q_bstride, (const bf16_t*)kv,
                     (const bf16_t*)dy, lse2, ws_p, ws_dp, ws_delta, (int)N, (int)H, (int)hd, scale, (int)s.nch);
  VJ_LAUNCH_CHECK("vj_xattn_bwd_ws");
  hipLaunchKernelGGL(xattn_bwd_split_d_kernel, grid, dim3(XA_THREADS), 0, stream, (const bf16_t*)q, q_bstride, (const bf16_t*)dy,
                     (const bf16_t*)kv, (const float*)ws_p, (const float*)ws_dp, (const float*)ws_delta, ws_dq, (bf16_t*)dkv,
                     (int)N, (int)H, (int)hd, scale, (int)s.nch);
  VJ_LAUNCH_CHECK("vj_xattn_bwd_ws");
  hipLaunchKernelGGL(xattn_bwd_dq_kernel, dim3((unsigned)(B * H)), dim3(128), 0, stream, (const float*)ws_dq, (bf16_t*)dq, (int)hd,
                     scale, (int)s.nch);
  VJ_LAUNCH_CHECK("vj_xattn_bwd_ws");
  return 0;
}
