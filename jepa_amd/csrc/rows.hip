// Token-row movers and position adds of the V-JEPA step, one wave per row: bit-exact mask gather / scatter and row-window copy,
// positional-embedding add (plain, broadcast over the temporal slices of a still image and that broadcast's adjoint, the sum over
// the slices; per frame) and predictor token assembly.
//
// Reference behaviour restated (never copied):
//   apply_masks                      src/masks/utils.py:11-23      (gather of kept token rows)
//   x += pos_embed                   src/models/vision_transformer.py:172-174
//   predictor token assembly         src/models/predictor.py:194-221
#include "common.hpp"
#include "../../include/vjepa_hip.h"

// ---------------------------------------------------------------------------------------------
// gather_rows: dst[b,k,:] = src[b*src_bstride + idx[b,k], :]   (payload moved verbatim -> bit exact)
// scatter_rows: dst[b, idx[b,k], :] = src[b,k,:]  (dst pre-zeroed; indices unique per b as produced by
// the collator, multiblock3d.py:185-186) -- backward of gather_rows.
// One body: row r = (b,k) on the plain side, row b * bstride + idx[r] on the indexed side (GATHER: the source).
// one wave per row, 16 B per lane per trip (row_bytes % 16 == 0) or 4 B per lane (row_bytes % 4 == 0)
// ---------------------------------------------------------------------------------------------
template <typename VEC, bool GATHER>
__device__ __forceinline__ void move_rows(const char* __restrict__ src, char* __restrict__ dst, const int64_t* __restrict__ idx,
                                          int64_t rows, int64_t K, int64_t row_bytes, int64_t bstride) {
  const int lane = wave_lane();
  const int64_t wave = wave_row(), nw = wave_row_step();
  const int64_t nvec = row_bytes / (int64_t)sizeof(VEC);
  for (int64_t r = wave; r < rows; r += nw) {
    const int64_t b = r / K;
    const int64_t i = b * bstride + idx[r];
    const VEC* sp = (const VEC*)(src + (GATHER ? i : r) * row_bytes);
    VEC* dp = (VEC*)(dst + (GATHER ? r : i) * row_bytes);
    for (int64_t v = lane; v < nvec; v += 64) dp[v] = sp[v];
  }
}

template <typename VEC>
__global__ __launch_bounds__(256) void gather_rows_kernel(const char* __restrict__ src, char* __restrict__ dst,
                                                          const int64_t* __restrict__ idx, int64_t rows, int64_t K,
                                                          int64_t row_bytes, int64_t src_bstride_rows) {
  move_rows<VEC, true>(src, dst, idx, rows, K, row_bytes, src_bstride_rows);
}

template <typename VEC>
__global__ __launch_bounds__(256) void scatter_rows_kernel(const char* __restrict__ src, char* __restrict__ dst,
                                                           const int64_t* __restrict__ idx, int64_t rows, int64_t K,
                                                           int64_t row_bytes, int64_t N) {
  move_rows<VEC, false>(src, dst, idx, rows, K, row_bytes, N);
}

// the 16-byte form when the rows and both bases allow it, else the 4-byte form
typedef void (*MoveRowsKernel)(const char*, char*, const int64_t*, int64_t, int64_t, int64_t, int64_t);
static inline void launch_move_rows(MoveRowsKernel k16, MoveRowsKernel k4, const void* src, void* dst, const int64_t* idx,
                                    int64_t rows, int64_t K, int64_t row_bytes, int64_t bstride, hipStream_t stream) {
  const bool v16 = (row_bytes % 16 == 0) && (((uintptr_t)src | (uintptr_t)dst) % 16 == 0);
  hipLaunchKernelGGL(v16 ? k16 : k4, dim3(rows_grid(rows)), dim3(256), 0, stream, (const char*)src, (char*)dst, idx, rows, K,
                     row_bytes, bstride);
}

extern "C" int vj_gather_rows(const void* src, void* dst, const int64_t* idx, int64_t B, int64_t K, int64_t row_bytes,
                              int64_t src_batch_stride_rows, hipStream_t stream) {
  VJ_CHECK_ARG(B >= 0 && K >= 0 && row_bytes > 0, "vj_gather_rows: bad dims B=%ld K=%ld row_bytes=%ld", (long)B,
               (long)K, (long)row_bytes);
  VJ_CHECK_ARG(row_bytes % 4 == 0, "vj_gather_rows: row_bytes=%ld must be a multiple of 4", (long)row_bytes);
  const int64_t rows = B * K;
  if (rows == 0) return 0;
  launch_move_rows(gather_rows_kernel<u32x4_t>, gather_rows_kernel<uint32_t>, src, dst, idx, rows, K, row_bytes,
                   src_batch_stride_rows, stream);
  VJ_LAUNCH_CHECK("vj_gather_rows");
  return 0;
}

extern "C" int vj_scatter_rows(const void* src, void* dst, const int64_t* idx, int64_t B, int64_t N, int64_t K,
                               int64_t row_bytes, hipStream_t stream) {
  VJ_CHECK_ARG(B >= 0 && K >= 0 && N >= 0 && row_bytes > 0, "vj_scatter_rows: bad dims");
  VJ_CHECK_ARG(row_bytes % 4 == 0, "vj_scatter_rows: row_bytes=%ld must be a multiple of 4", (long)row_bytes);
  if (B * N == 0) return 0;
  hipError_t e = hipMemsetAsync(dst, 0, (size_t)(B * N * row_bytes), stream);
  if (e != hipSuccess) {
    vj_set_error("vj_scatter_rows: memset failed: %s", hipGetErrorString(e));
    return (int)e;
  }
  const int64_t rows = B * K;
  if (rows == 0) return 0;
  launch_move_rows(scatter_rows_kernel<u32x4_t>, scatter_rows_kernel<uint32_t>, src, dst, idx, rows, K, row_bytes, N, stream);
  VJ_LAUNCH_CHECK("vj_scatter_rows");
  return 0;
}

// ---------------------------------------------------------------------------------------------
// copy_rows_strided: dst[b, dst_off + j, :] = src[b, src_off + j, :] for j < n  (bf16 rows; used to split the
// predictor stream into its context rows (grad of predictor_embed) and to slice target rows).  src == nullptr: the
// destination rows are ZEROED (the context rows of the predictor trunk's output gradient: no ATen fill on the step).
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void copy_rows_kernel(const bf16_t* __restrict__ src, bf16_t* __restrict__ dst,
                                                        int64_t B, int64_t src_rows, int64_t src_off,
                                                        int64_t dst_rows, int64_t dst_off, int64_t n, int D) {
  const int lane = wave_lane();
  const int64_t wave = wave_row(), nw = wave_row_step();
  for (int64_t r = wave; r < B * n; r += nw) {
    const int64_t b = r / n, j = r - b * n;
    u32x4_t* dp = (u32x4_t*)(dst + (b * dst_rows + dst_off + j) * D);
    if (src != nullptr) {   // (kernel argument: uniform)
      const u32x4_t* sp = (const u32x4_t*)(src + (b * src_rows + src_off + j) * D);
      for (int c = lane; c < D / 8; c += 64) dp[c] = sp[c];
    } else {
      for (int c = lane; c < D / 8; c += 64) dp[c] = (u32x4_t){0u, 0u, 0u, 0u};
    }
  }
}

extern "C" int vj_copy_rows(const void* src, void* dst, int64_t B, int64_t src_rows, int64_t src_off,
                            int64_t dst_rows, int64_t dst_off, int64_t n, int64_t D, hipStream_t stream) {
  VJ_CHECK_ARG(D % 8 == 0, "vj_copy_rows: D must be a multiple of 8");
  VJ_CHECK_ARG((src == nullptr || src_off + n <= src_rows) && dst_off + n <= dst_rows, "vj_copy_rows: slice out of range");
  if (B * n == 0) return 0;
  hipLaunchKernelGGL(copy_rows_kernel, dim3(rows_grid(B * n)), dim3(256), 0, stream, (const bf16_t*)src,
                     (bf16_t*)dst, B, src_rows, src_off, dst_rows, dst_off, n, (int)D);
  VJ_LAUNCH_CHECK("vj_copy_rows");
  return 0;
}

// ---------------------------------------------------------------------------------------------
// add_pos: x[b,k,:] (bf16) += pos[idx ? idx[b,k] : k, :] (fp32), fp32 add, one rounding.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void add_pos_kernel(bf16_t* __restrict__ x, const float* __restrict__ pos,
                                                      const int64_t* __restrict__ idx, int64_t rows, int64_t K,
                                                      int D) {
  const int lane = wave_lane();
  const int64_t wave = wave_row(), nw = wave_row_step();
  for (int64_t r = wave; r < rows; r += nw) {
    const int64_t n = idx ? idx[r] : (r % K);
    bf16_t* xp = x + r * D;
    const float* pp = pos + n * D;
    for (int c = lane * 8; c < D; c += 512) {
      *(u32x4_t*)(xp + c) = add_pos8(*(const u32x4_t*)(xp + c), pp + c);
    }
  }
}

extern "C" int vj_add_pos(void* x_bf16, const float* pos, const int64_t* idx, int64_t B, int64_t K, int64_t D,
                          hipStream_t stream) {
  VJ_CHECK_ARG(D % 8 == 0, "vj_add_pos: D=%ld must be a multiple of 8", (long)D);
  const int64_t rows = B * K;
  if (rows == 0) return 0;
  hipLaunchKernelGGL(add_pos_kernel, dim3(rows_grid(rows)), dim3(256), 0, stream, (bf16_t*)x_bf16, pos, idx, rows, K,
                     (int)D);
  VJ_LAUNCH_CHECK("vj_add_pos");
  return 0;
}

// ---------------------------------------------------------------------------------------------
// add_pos_bcast: out[b, t*S + s, :] = bf16(float(y[b,s,:]) + pos[t*S + s, :]), t < Gt.  y = patch embedding of the S
// distinct tubelets of a still image; the Gt temporal slices of the repeated clip share it and differ only in their
// position rows.  The add is add_pos_kernel's (fp32, one rounding), so out equals add_pos on the Gt-fold repeated rows
// bit for bit.  One wave per (b,s): y is read once, Gt position rows are read and Gt output rows written.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void add_pos_bcast_kernel(const bf16_t* __restrict__ y, const float* __restrict__ pos,
                                                            bf16_t* __restrict__ out, int64_t rows, int64_t S, int64_t Gt,
                                                            int D) {
  const int lane = wave_lane();
  const int64_t wave = wave_row(), nw = wave_row_step();
  for (int64_t r = wave; r < rows; r += nw) {
    const int64_t b = r / S, s = r - b * S;
    const bf16_t* yp = y + r * D;
    for (int c = lane * 8; c < D; c += 512) {
      const u32x4_t v = *(const u32x4_t*)(yp + c);
      for (int64_t t = 0; t < Gt; t++) {
        *(u32x4_t*)(out + ((b * Gt + t) * S + s) * D + c) = add_pos8(v, pos + (t * S + s) * D + c);
      }
    }
  }
}

extern "C" int vj_add_pos_bcast(const void* y_bf16, const float* pos, void* out_bf16, int64_t B, int64_t S, int64_t Gt,
                                int64_t D, hipStream_t stream) {
  VJ_CHECK_ARG(B >= 0 && S >= 0 && Gt >= 0 && D > 0, "vj_add_pos_bcast: bad dims B=%ld S=%ld Gt=%ld D=%ld", (long)B, (long)S,
               (long)Gt, (long)D);
  VJ_CHECK_ARG(D % 8 == 0, "vj_add_pos_bcast: D=%ld must be a multiple of 8", (long)D);
  const int64_t rows = B * S;
  if (rows * Gt == 0) return 0;
  hipLaunchKernelGGL(add_pos_bcast_kernel, dim3(rows_grid(rows)), dim3(256), 0, stream, (const bf16_t*)y_bf16, pos,
                     (bf16_t*)out_bf16, rows, S, Gt, (int)D);
  VJ_LAUNCH_CHECK("vj_add_pos_bcast");
  return 0;
}

// ---------------------------------------------------------------------------------------------
// slice_sum: dy[b,s,:] = bf16(sum_{t<Gt} float(dx[b, t*S + s, :])), the adjoint of add_pos_bcast: the gradient of the S distinct
// patch embeddings of a still image is the sum of the gradients of the Gt temporal slices they were fanned out to.  fp32, slice 0
// first and then one plain add per slice in ascending t (no tree: the order is part of the contract), one rounding at the end;
// Gt == 1 moves the bits.  One wave per output row (b,s), one lane per 16-byte chunk of it; the lane's Gt source chunks sit S*D
// elements apart and are fetched four at a time before they are added, so four 16-byte loads are in flight per lane.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void slice_sum_kernel(const bf16_t* __restrict__ dx, bf16_t* __restrict__ dy, int64_t rows,
                                                        int64_t S, int64_t Gt, int64_t D) {
  const int lane = wave_lane();
  const int64_t wave = wave_row(), nw = wave_row_step();
  const int64_t step = S * D;
  for (int64_t r = wave; r < rows; r += nw) {
    const int64_t b = r / S, s = r - b * S;
    const bf16_t* sp = dx + (b * Gt * S + s) * D;   // slice 0 of this row; slice t is t * step further on
    bf16_t* op = dy + r * D;
    for (int64_t c = (int64_t)lane * 8; c < D; c += 512) {
      const u32x4_t w0 = *(const u32x4_t*)(sp + c);
      if (Gt == 1) {   // (kernel argument: uniform)
        *(u32x4_t*)(op + c) = w0;
        continue;
      }
      float acc[8], v[8];
      unpack8(w0, acc);
      int64_t t = 1;
      for (; t + 4 <= Gt; t += 4) {
        u32x4_t w[4];
#pragma unroll
        for (int i = 0; i < 4; i++) w[i] = *(const u32x4_t*)(sp + (t + i) * step + c);
#pragma unroll
        for (int i = 0; i < 4; i++) {
          unpack8(w[i], v);
#pragma unroll
          for (int j = 0; j < 8; j++) acc[j] = acc[j] + v[j];
        }
      }
      for (; t < Gt; t++) {
        load8(sp + t * step + c, v);
#pragma unroll
        for (int j = 0; j < 8; j++) acc[j] = acc[j] + v[j];
      }
      store8(op + c, acc);
    }
  }
}

extern "C" int vj_slice_sum(const void* dx_bf16, void* dy_bf16, int64_t B, int64_t S, int64_t Gt, int64_t D, hipStream_t stream) {
  VJ_CHECK_ARG(B >= 0 && S >= 0 && Gt >= 0 && D > 0, "vj_slice_sum: bad dims B=%ld S=%ld Gt=%ld D=%ld", (long)B, (long)S, (long)Gt,
               (long)D);
  VJ_CHECK_ARG(D % 8 == 0, "vj_slice_sum: D=%ld must be a multiple of 8", (long)D);
  const int64_t rows = B * S;
  if (rows * Gt == 0) return 0;
  int64_t n = 0;
  VJ_CHECK_ARG(!__builtin_mul_overflow(B, S, &n) && !__builtin_mul_overflow(n, Gt, &n) && !__builtin_mul_overflow(n, D, &n) &&
                   n <= INT64_MAX / 2,
               "vj_slice_sum: B=%ld S=%ld Gt=%ld D=%ld overflows the element offsets", (long)B, (long)S, (long)Gt, (long)D);
  VJ_CHECK_ARG(dx_bf16 != nullptr && dy_bf16 != nullptr, "vj_slice_sum: null pointer");
  VJ_CHECK_ARG(dx_bf16 != dy_bf16, "vj_slice_sum: dx and dy must differ (the sum is not done in place)");
  VJ_CHECK_ARG(((uintptr_t)dx_bf16 | (uintptr_t)dy_bf16) % 16 == 0, "vj_slice_sum: dx and dy must be 16-byte aligned");
  hipLaunchKernelGGL(slice_sum_kernel, dim3(rows_grid(rows)), dim3(256), 0, stream, (const bf16_t*)dx_bf16, (bf16_t*)dy_bf16, rows,
                     S, Gt, D);
  VJ_LAUNCH_CHECK("vj_slice_sum");
  return 0;
}

// ---------------------------------------------------------------------------------------------
// add_pos_frames: x[b, f*N + n, :] (bf16) += pos[idx[b,f], :] (fp32), the temporal position embedding of FrameAggregation
// (evals/video_classification_frozen/utils.py:74-80): every token of frame f of sample b takes the table row of that frame's
// index.  add_pos_kernel's add (fp32, one rounding).  One wave per token row; idx values were validated on the host and are
// clamped into [0, max_frames) here all the same, so no row outside the table is ever read.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void add_pos_frames_kernel(bf16_t* __restrict__ x, const float* __restrict__ pos,
                                                             const int64_t* __restrict__ idx, int64_t rows, int64_t N, int D,
                                                             int64_t max_frames) {
  const int lane = wave_lane();
  const int64_t wave = wave_row(), nw = wave_row_step();
  for (int64_t r = wave; r < rows; r += nw) {
    int64_t n = idx[r / N];   // rows = B*F*N, idx is [B,F]: row r belongs to frame r / N
    n = n < 0 ? 0 : (n > max_frames - 1 ? max_frames - 1 : n);
    bf16_t* xp = x + r * D;
    const float* pp = pos + n * D;
    for (int c = lane * 8; c < D; c += 512) {
      *(u32x4_t*)(xp + c) = add_pos8(*(const u32x4_t*)(xp + c), pp + c);
    }
  }
}

extern "C" int vj_add_pos_frames(void* x_bf16, const float* pos, const int64_t* idx, int64_t B, int64_t F, int64_t N, int64_t D,
                                 int64_t max_frames, hipStream_t stream) {
  VJ_CHECK_ARG(B >= 0 && F >= 0 && N >= 0 && D > 0 && max_frames > 0, "vj_add_pos_frames: bad dims B=%ld F=%ld N=%ld D=%ld max_frames=%ld",
               (long)B, (long)F, (long)N, (long)D, (long)max_frames);
  VJ_CHECK_ARG(D % 8 == 0, "vj_add_pos_frames: D=%ld must be a multiple of 8", (long)D);
  const int64_t rows = B * F * N;
  if (rows == 0) return 0;
  VJ_CHECK_ARG(x_bf16 != nullptr && pos != nullptr && idx != nullptr, "vj_add_pos_frames: null pointer");
  VJ_CHECK_ARG(((uintptr_t)x_bf16 | (uintptr_t)pos) % 16 == 0, "vj_add_pos_frames: x and pos must be 16-byte aligned");
  hipLaunchKernelGGL(add_pos_frames_kernel, dim3(rows_grid(rows)), dim3(256), 0, stream, (bf16_t*)x_bf16, pos, idx, rows, N,
                     (int)D, max_frames);
  VJ_LAUNCH_CHECK("vj_add_pos_frames");
  return 0;
}

// ---------------------------------------------------------------------------------------------
// pred_assemble_fwd: out[b, j, :] = j < Ke ? e[b,j,:] + pos[idx_e[b,j]] : tok[:] + pos[idx_p[b,j-Ke]]
//   e  = predictor_embed(z)   bf16 [B,Ke,Dp]     (predictor.py:194-200)
//   tok = mask_tokens[i]      fp32 [Dp]          (predictor.py:207-217)
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void pred_assemble_kernel(const bf16_t* __restrict__ e, const float* __restrict__ tok,
                                                            const float* __restrict__ pos,
                                                            const int64_t* __restrict__ idx_e,
                                                            const int64_t* __restrict__ idx_p,
                                                            bf16_t* __restrict__ out, int64_t B, int64_t Ke,
                                                            int64_t Kp, int D) {
  const int lane = wave_lane();
  const int64_t wave = wave_row(), nw = wave_row_step();
  const int64_t S = Ke + Kp;
  for (int64_t r = wave; r < B * S; r += nw) {
    const int64_t b = r / S, j = r - b * S;
    const bool ctx = j < Ke;
    const int64_t n = ctx ? idx_e[b * Ke + j] : idx_p[b * Kp + (j - Ke)];
    const float* pp = pos + n * D;
    const bf16_t* ep = e + (b * Ke + j) * D;
    bf16_t* op = out + r * D;
    for (int c = lane * 8; c < D; c += 512) {
      float v[8];
      if (ctx) {
        const u32x4_t w = *(const u32x4_t*)(ep + c);
#pragma unroll
        for (int i = 0; i < 4; i++) {
          v[2 * i] = bf_lo(w[i]);
          v[2 * i + 1] = bf_hi(w[i]);
        }
      } else {
#pragma unroll
        for (int i = 0; i < 8; i++) v[i] = tok[c + i];
      }
      u32x4_t o;
#pragma unroll
      for (int i = 0; i < 4; i++) o[i] = pack_bf2(v[2 * i] + pp[c + 2 * i], v[2 * i + 1] + pp[c + 2 * i + 1]);
      *(u32x4_t*)(op + c) = o;
    }
  }
}

extern "C" int vj_pred_assemble_fwd(const void* e_bf16, const float* mask_token, const float* pos,
                                    const int64_t* idx_e, const int64_t* idx_p, void* out_bf16, int64_t B,
                                    int64_t Ke, int64_t Kp, int64_t D, hipStream_t stream) {
  VJ_CHECK_ARG(D % 8 == 0, "vj_pred_assemble_fwd: D=%ld must be a multiple of 8", (long)D);
  const int64_t rows = B * (Ke + Kp);
  if (rows == 0) return 0;
  hipLaunchKernelGGL(pred_assemble_kernel, dim3(rows_grid(rows)), dim3(256), 0, stream, (const bf16_t*)e_bf16,
                     mask_token, pos, idx_e, idx_p, (bf16_t*)out_bf16, B, Ke, Kp, (int)D);
  VJ_LAUNCH_CHECK("vj_pred_assemble_fwd");
  return 0;
}
