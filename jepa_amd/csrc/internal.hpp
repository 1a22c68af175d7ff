// Functions that cross source files INSIDE the library and are not part of the C ABI (include/vjepa_hip.h), declared once:
// the file that defines one and every file that calls it include this header, so a signature cannot drift unnoticed.
#pragma once
#include "common.hpp"

// ---- layernorm.hip
// The LayerNorm backward kernel alone: dx is complete, the column partials part[*nb_out][nseg * D] (nseg = 3 with `cs`:
// dgamma | dbeta | column sums of dx; else 2) stay in `ws` for the caller to reduce.
int vj_layernorm_bwd_partials(const void* dy_bf16, const void* x_bf16, const float* gamma, const float* mean, const float* rstd,
                              const void* dres_bf16, void* dx_bf16, bool cs, int64_t rows, int64_t D, void* ws,
                              int64_t ws_bytes, int64_t* nb_out, hipStream_t stream);

// ---- reduce.hip
// out[n] = alpha * sum_p part[p * stride + n] + beta * out[n]
int vj_reduce_partials_strided(const float* part, float* out, int64_t P, int64_t N, int64_t stride, float alpha,
                               float beta, hipStream_t stream);
// part[p][k*D : (k+1)*D] -> outs[k], k < nseg <= 3, in one launch
int vj_reduce_partials_multi(const float* part, float* const* outs, int nseg, int64_t P, int64_t D, float alpha, float beta,
                             hipStream_t stream);

// ---- the launchers behind gemm.hip's dispatcher (GemmArgs, VJ_PERSIST_NA: gemm_common.hpp)
struct GemmArgs;
int vj_gemm_launch_8phase(const GemmArgs& a, int epilogue, void* ws, int64_t ws_bytes, hipStream_t stream);   // gemm8.hip
int vj_gemm_launch_4w(const GemmArgs& a, int epilogue, void* ws, int64_t ws_bytes, hipStream_t stream);       // gemm4w.hip
int vj_gemm_launch_8phase_persist(const GemmArgs& a, int epilogue, hipStream_t stream);   // gemm8p.hip; VJ_PERSIST_NA: does not apply
