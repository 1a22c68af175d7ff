// Position-table interpolation of interpolate_pos_encoding (src/models/vision_transformer.py:197-246): trilinear for video
// grids, bicubic for the image branch, both on the channels-last view the reference permutes to and from.  InterpAxis and
// CubicAxis stay separate from each other and from input_pack.hip's ClipAxis: see the comment there.
#include "common.hpp"
#include "../../include/vjepa_hip.h"

// ---------------------------------------------------------------------------------------------
// pos_interp3d: fp32 table [Nt,Nh,Nw,D] -> [To,Ho,Wo,D], the trilinear F.interpolate(scale_factor=(st,sh,sw)) of
// interpolate_pos_encoding (src/models/vision_transformer.py:197-228) on the channels-last view it permutes to and from.
// align_corners=False with the scale factor GIVEN: per axis src = (dst + 0.5) * r - 0.5 clamped below at 0, with
// r = float(1 / scale) (not in/out); i0 = int(src), i1 = i0 + (i0 < in - 1), weights src - i0 and 1 - (src - i0).  The
// products and differences of the coordinate are kept unfused so they round as the plain expression does.  One thread
// per 4 output floats; the 8 corner rows are 16-byte loads.
// ---------------------------------------------------------------------------------------------
struct InterpAxis {
  int i0, i1;
  float w0, w1;
};

__device__ __forceinline__ InterpAxis interp_axis(int dst, float r, int in) {
  float src = __fsub_rn(__fmul_rn(r, (float)dst + 0.5f), 0.5f);
  if (src < 0.f) src = 0.f;
  int i0 = (int)src;
  if (i0 > in - 1) i0 = in - 1;
  float l = src - (float)i0;
  l = l < 0.f ? 0.f : (l > 1.f ? 1.f : l);
  InterpAxis a;
  a.i0 = i0;
  a.i1 = i0 + (i0 < in - 1 ? 1 : 0);
  a.w1 = l;
  a.w0 = 1.f - l;
  return a;
}

__global__ __launch_bounds__(256) void pos_interp3d_kernel(const float* __restrict__ in, float* __restrict__ out, int Nt,
                                                           int Nh, int Nw, int D, float rt, float rh, float rw, int To,
                                                           int Ho, int Wo) {
  const int dv = D / 4;
  const int64_t total = (int64_t)To * Ho * Wo * dv;
  for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q < total; q += (int64_t)gridDim.x * 256) {
    const int64_t cell = q / dv;
    const int c = (int)(q - cell * dv) * 4;
    const int w = (int)(cell % Wo), h = (int)((cell / Wo) % Ho), t = (int)(cell / ((int64_t)Wo * Ho));
    const InterpAxis at = interp_axis(t, rt, Nt), ah = interp_axis(h, rh, Nh), aw = interp_axis(w, rw, Nw);
    float4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int k = 0; k < 8; k++) {
      const int ti = (k & 4) ? at.i1 : at.i0, hi = (k & 2) ? ah.i1 : ah.i0, wi = (k & 1) ? aw.i1 : aw.i0;
      const float wt = ((k & 4) ? at.w1 : at.w0) * ((k & 2) ? ah.w1 : ah.w0) * ((k & 1) ? aw.w1 : aw.w0);
      const float4 v = *(const float4*)(in + (((int64_t)ti * Nh + hi) * Nw + wi) * D + c);
      acc.x += wt * v.x;
      acc.y += wt * v.y;
      acc.z += wt * v.z;
      acc.w += wt * v.w;
    }
    *(float4*)(out + cell * D + c) = acc;
  }
}

extern "C" int vj_pos_interp3d(const float* table, float* out, int64_t Nt, int64_t Nh, int64_t Nw, int64_t D, double scale_t,
                               double scale_h, double scale_w, int64_t To, int64_t Ho, int64_t Wo, hipStream_t stream) {
  VJ_CHECK_ARG(Nt > 0 && Nh > 0 && Nw > 0 && D > 0 && Nt < (1 << 20) && Nh < (1 << 20) && Nw < (1 << 20),
               "vj_pos_interp3d: bad table dims %ldx%ldx%ldx%ld", (long)Nt, (long)Nh, (long)Nw, (long)D);
  VJ_CHECK_ARG(D % 4 == 0, "vj_pos_interp3d: D=%ld must be a multiple of 4", (long)D);
  VJ_CHECK_ARG(scale_t > 0.0 && scale_h > 0.0 && scale_w > 0.0, "vj_pos_interp3d: scale factors must be positive");
  VJ_CHECK_ARG(To > 0 && Ho > 0 && Wo > 0 && To < (1 << 20) && Ho < (1 << 20) && Wo < (1 << 20),
               "vj_pos_interp3d: non-positive output grid %ldx%ldx%ld", (long)To, (long)Ho, (long)Wo);
  // F.interpolate's output extent for a given scale factor: floor(in * scale) in double
  VJ_CHECK_ARG(To == (int64_t)floor((double)Nt * scale_t) && Ho == (int64_t)floor((double)Nh * scale_h) &&
                   Wo == (int64_t)floor((double)Nw * scale_w),
               "vj_pos_interp3d: output grid %ldx%ldx%ld is not floor(in * scale)", (long)To, (long)Ho, (long)Wo);
  const int64_t total = To * Ho * Wo * (D / 4);
  hipLaunchKernelGGL(pos_interp3d_kernel, dim3(flat_grid(total, 256 * 32)), dim3(256), 0, stream, table, out, (int)Nt, (int)Nh, (int)Nw, (int)D,
                     (float)(1.0 / scale_t), (float)(1.0 / scale_h), (float)(1.0 / scale_w), (int)To, (int)Ho, (int)Wo);
  VJ_LAUNCH_CHECK("vj_pos_interp3d");
  return 0;
}

// ---------------------------------------------------------------------------------------------
// pos_interp2d_bicubic: fp32 table [Nh,Nw,D] -> [Ho,Wo,D], the bicubic F.interpolate(scale_factor=s) of the image branch of
// interpolate_pos_encoding (src/models/vision_transformer.py:230-246) on the channels-last view it permutes to and from.
// align_corners=False with the scale factor GIVEN: per axis src = (dst + 0.5) * r - 0.5 with r = float(1 / scale), NOT
// clamped at zero (only the linear modes clamp); i = floor(src), t = src - i; the four taps i-1 .. i+2 are clamped into
// [0, in-1] and weighted by the cubic convolution with A = -0.75:
//   w0 = ((A(t+1) - 5A)(t+1) + 8A)(t+1) - 4A,  w1 = ((A+2)t - (A+3))t^2 + 1,  w2 = w1(1-t),  w3 = w0(1-t).
// Rows are blended last, each an fp32 sum of its four columns.  One thread per 4 output floats; the 16 taps are 16-byte loads.
// ---------------------------------------------------------------------------------------------
struct CubicAxis {
  int i[4];
  float w[4];
};

__device__ __forceinline__ float cubic_near(float x) {   // |x| <= 1
  const float A = -0.75f;
  return ((A + 2.f) * x - (A + 3.f)) * x * x + 1.f;
}

__device__ __forceinline__ float cubic_far(float x) {   // 1 < |x| < 2
  const float A = -0.75f;
  return ((A * x - 5.f * A) * x + 8.f * A) * x - 4.f * A;
}

__device__ __forceinline__ CubicAxis cubic_axis(int dst, float r, int in) {
  const float src = __fsub_rn(__fmul_rn(r, (float)dst + 0.5f), 0.5f);
  int i0 = (int)floorf(src);
  if (i0 > in - 1) i0 = in - 1;
  float t = src - (float)i0;
  t = t < 0.f ? 0.f : (t > 1.f ? 1.f : t);
  CubicAxis a;
#pragma unroll
  for (int k = 0; k < 4; k++) a.i[k] = min(max(i0 - 1 + k, 0), in - 1);
  a.w[0] = cubic_far(t + 1.f);
  a.w[1] = cubic_near(t);
  a.w[2] = cubic_near(1.f - t);
  a.w[3] = cubic_far((1.f - t) + 1.f);
  return a;
}

__global__ __launch_bounds__(256) void pos_interp2d_bicubic_kernel(const float* __restrict__ in, float* __restrict__ out,
                                                                   int Nh, int Nw, int D, float r, int Ho, int Wo) {
  const int dv = D / 4;
  const int64_t total = (int64_t)Ho * Wo * dv;
  for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q < total; q += (int64_t)gridDim.x * 256) {
    const int64_t cell = q / dv;
    const int c = (int)(q - cell * dv) * 4;
    const int w = (int)(cell % Wo), h = (int)(cell / Wo);
    const CubicAxis ah = cubic_axis(h, r, Nh), aw = cubic_axis(w, r, Nw);
    float4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const float* row = in + (int64_t)ah.i[j] * Nw * D + c;
      float4 s = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int k = 0; k < 4; k++) {
        const float4 v = *(const float4*)(row + (int64_t)aw.i[k] * D);
        s.x += aw.w[k] * v.x;
        s.y += aw.w[k] * v.y;
        s.z += aw.w[k] * v.z;
        s.w += aw.w[k] * v.w;
      }
      acc.x += ah.w[j] * s.x;
      acc.y += ah.w[j] * s.y;
      acc.z += ah.w[j] * s.z;
      acc.w += ah.w[j] * s.w;
    }
    *(float4*)(out + cell * D + c) = acc;
  }
}

extern "C" int vj_pos_interp2d_bicubic(const float* table, float* out, int64_t Nh, int64_t Nw, int64_t D, double scale,
                                       int64_t Ho, int64_t Wo, hipStream_t stream) {
  VJ_CHECK_ARG(Nh > 0 && Nw > 0 && D > 0 && Nh < (1 << 20) && Nw < (1 << 20), "vj_pos_interp2d_bicubic: bad table dims %ldx%ldx%ld",
               (long)Nh, (long)Nw, (long)D);
  VJ_CHECK_ARG(D % 4 == 0, "vj_pos_interp2d_bicubic: D=%ld must be a multiple of 4", (long)D);
  VJ_CHECK_ARG(scale > 0.0, "vj_pos_interp2d_bicubic: the scale factor must be positive");
  VJ_CHECK_ARG(Ho > 0 && Wo > 0 && Ho < (1 << 20) && Wo < (1 << 20), "vj_pos_interp2d_bicubic: non-positive output grid %ldx%ld",
               (long)Ho, (long)Wo);
  // F.interpolate's output extent for a given scale factor: floor(in * scale) in double
  VJ_CHECK_ARG(Ho == (int64_t)floor((double)Nh * scale) && Wo == (int64_t)floor((double)Nw * scale),
               "vj_pos_interp2d_bicubic: output grid %ldx%ld is not floor(in * scale)", (long)Ho, (long)Wo);
  VJ_CHECK_ARG(table != nullptr && out != nullptr, "vj_pos_interp2d_bicubic: null pointer");
  VJ_CHECK_ARG(((uintptr_t)table | (uintptr_t)out) % 16 == 0, "vj_pos_interp2d_bicubic: table and out must be 16-byte aligned");
  const int64_t total = Ho * Wo * (D / 4);
  hipLaunchKernelGGL(pos_interp2d_bicubic_kernel, dim3(flat_grid(total, 256 * 32)), dim3(256), 0, stream, table, out, (int)Nh, (int)Nw, (int)D,
                     (float)(1.0 / scale), (int)Ho, (int)Wo);
  VJ_LAUNCH_CHECK("vj_pos_interp2d_bicubic");
  return 0;
}
