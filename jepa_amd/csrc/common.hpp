// Shared device/host helpers for the V-JEPA gfx950 kernels.
// Everything here is CDNA4-only (wave64, MFMA, LDS-DMA); there is no other backend.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

typedef uint16_t bf16_t;  // raw bfloat16 bits in HBM

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8_t;
typedef __attribute__((ext_vector_type(4))) float f32x4_t;
typedef __attribute__((ext_vector_type(4))) uint32_t u32x4_t;
typedef __attribute__((ext_vector_type(2))) uint32_t u32x2_t;

#define VJ_WAVE 64

__device__ __forceinline__ float bf2f(bf16_t v) { return __uint_as_float(((uint32_t)v) << 16); }

// round-to-nearest-even, NaN preserved: identical to torch's float -> bfloat16
__device__ __forceinline__ bf16_t f2bf(float f) {
  uint32_t u = __float_as_uint(f);
  if ((u & 0x7fffffffu) > 0x7f800000u) return (bf16_t)((u >> 16) | 0x40u);
  u += 0x7fffu + ((u >> 16) & 1u);
  return (bf16_t)(u >> 16);
}
// two fp32 -> packed bf16x2 (RNE); lowers to one v_cvt_pk_bf16_f32 on gfx950
__device__ __forceinline__ uint32_t pack_bf2(float lo, float hi) {
  typedef __bf16 bf2_t __attribute__((ext_vector_type(2)));
  bf2_t v = {(__bf16)lo, (__bf16)hi};
  return __builtin_bit_cast(uint32_t, v);
}
// the same, opaque to the optimiser: when only the UNPACKED halves of the result are used, hipcc otherwise converts each
// element on its own (v_cvt_pk_bf16_f32 with a dummy partner) -- twice the conversions
__device__ __forceinline__ uint32_t pack_bf2_opaque(float lo, float hi) {
  uint32_t w = pack_bf2(lo, hi);
  asm("" : "+v"(w));
  return w;
}
__device__ __forceinline__ float bf_lo(uint32_t w) { return __uint_as_float(w << 16); }
__device__ __forceinline__ float bf_hi(uint32_t w) { return __uint_as_float(w & 0xffff0000u); }

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
// sum over the 16 lanes of a DPP row (lanes 16k .. 16k+15); every lane of the row receives the total.  Rotate-and-add with
// row_ror: four v_add_f32 with a DPP source, no LDS round trip (ds_bpermute: ~24 cycles of the LDS pipe each).
__device__ __forceinline__ float row16_sum(float v) {
  v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x128, 0xf, 0xf, false));   // row_ror:8
  v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x124, 0xf, 0xf, false));   // row_ror:4
  v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x122, 0xf, 0xf, false));   // row_ror:2
  v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x121, 0xf, 0xf, false));   // row_ror:1
  return v;
}
// sum over the four waves of a 256-thread workgroup, N values at once for one barrier: block4_stage leaves every wave's totals in
// red[k][wave] and synchronises; block4_total(red[k]) then adds them in the fixed order wave 0 + 1 + 2 + 3, in whichever threads want it
template <int N>
__device__ __forceinline__ void block4_stage(float (*red)[4], const float (&v)[N]) {
  float w[N];
#pragma unroll
  for (int k = 0; k < N; k++) w[k] = wave_sum(v[k]);
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int k = 0; k < N; k++) red[k][threadIdx.x >> 6] = w[k];
  }
  __syncthreads();
}
__device__ __forceinline__ float block4_total(const float* red) { return red[0] + red[1] + red[2] + red[3]; }
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}

// erf-GELU (nn.GELU() default, reference modules.py:32) and its derivative, 2-wide for the GEMM epilogues: the polynomial, the products
// and the final combination issue as v_pk_fma_f32 / v_pk_mul_f32 / v_pk_add_f32 (two elements per instruction); only exp2 and the sign
// handling stay scalar.  The fc1 epilogue of a layer that will run backward stores gelu'(u) (bf16) instead of the pre-activation u, and
// the fc2 dgrad epilogue only multiplies by it -- the backward never re-evaluates exp / the polynomial (u has no other consumer).
// q = Phi(-|x|) is exp2 of a polynomial.  Rounds 1-3 took it from erf by Abramowitz-Stegun 7.1.26 (one v_rcp + one v_exp + 4 FMAs +
// 3 multiplies, relu on the bit pattern); round 4 replaced that form and round 6 removed its run-time switch (docs/history/,
// profiles/r04_abab_gelu_poly.md).
// log2 Phi(-a) is a smooth, nearly quadratic function of a >= 0 (-1 at 0, ~ -a^2 log2(e)/2 - log2(a sqrt(2 pi)) far out), so
// q(a) = exp2(L(a)) with a degree-6 minimax polynomial L on [0, 5] (Lawson iteration, max |dL| 1.8e-5, i.e. q to 1.3e-5
// RELATIVE over the whole range, tail included) needs 6 FMAs and one v_exp, no reciprocal.
// a = min(|x|, 5) is ONE instruction (v_min_f32 with the |x| source modifier) and is used for the product a * q as
// well: beyond 5 the result is relu(x) - 5 q(5) = relu(x) - 1.4e-6 (exact: relu(x) - |x| Phi(-|x|), at most 1.4e-6 there).
// Against the correctly rounded bf16 erf-GELU over ALL finite bf16 inputs x > -5: 5 of 20712 results differ (by one bf16 ulp);
// the A-S form: 22 (tests/test_gelu_poly.py enumerates them on the CPU with this arithmetic).  relu(x) is taken as
// 0.5 * (x + |x|): exact for finite x, and a NaN of EITHER sign propagates.
typedef float f32x2_t __attribute__((ext_vector_type(2)));
// x + |x| = 2 relu(x) as ONE v_add_f32 with the |x| source modifier (hipcc turns the C expression into v_and + a packed add);
// exact for |x| < 2^127 (no cancellation error for negative x, unlike 0.5 x + 0.5 |x| - ...), +inf above; a NaN of either sign stays a NaN
__device__ __forceinline__ float twice_relu(float x) {
  float s;
  asm("v_add_f32 %0, %1, |%1|" : "=v"(s) : "v"(x));
  return s;
}
__device__ __forceinline__ f32x2_t half_erfc2_lp(f32x2_t x, f32x2_t& a) {
  // v_med3_f32 a, |x|, 0, 5: one instruction (fminf(fabsf(x), 5) costs a canonicalising v_max + v_min + v_and)
  a = (f32x2_t){__builtin_amdgcn_fmed3f(__builtin_fabsf(x[0]), 0.0f, 5.0f), __builtin_amdgcn_fmed3f(__builtin_fabsf(x[1]), 0.0f, 5.0f)};
  const f32x2_t c6 = {2.945814386e-05f, 2.945814386e-05f}, c5 = {-7.087827263e-04f, -7.087827263e-04f},
                 c4 = {7.746013931e-03f, 7.746013931e-03f}, c3 = {-5.260629358e-02f, -5.260629358e-02f},
                 c2 = {-4.596254594e-01f, -4.596254594e-01f}, c1 = {-1.150867238e+00f, -1.150867238e+00f},
                 c0 = {-1.000017643e+00f, -1.000017643e+00f};
  f32x2_t p = __builtin_elementwise_fma(c6, a, c5);
  p = __builtin_elementwise_fma(p, a, c4);
  p = __builtin_elementwise_fma(p, a, c3);
  p = __builtin_elementwise_fma(p, a, c2);
  p = __builtin_elementwise_fma(p, a, c1);
  p = __builtin_elementwise_fma(p, a, c0);
  return (f32x2_t){__builtin_amdgcn_exp2f(p[0]), __builtin_amdgcn_exp2f(p[1])};
}
// gelu(x) = relu(x) - a q(a)
__device__ __forceinline__ f32x2_t gelu2_lp(f32x2_t x) {
  f32x2_t a;
  const f32x2_t q = half_erfc2_lp(x, a);
  const f32x2_t s = {twice_relu(x[0]), twice_relu(x[1])};
  const f32x2_t half = {0.5f, 0.5f};
  return __builtin_elementwise_fma(s, half, -(a * q));
}
// gelu(x) and gelu'(x) = Phi(x) + x pdf(x): Phi from the same q, the Gaussian term from its own v_exp
__device__ __forceinline__ void gelu_dgelu2_lp(f32x2_t x, f32x2_t& y, f32x2_t& d) {
  f32x2_t a;
  const f32x2_t q = half_erfc2_lp(x, a);
  const f32x2_t s = {twice_relu(x[0]), twice_relu(x[1])};
  const f32x2_t half = {0.5f, 0.5f};
  y = __builtin_elementwise_fma(s, half, -(a * q));                                  // = gelu2_lp(x), bit for bit
  const f32x2_t c = {-0.72134752044448170f, -0.72134752044448170f};                  // -0.5 * log2(e)
  const f32x2_t e = (x * c) * x;
  const f32x2_t g = {__builtin_amdgcn_exp2f(e[0]), __builtin_amdgcn_exp2f(e[1])};    // exp(-x^2/2)
  const f32x2_t hq = half - q;
  const f32x2_t phi = half + (f32x2_t){copysignf(hq[0], x[0]), copysignf(hq[1], x[1])};
  const f32x2_t k = {0.3989422804014327f, 0.3989422804014327f};
  d = __builtin_elementwise_fma(x * k, g, phi);
}

// XCD-aware band mapping (bijective for any grid size): workgroup `bid` of `nblk` -> logical index such that each XCD (private L2;
// hardware dispatches workgroup b to XCD b % 8) works on a contiguous band of tiles (GEMM) or of (sample, head, block) items (attention).
__device__ __forceinline__ int xcd_logical(int bid, int nblk) {
  const int qx = nblk >> 3, rx = nblk & 7, xcd = bid & 7, pos = bid >> 3;
  return (xcd < rx ? xcd * (qx + 1) : rx * (qx + 1) + (xcd - rx) * qx) + pos;
}

// ---- per-device one-time setup ------------------------------------------------------------------------------------
// Function attributes (dynamic LDS limit), event pools and small constant buffers belong to a DEVICE, not to the process:
// a host that drives several GPUs from one process (not this package's own launcher: one process per GPU) calls the C ABI
// with different current devices.  vj_device_slot() = current HIP device (0 on error); VjPerDeviceOnce runs an idempotent
// setup once per device (a lost race repeats it harmlessly).
#include <atomic>
#define VJ_MAX_DEVICES 64
inline int vj_device_slot() {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0) dev = 0;
  return dev % VJ_MAX_DEVICES;
}
struct VjPerDeviceOnce {
  std::atomic<unsigned long long> done{0};
  template <class F>
  void operator()(F&& f) {
    const unsigned long long bit = 1ull << vj_device_slot();
    if (!(done.load(std::memory_order_acquire) & bit)) {
      f();
      done.fetch_or(bit, std::memory_order_release);
    }
  }
};

// ---- host side error plumbing (no C++ exception crosses the C ABI) ----
extern "C" const char* vj_last_error(void);
void vj_set_error(const char* fmt, ...);

#define VJ_CHECK_ARG(cond, ...)            \
  do {                                     \
    if (!(cond)) {                         \
      vj_set_error(__VA_ARGS__);           \
      return -1;                           \
    }                                      \
  } while (0)

#define VJ_LAUNCH_CHECK(name)                                              \
  do {                                                                     \
    hipError_t _e = hipGetLastError();                                     \
    if (_e != hipSuccess) {                                                \
      vj_set_error("%s: launch failed: %s", name, hipGetErrorString(_e)); \
      return (int)_e;                                                      \
    }                                                                      \
  } while (0)

__host__ __device__ static inline int64_t cdiv64(int64_t a, int64_t b) { return (a + b - 1) / b; }

// ---- launch shapes of the HBM-bound kernels ----
// one wave per row, four waves per 256-thread workgroup, at most cap_blocks workgroups (256 * 8 for the LayerNorm family)
static inline int rows_grid(int64_t rows, int64_t cap_blocks = 256 * 16) {
  int64_t g = cdiv64(rows, 4);
  if (g > cap_blocks) g = cap_blocks;
  if (g < 1) g = 1;
  return (int)g;
}
// one thread per item in 256-thread workgroups, at most cap_blocks of them (the kernels stride by the grid)
static inline int flat_grid(int64_t total, int64_t cap_blocks) {
  int64_t g = cdiv64(total, 256);
  if (g > cap_blocks) g = cap_blocks;
  return (int)g;
}
// the kernel's side of rows_grid: this lane's index in its wave, the first row of its wave, and the step to the wave's next row
__device__ __forceinline__ int wave_lane() { return threadIdx.x & 63; }
__device__ __forceinline__ int64_t wave_row() { return (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); }
__device__ __forceinline__ int64_t wave_row_step() { return (int64_t)gridDim.x * 4; }

// ---- 16-byte bf16 chunks ----
// 8 bf16 in registers -> 8 fp32; the same from memory; 8 fp32 -> 8 bf16 (RNE) to memory
__device__ __forceinline__ void unpack8(const u32x4_t& w, float* v) {
#pragma unroll
  for (int i = 0; i < 4; i++) {
    v[2 * i] = bf_lo(w[i]);
    v[2 * i + 1] = bf_hi(w[i]);
  }
}
__device__ __forceinline__ void load8(const bf16_t* p, float* v) { unpack8(*(const u32x4_t*)p, v); }
__device__ __forceinline__ void store8(bf16_t* p, const float* v) {
  u32x4_t w;
#pragma unroll
  for (int i = 0; i < 4; i++) w[i] = pack_bf2(v[2 * i], v[2 * i + 1]);
  *(u32x4_t*)p = w;
}
// 4 fp32 -> 4 bf16 (RNE): the shadow weights of optim.hip
__device__ __forceinline__ u32x2_t pack4_bf16(float a, float b, float c, float d) {
  u32x2_t w;
  w[0] = pack_bf2(a, b);
  w[1] = pack_bf2(c, d);
  return w;
}
// 8 fp32 -> 8 bf16 (RNE): the pixel packing of tubelet_pack / image_pack
__device__ __forceinline__ u32x4_t pack8_bf16(float4 lo, float4 hi) {
  u32x4_t o;
  o[0] = pack_bf2(lo.x, lo.y);
  o[1] = pack_bf2(lo.z, lo.w);
  o[2] = pack_bf2(hi.x, hi.y);
  o[3] = pack_bf2(hi.z, hi.w);
  return o;
}
// 8 bf16 + 8 fp32 position values -> 8 bf16: fp32 add, one rounding.  THE position add of add_pos / add_pos_bcast / add_pos_frames
__device__ __forceinline__ u32x4_t add_pos8(u32x4_t v, const float* pos) {
  const float4 p0 = *(const float4*)pos;
  const float4 p1 = *(const float4*)(pos + 4);
  v[0] = pack_bf2(bf_lo(v[0]) + p0.x, bf_hi(v[0]) + p0.y);
  v[1] = pack_bf2(bf_lo(v[1]) + p0.z, bf_hi(v[1]) + p0.w);
  v[2] = pack_bf2(bf_lo(v[2]) + p1.x, bf_hi(v[2]) + p1.y);
  v[3] = pack_bf2(bf_lo(v[3]) + p1.z, bf_hi(v[3]) + p1.w);
  return v;
}
