// Mixup / cutmix of a batch of fp32 clips with its flipped self, in place: sample i of B is mixed with sample B-1-i.  One thread owns
// a 16-byte chunk of a row of BOTH samples of a pair (i, B-1-i), i < B/2: it reads both originals and then writes both results, so no
// second buffer is needed and the order of the pairs cannot matter.  A stream at memory rate without LDS; what a plan leaves alone
// (outside a cutmix box, a side with lam == 1) is neither read nor written.
//
// Reference behaviour restated (never copied): the ViT lineage's batch-mode mixup (x = lam * x + (1 - lam) * x.flip(0)) and cutmix
// (x[..., y0:y1, x0:x1] = x.flip(0)[..., y0:y1, x0:x1]) as the VideoMAE fine-tuning recipe applies them to a batch of clips.  The
// V-JEPA reference has neither; the draws stay on the host (jepa_amd/evals/mix.py).
#include "common.hpp"
#include "../../include/vjepa_hip.h"

struct mix_side {
  float lam, om;            // lam and fp32(1 - lam)
  int y0, y1, x0, x1;       // the box: rows y0 .. y1-1, columns x0 .. x1-1
};

__device__ __forceinline__ mix_side mix_side_load(const float* __restrict__ lam, const int32_t* __restrict__ box, int64_t b) {
  mix_side s;
  s.lam = lam[b];
  s.om = 1.0f - s.lam;
  s.y0 = box[4 * b], s.y1 = box[4 * b + 1], s.x0 = box[4 * b + 2], s.x1 = box[4 * b + 3];
  return s;
}
__device__ __forceinline__ bool mix_side_idle(const mix_side& s) { return s.lam == 1.0f && (s.y0 >= s.y1 || s.x0 >= s.x1); }

// one element of a side: `own` is this sample's value, `other` its partner's.  Inside the box the partner's bits; outside it with
// lam == 1 the own bits; otherwise lam * own + (1 - lam) * other with the product (1 - lam) * other rounded on its own and the rest
// fused -- three fp32 roundings with that of 1 - lam.  The fused multiply-add is written out, as in drop_path.hip.
__device__ __forceinline__ uint32_t mix_element(const mix_side& s, bool inside, uint32_t own, uint32_t other) {
  const float blend = fmaf(s.lam, __uint_as_float(own), s.om * __uint_as_float(other));
  return inside ? other : (s.lam == 1.0f ? own : __float_as_uint(blend));
}

// x [B, n4 chunks of 4 floats]; a chunk q of a sample lies in row (q / w4) % H at columns 4 * (q % w4) .. + 3.
__global__ __launch_bounds__(256) void clip_mix_kernel(float* __restrict__ x, const float* __restrict__ lam, const int32_t* __restrict__ box,
                                                       int64_t B, uint32_t n4, uint32_t w4, uint32_t H) {
  const int64_t pairs = B / 2;
  for (int64_t i = blockIdx.y; i < pairs; i += gridDim.y) {
    const int64_t j = B - 1 - i;
    const mix_side si = mix_side_load(lam, box, i), sj = mix_side_load(lam, box, j);   // (the same addresses in every lane)
    if (mix_side_idle(si) && mix_side_idle(sj)) continue;                                // the whole pair: not read
    u32x4_t* xi = (u32x4_t*)(x + i * (int64_t)n4 * 4);
    u32x4_t* xj = (u32x4_t*)(x + j * (int64_t)n4 * 4);
    for (uint64_t q64 = (uint64_t)blockIdx.x * 256 + threadIdx.x; q64 < n4; q64 += (uint64_t)gridDim.x * 256) {
      const uint32_t q = (uint32_t)q64;
      const uint32_t row = q / w4;
      const int c0 = (int)(q - row * w4) * 4, y = (int)(row % H);
      // does the chunk hold an element of the side's box?  does the side change in this chunk at all?
      const bool rows_i = y >= si.y0 && y < si.y1, rows_j = y >= sj.y0 && y < sj.y1;
      const bool hit_i = rows_i && c0 < si.x1 && c0 + 4 > si.x0, hit_j = rows_j && c0 < sj.x1 && c0 + 4 > sj.x0;
      const bool touch_i = hit_i || si.lam != 1.0f, touch_j = hit_j || sj.lam != 1.0f;
      if (!touch_i && !touch_j) continue;
      const u32x4_t a = xi[q], b = xj[q];
      if (touch_i) {
        u32x4_t o;
#pragma unroll
        for (int e = 0; e < 4; e++) o[e] = mix_element(si, rows_i && c0 + e >= si.x0 && c0 + e < si.x1, a[e], b[e]);
        xi[q] = o;
      }
      if (touch_j) {
        u32x4_t o;
#pragma unroll
        for (int e = 0; e < 4; e++) o[e] = mix_element(sj, rows_j && c0 + e >= sj.x0 && c0 + e < sj.x1, b[e], a[e]);
        xj[q] = o;
      }
    }
  }
}

// every argument is refused on the host, before any HIP call
static int clip_mix_check(const char* who, const float* x, const float* lam, const int32_t* box, int64_t B, int64_t P, int64_t H,
                          int64_t W, int64_t* per_sample) {
  VJ_CHECK_ARG(B >= 0 && P >= 0 && H >= 0 && W >= 0, "%s: bad dims B=%ld P=%ld H=%ld W=%ld", who, (long)B, (long)P, (long)H, (long)W);
  VJ_CHECK_ARG(W % 4 == 0, "%s: W=%ld must be a multiple of 4", who, (long)W);
  int64_t n = P;
  VJ_CHECK_ARG(H == 0 || n <= INT64_MAX / H, "%s: B*P*H*W overflows", who);
  n *= H;
  VJ_CHECK_ARG(W == 0 || n <= INT64_MAX / W, "%s: B*P*H*W overflows", who);
  n *= W;
  VJ_CHECK_ARG(n == 0 || B <= INT64_MAX / 4 / n, "%s: B*P*H*W overflows", who);
  *per_sample = n;
  if (B == 0 || n == 0) return 0;
  VJ_CHECK_ARG(n / 4 <= (int64_t)INT32_MAX && H <= (int64_t)INT32_MAX, "%s: P*H*W=%ld per sample exceeds 2^33", who, (long)n);
  VJ_CHECK_ARG(x != nullptr && lam != nullptr && box != nullptr, "%s: null pointer", who);
  VJ_CHECK_ARG((uintptr_t)x % 16 == 0 && (uintptr_t)lam % 4 == 0 && (uintptr_t)box % 4 == 0, "%s: x must be 16-byte aligned", who);
  return 0;
}

extern "C" int vj_clip_mix(float* x, const float* lam, const int32_t* box, int64_t B, int64_t P, int64_t H, int64_t W,
                           hipStream_t stream) {
  int64_t n = 0;
  if (int rc = clip_mix_check("vj_clip_mix", x, lam, box, B, P, H, W, &n)) return rc;
  if (B < 2 || n == 0) return 0;   // no pair: nothing to mix
  const int64_t n4 = n / 4, pairs = B / 2;
  const int gx = flat_grid(n4, 2048);
  int64_t gy = 4096 / gx;
  if (gy > pairs) gy = pairs;
  if (gy < 1) gy = 1;
  hipLaunchKernelGGL(clip_mix_kernel, dim3(gx, (unsigned)gy), dim3(256), 0, stream, x, lam, box, B, (uint32_t)n4, (uint32_t)(W / 4),
                     (uint32_t)H);
  VJ_LAUNCH_CHECK("vj_clip_mix");
  return 0;
}
