// Soft-target cross-entropy of fp32 logits against a smoothed two-label target, one wave per row: the loss of every row, the
// gradient softmax - target and (optionally) the soft-max itself in three passes over a row that stays in cache.  The target
//   t_c = eps / C + (1 - eps) * (lam * [c == a] + (1 - lam) * [c == b])
// is never materialised: the loss is lse - (1 - eps) * (lam * z_a + (1 - lam) * z_b) - (eps / C) * sum_c z_c.
//
// Reference behaviour restated (never copied): the ViT lineage's mixup_target (label smoothing applied to both one-hot rows, which
// are then blended with lam) and SoftTargetCrossEntropy (sum(-t * log_softmax(z), dim=-1).mean()); the V-JEPA reference trains its
// probes with the hard nn.CrossEntropyLoss (evals/video_classification_frozen/eval.py:309), which eps = 0, lam = 1 gives.
#include "common.hpp"
#include "../../include/vjepa_hip.h"

__global__ __launch_bounds__(256) void soft_ce_kernel(const float* __restrict__ logits, int64_t ld, const int32_t* __restrict__ label_a,
                                                      const int32_t* __restrict__ label_b, const float* __restrict__ lam, float eps,
                                                      int64_t R, int C, float* __restrict__ loss, float* __restrict__ dlogits,
                                                      float* __restrict__ probs) {
  const int lane = wave_lane();
  const int64_t wave = wave_row(), nw = wave_row_step();
  const float uni = eps / (float)C, keep = 1.0f - eps;
  for (int64_t r = wave; r < R; r += nw) {
    const float* z = logits + r * ld;
    // labels outside [0, C) are refused by the caller on the host; clamped here all the same, so that nothing outside the row is read
    const int a = min(max(label_a[r], 0), C - 1), b = min(max(label_b[r], 0), C - 1);
    // weights of the two label columns: a == b gives the one column the whole 1 - eps
    const float l = lam[r];
    const float wa = a == b ? keep : keep * l, wb = a == b ? 0.0f : keep * (1.0f - l);
    // pass 1: the maximum
    float m = -INFINITY;
    for (int c = lane; c < C; c += VJ_WAVE) m = fmaxf(m, z[c]);
    m = wave_max(m);
    // pass 2: sum exp(z - max) and sum z
    float se = 0.0f, sz = 0.0f;
    for (int c = lane; c < C; c += VJ_WAVE) {
      const float v = z[c];
      se += expf(v - m);
      sz += v;
    }
    se = wave_sum(se);
    sz = wave_sum(sz);
    if (lane == 0) loss[r] = (m + logf(se)) - (wa * z[a] + wb * z[b]) - uni * sz;
    // pass 3: the outputs
    const float inv = 1.0f / se;
    float* d = dlogits + r * (int64_t)C;
    float* p = probs ? probs + r * (int64_t)C : nullptr;
    for (int c = lane; c < C; c += VJ_WAVE) {
      const float pc = expf(z[c] - m) * inv;
      const float t = uni + (c == a ? wa : 0.0f) + (c == b ? wb : 0.0f);
      d[c] = pc - t;
      if (p) p[c] = pc;
    }
  }
}

extern "C" int vj_soft_ce(const float* logits, int64_t ld, const int32_t* label_a, const int32_t* label_b, const float* lam,
                          float smoothing, int64_t R, int64_t C, float* loss, float* dlogits, float* probs, hipStream_t stream) {
  const char* who = "vj_soft_ce";
  VJ_CHECK_ARG(R >= 0 && C >= 1 && C <= (int64_t)INT32_MAX, "%s: bad dims R=%ld C=%ld", who, (long)R, (long)C);
  VJ_CHECK_ARG(ld >= C, "%s: row stride ld=%ld is smaller than C=%ld", who, (long)ld, (long)C);
  VJ_CHECK_ARG(smoothing >= 0.0f && smoothing < 1.0f, "%s: smoothing=%g must lie in [0, 1)", who, (double)smoothing);
  VJ_CHECK_ARG(R == 0 || ld <= INT64_MAX / 4 / R, "%s: R*ld overflows", who);
  if (R == 0) return 0;
  VJ_CHECK_ARG(logits != nullptr && label_a != nullptr && label_b != nullptr && lam != nullptr && loss != nullptr && dlogits != nullptr,
               "%s: null pointer", who);
  VJ_CHECK_ARG(((uintptr_t)logits | (uintptr_t)label_a | (uintptr_t)label_b | (uintptr_t)lam | (uintptr_t)loss | (uintptr_t)dlogits |
                (uintptr_t)probs) % 4 == 0, "%s: buffers must be 4-byte aligned", who);
  hipLaunchKernelGGL(soft_ce_kernel, dim3(rows_grid(R)), dim3(256), 0, stream, logits, ld, label_a, label_b, lam, smoothing, R, (int)C,
                     loss, dlogits, probs);
  VJ_LAUNCH_CHECK("vj_soft_ce");
  return 0;
}
