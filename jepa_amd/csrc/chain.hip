// Whole-trunk launch chains: N transformer blocks forward / backward enqueued by ONE C call.
//
// Reference semantics (restated, never copied): Block / Attention / MLP forward of src/models/utils/modules.py:30-36,
// 61-78,114-120 and what autograd derives from them for app/vjepa/train.py:461-464.  The Python engine used to issue the
// ~1800 kernel launches of a step one ctypes call at a time (~39 us each: 70 ms of host time against an 85 ms GPU step);
// here the per-block sequence lives behind the C ABI, so the host cost of a block is 7 (forward) / ~25 (backward)
// hipLaunchKernel calls and nothing else.  No arithmetic happens in this file: it only sequences the kernels of
// gemm*.hip / attention.hip / layernorm.hip / rows.hip / reduce.hip, lays the saved activations out in a caller-provided workspace
// and orders the two HIP streams (dgrad chain on `stream`, weight gradients on `side`) with events.
//
// Saved-activation layout per block (workspace `save_ws`, everything 256-byte aligned, bf16 unless noted):
//   x [M,D] (block input; block 0 uses the caller's x_in), y1 [M,D], qkv [M,3D], o [M,D], x1 [M,D], y2 [M,D],
//   u [M,Dh] (gelu'(pre-activation): the saved GELU derivative), g [M,Dh], mean1 rstd1 mean2 rstd2 [M] fp32, lse2 [H*M] fp32 (per segment [B,H,S]).
// With save = 0 (EMA target encoder, inference) one such set is reused by every block and x ping-pongs.
//
// This file holds the two workspace layouts, the forward and the backward; the guard bands behind the layouts' members, the
// pool of ordering events and the launch profiler are chain_support.cpp.
#include "chain_support.hpp"
#include "internal.hpp"
#include "options.hpp"
#include "../../include/vjepa_hip.h"
#include <cmath>

static inline int64_t al256(int64_t n) { return (n + 255) / 256 * 256; }
static inline int64_t pad64i(int64_t m) { return (m + 63) / 64 * 64; }

// ---------------------------------------------------------------------------------------------------- workspace layouts
// Base of both layouts: take() hands out the members in order, each 256-byte aligned and, under option ws_guard, followed by a
// 256-byte gap whose offset is recorded for poison_gaps().
struct WsLayout {
  int64_t total = 0;   // the running offset while members are taken, the size of the layout afterwards
  int64_t gap[32];
  int n_gap = 0;
  const int64_t gg = guard_gap();
  int64_t take(int64_t bytes) {
    const int64_t o = total;
    total += al256(bytes);
    if (gg) {
      gap[n_gap++] = total;
      total += gg;
    }
    return o;
  }
};
static int poison_gaps(const WsLayout& L, char* base, hipStream_t st) {
  for (int k = 0; k < L.n_gap; k++) CH(poison_gap(base + L.gap[k], st));
  return 0;
}

struct FwdLayout : WsLayout {
  int64_t x, y1, qkv, o, x1, y2, u, g, mean1, rstd1, mean2, rstd2, lse, rs;
};
static FwdLayout fwd_layout(int64_t M, int64_t D, int64_t Dh, int64_t H) {
  FwdLayout L;
  L.x = L.take(M * D * 2);
  L.y1 = L.take(M * D * 2);
  L.qkv = L.take(M * 3 * D * 2);
  L.o = L.take(M * D * 2);
  L.x1 = L.take(M * D * 2);
  L.y2 = L.take(M * D * 2);
  L.u = L.take(M * Dh * 2);
  L.g = L.take(M * Dh * 2);
  L.mean1 = L.take(M * 4);
  L.rstd1 = L.take(M * 4);
  L.mean2 = L.take(M * 4);
  L.rstd2 = L.take(M * 4);
  L.lse = L.take(H * M * 4);
  L.rs = L.take(M * 8);   // {rstd, -mean * rstd} per row: the LayerNorm folded into the consuming GEMM (vj_blocks_fwd_lnfold)
  return L;
}

extern "C" int64_t vj_blocks_fwd_ws_bytes(int64_t M, int64_t D, int64_t Dh, int64_t heads, int64_t n_blocks, int save) {
  const FwdLayout L = fwd_layout(M, D, Dh, heads);
  return save ? L.total * n_blocks : L.total + al256(M * D * 2) + L.gg;
}

#define WGRAD_WS_BYTES ((int64_t)96 << 20)    // what the single weight-gradient launches are told they may use (their split factor follows)
#define GROUP_WS_BYTES ((int64_t)192 << 20)   // grouped weight gradients: 4 * sum N1*N2 (ViT-H: 79 MB) x split factor

struct BwdLayout : WsLayout {
  int64_t du[2], dx1[2], dqkv[2], dx[3], dy2, dob, dy1, delta, ln_ws, ln_ws2, colp_fc1, colp_q, colp_kv, dyT, xT, tcs_ws, wg_ws;
  int64_t ln_ws_bytes, tcs_ws_bytes, delta_bytes, colp_fc1_rows, colp_attn_rows;
};
static BwdLayout bwd_layout(int64_t M, int64_t D, int64_t Dh, int64_t H) {
  BwdLayout L;
  const int64_t Mp = pad64i(M), nmax = 3 * D > Dh ? 3 * D : Dh;
  for (int p = 0; p < 2; p++) {
    L.du[p] = L.take(M * Dh * 2);
    L.dx1[p] = L.take(M * D * 2);
    L.dqkv[p] = L.take(M * 3 * D * 2);
  }
  for (int p = 0; p < 3; p++) L.dx[p] = L.take(M * D * 2);
  L.dy2 = L.take(M * D * 2);
  L.dob = L.take(M * D * 2);
  L.dy1 = L.take(M * D * 2);
  L.delta_bytes = H * M * 4;
  L.delta = L.take(L.delta_bytes);
  L.ln_ws_bytes = vj_layernorm_bwd_ws_bytes(D);
  L.ln_ws = L.take(L.ln_ws_bytes);
  // option bias_fuse: the block's column partials stay alive until ONE reduction at the end of the block's backward --
  // a second LayerNorm partial buffer (norm2's), the fc2-dgrad epilogue's sums of du (fc1 bias) and the attention backward's
  // sums of dqkv (qkv bias; rows bounded by M/8 + 16: enough for sequences of >= 10 tokens, shorter ones take the unfused route)
  L.ln_ws2 = L.take(L.ln_ws_bytes);
  L.colp_fc1_rows = vj_gemm_colsum_rows(M);
  L.colp_fc1 = L.take(L.colp_fc1_rows * Dh * 4);
  L.colp_attn_rows = M / 8 + 16;
  L.colp_q = L.take(L.colp_attn_rows * D * 4);
  L.colp_kv = L.take(L.colp_attn_rows * 2 * D * 4);
  L.tcs_ws_bytes = vj_transpose_colsum_ws_bytes(M, nmax);
  if (vj_colsum_ws_bytes(nmax) > L.tcs_ws_bytes) L.tcs_ws_bytes = vj_colsum_ws_bytes(nmax);
  // scratch of the weight-gradient stream
  L.dyT = L.take(nmax * Mp * 2);
  L.xT = L.take(Dh * Mp * 2);
  L.tcs_ws = L.take(L.tcs_ws_bytes);
  L.wg_ws = L.take(GROUP_WS_BYTES);   // split-K partials of the single launches and of the grouped one
  return L;
}

extern "C" int64_t vj_blocks_bwd_ws_bytes(int64_t M, int64_t D, int64_t Dh, int64_t heads) {
  return bwd_layout(M, D, Dh, heads).total;
}

// ---------------------------------------------------------------------------------------------------- shared by both directions
static int check_shapes(const vj_block_t* blocks, int64_t n_blocks, int64_t D, int64_t heads, const vj_seg_t* segs, int64_t n_segs,
                        int64_t M, const char* who) {
  VJ_CHECK_ARG(blocks != nullptr && n_blocks > 0, "%s: no blocks", who);
  const int64_t Dh = blocks[0].fc1.n_out;
  for (int64_t i = 0; i < n_blocks; i++) {
    const vj_block_t& b = blocks[i];
    VJ_CHECK_ARG(b.qkv.n_out == 3 * D && b.qkv.k_in == D && b.proj.n_out == D && b.proj.k_in == D && b.fc1.n_out == Dh &&
                     b.fc1.k_in == D && b.fc2.n_out == D && b.fc2.k_in == Dh,
                 "%s: block %ld has inconsistent Linear shapes for D=%ld", who, (long)i, (long)D);
  }
  VJ_CHECK_ARG(segs != nullptr && n_segs > 0, "%s: no segments", who);
  int64_t r = 0;
  for (int64_t i = 0; i < n_segs; i++) {
    VJ_CHECK_ARG(segs[i].row0 == r && segs[i].B >= 0 && segs[i].S >= 0, "%s: segments must tile the rows in order", who);
    r += segs[i].B * segs[i].S;
  }
  VJ_CHECK_ARG(r == M, "%s: segments cover %ld rows, M=%ld", who, (long)r, (long)M);
  VJ_CHECK_ARG(heads > 0 && D % heads == 0, "%s: D=%ld not divisible by heads=%ld", who, (long)D, (long)heads);
  return 0;
}

// One profiled NT GEMM of the chains: C = epilogue(alpha * A B^T + bias, res | aux).  Kernel-selection flags per role: the
// run-time options gemm_fwd_flags / gemm_dgrad_flags (options.hpp), e.g. 256 = gemm4w.hip.  With ln_rowstats the LayerNorm
// of the rows of A is folded into the GEMM (vj_gemm_bf16_nt_lnfold: A holds the raw rows, B / bias the folded weights, no res / aux).
// The profiler's tag is the epilogue; epilogue 4 (the bf16 epilogue with alpha on the q columns) counts as 0.
static int gemm(const void* A, int64_t lda, const void* B, int64_t ldb, void* C, int64_t ldc, int64_t M, int64_t N,
                int64_t K, const float* bias, const void* res, int64_t ldr, const void* aux_in, void* aux_out,
                int64_t ldaux, int epi, hipStream_t st, int flags = 0, float alpha = 1.0f, const float* ln_rowstats = nullptr,
                const float* ln_colsum_w = nullptr) {
  ProfScope ps(st, 0, 2.0 * M * N * K, M, N, K, epi == 4 ? 0 : epi);
  if (ln_rowstats) return vj_gemm_bf16_nt_lnfold(A, lda, B, ldb, C, ldc, M, N, K, bias, ln_rowstats, ln_colsum_w, epi, alpha, flags, st);
  return vj_gemm_bf16_nt(A, lda, B, ldb, C, ldc, M, N, K, bias, res, ldr, aux_in, aux_out, ldaux, epi, alpha, 0.0f, flags, st);
}

// All masks of the batch in ONE attention launch, the short one's workgroups filling the long one's tail (profiles/r04_abab_attn_merge.md)
static inline bool merge_segs(int64_t n_segs) { return n_segs > 1 && n_segs <= 4; }

// The profiler's record of one attention launch over a segment list: m = segs[0].B, n = the longest S, k = heads, tag = head_dim;
// flop_per_qk: 4 forward (QK^T and PV), 8 backward
static ProfScope attn_prof(hipStream_t st, int family, double flop_per_qk, const vj_seg_t* segs, int64_t n_segs, int64_t heads,
                           int64_t hd) {
  double fl = 0;
  int64_t smax = 0;
  for (int64_t s = 0; s < n_segs; s++) {
    fl += flop_per_qk * segs[s].B * heads * segs[s].S * segs[s].S * hd;
    if (segs[s].S > smax) smax = segs[s].S;
  }
  return ProfScope(st, family, fl, segs[0].B, smax, heads, (int)hd);
}

// ---------------------------------------------------------------------------------------------------- forward
// Attention over the rows of qkv: one launch for all segments where they merge, else one per non-empty segment.  lse: nullable
static int attn_forward(const char* qkv, char* o, float* lse, const vj_seg_t* segs, int64_t n_segs, int64_t heads, int64_t hd,
                        float ascale, hipStream_t st) {
  const int64_t D = heads * hd;
  if (merge_segs(n_segs)) {
    ProfScope ps = attn_prof(st, 1, 4.0, segs, n_segs, heads, hd);
    return vj_attn_fwd_segs(qkv, o, lse, segs, n_segs, heads, hd, ascale, st);
  }
  for (int64_t s = 0; s < n_segs; s++) {
    const vj_seg_t& sg = segs[s];
    if (sg.B * sg.S == 0) continue;
    ProfScope ps = attn_prof(st, 1, 4.0, &sg, 1, heads, hd);
    CH(vj_attn_fwd(qkv + sg.row0 * 3 * D * 2, o + sg.row0 * D * 2, lse ? lse + heads * sg.row0 : nullptr, sg.B, sg.S, heads, hd,
                   ascale, st));
  }
  return 0;
}

// A Linear behind a LayerNorm reads the LayerNorm's output and its own weights, or (folded) the raw rows, their statistics and the folded weights
struct NormedLinearIn {
  const void *a, *w;
  const float *bias, *ln_rowstats, *ln_colsum_w;
};

static int blocks_fwd_impl(const vj_block_t* blocks, const vj_lnfold_t* folds, int64_t n_blocks, const void* x_in, void* x_out, int64_t M,
                           int64_t D, int64_t heads, const vj_seg_t* segs, int64_t n_segs, float ln_eps, int save,
                           int gemm_flags, void* ws, int64_t ws_bytes, hipStream_t stream) {
  // gemm_flags: the selection applies from block sel_from on -- the EMA target encoder's late blocks run after the context
  // branch has left the GPU, where the two-workgroups-per-CU kernel (0x100) is the faster one
  const int auto_flags = vj_opt(VJ_OPT_GEMM_FWD_FLAGS);
  const int sel_flags = (gemm_flags & VJ_GEMM_FLAGS_SEL_MASK) ? (gemm_flags & VJ_GEMM_FLAGS_SEL_MASK) : auto_flags;
  const int64_t sel_from = (gemm_flags >> VJ_GEMM_FLAGS_FROM_SHIFT) & VJ_GEMM_FLAGS_FROM_MASK;
  CH(check_shapes(blocks, n_blocks, D, heads, segs, n_segs, M, "vj_blocks_fwd"));
  if (M == 0) return 0;
  const int64_t Dh = blocks[0].fc1.n_out, hd = D / heads;
  const float scale = (float)pow((double)hd, -0.5);   // head_dim ** -0.5 exactly as Attention.scale (modules.py:53) is computed on the host
  const int64_t need = vj_blocks_fwd_ws_bytes(M, D, Dh, heads, n_blocks, save);
  VJ_CHECK_ARG(ws != nullptr && ws_bytes >= need, "vj_blocks_fwd: workspace too small (%ld < %ld)", (long)ws_bytes, (long)need);
  VJ_CHECK_ARG(((uintptr_t)ws & 255) == 0, "vj_blocks_fwd: workspace must be 256-byte aligned");
  const FwdLayout L = fwd_layout(M, D, Dh, heads);
  char* base = (char*)ws;
  if (L.n_gap) {   // option ws_guard
    CH(guard_begin(ws, need));
    for (int64_t li = 0; li < (save ? n_blocks : 1); li++) CH(poison_gaps(L, base + li * L.total, stream));
    if (!save) CH(poison_gap(base + L.total + al256(M * D * 2), stream));
  }
  // option attn_softmax = 2: the q third of qkv carries scale * log2(e), applied before the bf16 rounding (epilogue 4), and the
  // attention entry points are told "q is pre-scaled" by a negative scale
  const bool qpre = vj_opt(VJ_OPT_ATTN_SOFTMAX) == 2 && (3 * D) % 12 == 0;
  const int qkv_epi = qpre ? 4 : 0;
  const float qkv_alpha = qpre ? scale * 1.4426950408889634f : 1.0f, ascale = qpre ? -scale : scale;
  char* pingpong[2] = {base + L.x, base + L.total};   // save = 0: block outputs alternate between these two
  const char* x = (const char*)x_in;
  for (int64_t li = 0; li < n_blocks; li++) {
    const vj_block_t& b = blocks[li];
    const int fwd_flags = li >= sel_from ? sel_flags : auto_flags;
    char* w = save ? base + li * L.total : base;
    char* x2 = li == n_blocks - 1 ? (char*)x_out : save ? base + (li + 1) * L.total + L.x : pingpong[li & 1];
    auto kept = [&](int64_t off) { return save ? (float*)(w + off) : nullptr; };   // what only a backward reads
    // folded (these blocks never run backward): a statistics pass over the rows instead of the LayerNorm, the GEMM reads the rows themselves
    const vj_lnfold_t* fo = folds ? folds + li : nullptr;
    float* rs = (float*)(w + L.rs);
    // attention half: norm1, qkv, attention, proj + residual
    if (fo) CH(vj_ln_rowstats(x, rs, M, D, ln_eps, stream));
    else CH(vj_layernorm_fwd(x, b.norm1.g, b.norm1.b, w + L.y1, kept(L.mean1), kept(L.rstd1), M, D, ln_eps, stream));
    const NormedLinearIn q = fo ? NormedLinearIn{x, fo->w_qkv, fo->b_qkv, rs, fo->c_qkv}
                                : NormedLinearIn{w + L.y1, b.qkv.w, b.qkv.b, nullptr, nullptr};
    CH(gemm(q.a, D, q.w, D, w + L.qkv, 3 * D, M, 3 * D, D, q.bias, nullptr, 0, nullptr, nullptr, 0, qkv_epi, stream, fwd_flags,
            qkv_alpha, q.ln_rowstats, q.ln_colsum_w));
    CH(attn_forward(w + L.qkv, w + L.o, kept(L.lse), segs, n_segs, heads, hd, ascale, stream));
    CH(gemm(w + L.o, D, b.proj.w, D, w + L.x1, D, M, D, D, b.proj.b, x, D, nullptr, nullptr, 0, 0, stream, fwd_flags));
    // MLP half: norm2, fc1 + GELU (saving gelu'(pre-activation) for a backward), fc2 + residual
    if (fo) CH(vj_ln_rowstats(w + L.x1, rs, M, D, ln_eps, stream));
    else CH(vj_layernorm_fwd(w + L.x1, b.norm2.g, b.norm2.b, w + L.y2, kept(L.mean2), kept(L.rstd2), M, D, ln_eps, stream));
    const NormedLinearIn f = fo ? NormedLinearIn{w + L.x1, fo->w_fc1, fo->b_fc1, rs, fo->c_fc1}
                                : NormedLinearIn{w + L.y2, b.fc1.w, b.fc1.b, nullptr, nullptr};
    CH(gemm(f.a, D, f.w, D, w + L.g, Dh, M, Dh, D, f.bias, nullptr, 0, nullptr, save ? w + L.u : nullptr, Dh, 1, stream, fwd_flags,
            1.0f, f.ln_rowstats, f.ln_colsum_w));
    CH(gemm(w + L.g, Dh, b.fc2.w, Dh, x2, D, M, D, Dh, b.fc2.b, w + L.x1, D, nullptr, nullptr, 0, 0, stream, fwd_flags));
    x = x2;
  }
  return 0;
}

extern "C" int vj_blocks_fwd(const vj_block_t* blocks, int64_t n_blocks, const void* x_in, void* x_out, int64_t M,
                             int64_t D, int64_t heads, const vj_seg_t* segs, int64_t n_segs, float ln_eps, int save,
                             int gemm_flags, void* ws, int64_t ws_bytes, hipStream_t stream) {
  return blocks_fwd_impl(blocks, nullptr, n_blocks, x_in, x_out, M, D, heads, segs, n_segs, ln_eps, save, gemm_flags, ws, ws_bytes, stream);
}

// The same trunk with both LayerNorms of every block folded into the Linear that consumes them (vj_gemm_bf16_nt_lnfold): for
// blocks that never run backward (save must be 0) -- the EMA target encoder, frozen-encoder inference.  folds[i] holds block
// i's folded qkv / fc1 weights (vj_ln_fold_weights); the blocks' own norm / qkv / fc1 weights are not read.  Workspace as
// vj_blocks_fwd_ws_bytes(..., save = 0).
extern "C" int vj_blocks_fwd_lnfold(const vj_block_t* blocks, const vj_lnfold_t* folds, int64_t n_blocks, const void* x_in, void* x_out,
                                    int64_t M, int64_t D, int64_t heads, const vj_seg_t* segs, int64_t n_segs, float ln_eps,
                                    int gemm_flags, void* ws, int64_t ws_bytes, hipStream_t stream) {
  VJ_CHECK_ARG(folds != nullptr, "vj_blocks_fwd_lnfold: no folded weights");
  for (int64_t i = 0; i < n_blocks; i++)
    VJ_CHECK_ARG(folds[i].w_qkv && folds[i].c_qkv && folds[i].b_qkv && folds[i].w_fc1 && folds[i].c_fc1 && folds[i].b_fc1,
                 "vj_blocks_fwd_lnfold: block %ld lacks folded weights", (long)i);
  return blocks_fwd_impl(blocks, folds, n_blocks, x_in, x_out, M, D, heads, segs, n_segs, ln_eps, 0, gemm_flags, ws, ws_bytes, stream);
}

// ---------------------------------------------------------------------------------------------------- backward
// The stages carry the names of their per-kernel mirrors in engine/layers.py (block_backward, _linear_backward, _wgrad,
// _wgrad_group): same kernels, same order.
struct BwdCtx {   // what one vj_blocks_bwd call fixes for all of its blocks
  const vj_block_t* blocks;
  int64_t n_blocks;
  hipStream_t main, side;   // dgrad chain / weight gradients; side == main: serial mode
  const char* sv;           // saved activations: one FwdLayout F per block
  char* tmp;                // temporaries: BwdLayout L
  FwdLayout F;
  BwdLayout L;
  int64_t M, D, Dh, heads, hd;
  const vj_seg_t* segs;
  int64_t n_segs;
  float alpha, beta, ascale;
  int dgrad_flags;
  bool tn;        // transpose-free weight gradients; the LayerNorm backwards then also produce the bias gradients of proj and of the
                  // previous block's fc2 (the NT route folds the bias gradient into its dY transpose instead)
  bool grouped;   // option wgrad_group: the block's four weight gradients in one launch
  bool bfuse;     // option bias_fuse (with tn): every column partial the block produces -- both LayerNorm backwards', the fc2-dgrad epilogue's
                  // sums of du (fc1's bias gradient), the attention backward's sums of dqkv (qkv's) -- is reduced by ONE vj_reduce_segments launch
                  // at the end of the block, not by 6 launches that re-read du / dqkv (143 MB per ViT-L context block)
  bool last_fc2_bias_done;   // the caller's final-norm backward already wrote the LAST block's fc2 bias gradient, the column sums of dout
};

struct WgradItem {   // one Linear's weight-gradient problem: dW = dy^T x
  const void *dy, *x;
  const vj_linear_t* lw;
  bool bias_done;   // the bias gradient (column sums of dy) comes out of the kernel that produced dy
};

struct ReduceList {   // the block's list for its one vj_reduce_segments launch (option bias_fuse)
  vj_reduce_seg_t seg[12];
  int n = 0;
  void add(const float* part, float* out, int64_t rows, int64_t cols, int64_t stride) { seg[n++] = vj_reduce_seg_t{part, out, rows, cols, stride}; }
};

// dW (fp32, += beta*old) = alpha * dy^T x ; db = alpha * colsum(dy) -- on the side stream, after `main` produced dy
static int wgrad(const BwdCtx& c, const WgradItem& it) {
  const vj_linear_t& lw = *it.lw;
  float* gb = it.bias_done ? nullptr : lw.gb;
  const BwdLayout& L = c.L;
  const int64_t M = c.M, Mp = pad64i(M), N = lw.n_out, K = lw.k_in;
  hipStream_t st = c.side;
  if (st != c.main) CH(stream_after(st, c.main, "vj_blocks_bwd(fork)"));
  if (c.tn && N % 8 == 0 && K % 8 == 0) {
    if (gb) CH(vj_colsum_bf16(it.dy, M, N, N, M > 0 ? M : 1, 0, M > 0 ? M : 1, gb, c.alpha, c.beta, c.tmp + L.tcs_ws, L.tcs_ws_bytes, st));
    ProfScope ps(st, 0, 2.0 * M * N * K, N, K, M, 3);
    return vj_gemm_bf16_tn_splitk(it.dy, N, it.x, K, lw.gw, K, M, N, K, c.alpha, c.beta, c.tmp + L.wg_ws, WGRAD_WS_BYTES, st);
  }
  char *dyT = c.tmp + L.dyT, *xT = c.tmp + L.xT;
  if (gb) CH(vj_transpose_colsum_bf16(it.dy, dyT, M, N, N, Mp, gb, c.alpha, c.beta, c.tmp + L.tcs_ws, L.tcs_ws_bytes, st));
  else CH(vj_transpose_bf16(it.dy, dyT, M, N, N, Mp, st));
  CH(vj_transpose_bf16(it.x, xT, M, K, K, Mp, st));
  ProfScope ps(st, 0, 2.0 * N * K * Mp, N, K, Mp, 3);
  return vj_gemm_bf16_nt_splitk(dyT, Mp, xT, Mp, lw.gw, K, N, K, Mp, c.alpha, c.beta, 0, c.tmp + L.wg_ws, WGRAD_WS_BYTES, st);
}

// The block's four weight gradients as ONE grouped launch (option wgrad_group): the bias column sums that no other kernel
// produced go first, then vj_gemm_bf16_tn_grouped; everything on the side stream, after `main` produced the last dY of the block.
static int wgrad_group(const BwdCtx& c, const WgradItem* it, int n) {
  hipStream_t st = c.side;
  if (st != c.main) CH(stream_after(st, c.main, "vj_blocks_bwd(fork)"));
  vj_tn_problem_t pr[4];
  double fl = 0;
  int64_t out_elems = 0;
  for (int i = 0; i < n; i++) {
    const vj_linear_t& lw = *it[i].lw;
    const int64_t N = lw.n_out, K = lw.k_in, M = c.M;
    if (lw.gb && !it[i].bias_done)
      CH(vj_colsum_bf16(it[i].dy, M, N, N, M > 0 ? M : 1, 0, M > 0 ? M : 1, lw.gb, c.alpha, c.beta, c.tmp + c.L.tcs_ws, c.L.tcs_ws_bytes, st));
    pr[i] = vj_tn_problem_t{it[i].dy, N, it[i].x, K, lw.gw, K, N, K};
    fl += 2.0 * M * N * K;
    out_elems += N * K;
  }
  ProfScope ps(st, 0, fl, out_elems / pr[0].N2, pr[0].N2, c.M, 4);
  return vj_gemm_bf16_tn_grouped(pr, n, c.M, c.alpha, c.beta, c.tmp + c.L.wg_ws, GROUP_WS_BYTES, st);
}

// One Linear's backward: its weight gradient (left to the block's grouped launch where that is on), then dx = dy W on `main`,
// through GELU' where the Linear's input was a GELU output (dgelu_aux: the saved derivative)
static int linear_backward(const BwdCtx& c, const WgradItem& it, void* dx, const void* dgelu_aux = nullptr) {
  const vj_linear_t& lw = *it.lw;
  if (!c.grouped) CH(wgrad(c, it));
  return gemm(it.dy, lw.n_out, lw.wT, lw.ldwT, dx, lw.k_in, c.M, lw.k_in, lw.n_out, nullptr, nullptr, 0, dgelu_aux, nullptr,
              dgelu_aux ? lw.k_in : 0, dgelu_aux ? 2 : 0, c.main, c.dgrad_flags);
}

// MLP half, items = {fc2, fc1}: du = (dx2 W_fc2) * gelu'(u), dy2 = du W_fc1.  With option bias_fuse the fc2 dgrad's epilogue also writes
// column partials of du (= fc1's bias gradient) for the block's reduction -- if the GEMM takes a kernel that has that epilogue;
// otherwise fc1's bias gradient keeps the stand-alone route.
static int mlp_backward(const BwdCtx& c, WgradItem* items, const void* dgelu_aux, void* du, void* dy2, ReduceList& rl) {
  const vj_linear_t &fc2 = *items[0].lw, &fc1 = *items[1].lw;
  const int64_t M = c.M, D = c.D, Dh = c.Dh;
  if (c.bfuse && fc1.gb != nullptr) {
    if (!c.grouped) CH(wgrad(c, items[0]));
    float* colp = (float*)(c.tmp + c.L.colp_fc1);
    int fused = 0;
    ProfScope ps(c.main, 0, 2.0 * M * Dh * D, M, Dh, D, 2);
    CH(vj_gemm_bf16_nt_dgelu_colsum(items[0].dy, D, fc2.wT, fc2.ldwT, du, Dh, M, Dh, D, dgelu_aux, Dh, colp, c.L.colp_fc1_rows,
                                    c.dgrad_flags, &fused, c.main));
    if (fused) rl.add(colp, fc1.gb, c.L.colp_fc1_rows, Dh, Dh);
    items[1].bias_done = fused != 0;
  } else {
    CH(linear_backward(c, items[0], du, dgelu_aux));
  }
  return linear_backward(c, items[1], dy2);
}

// LayerNorm backward: dx = LayerNorm'(dy) + dres, dgamma, dbeta and (dxsum non-null, transpose-free route) the column sums of dx: the
// bias gradient of the Linear whose dY dx is.  bias_fuse: the column partials stay in `ws` and join the block's reduction list;
// otherwise they are reduced here.
static int ln_backward(const BwdCtx& c, const void* dy, const void* x, const vj_norm_t& nm, const char* mean, const char* rstd,
                       const void* dres, void* dx, float* dxsum, char* ws, ReduceList& rl) {
  if (!c.bfuse)
    return vj_layernorm_bwd_colsum(dy, x, nm.g, (const float*)mean, (const float*)rstd, dres, dx, nm.gg, nm.gb, c.tn ? dxsum : nullptr,
                                   c.alpha, c.beta, c.M, c.D, ws, c.L.ln_ws_bytes, c.main);
  int64_t nb = 0;
  const bool cs = dxsum != nullptr;
  CH(vj_layernorm_bwd_partials(dy, x, nm.g, (const float*)mean, (const float*)rstd, dres, dx, cs, c.M, c.D, ws, c.L.ln_ws_bytes, &nb,
                               c.main));
  const int64_t D = c.D, stride = (cs ? 3 : 2) * D;
  const float* p = (const float*)ws;
  rl.add(p, nm.gg, nb, D, stride);
  rl.add(p + D, nm.gb, nb, D, stride);
  if (cs) rl.add(p + 2 * D, dxsum, nb, D, stride);
  return 0;
}

// Attention backward: dqkv from (qkv, o, lse, dO): one dQ + one dK/dV launch for all segments where they merge, else per non-empty
// segment (vj_attn_bwd / vj_attn_bwd_colsum are this call on the one segment {0, B, S} at the segment's rows).  qkv_gb non-null
// (option bias_fuse): the kernels also write column partials of dqkv (qkv's bias gradient), segment after segment, for the block's
// reduction -- unless the segments' partial rows exceed the workspace's budget: the bias gradient then takes the stand-alone route.
// *fused tells which.
static int attn_backward(const BwdCtx& c, const char* qkv, const char* o, const char* dob, const float* lse, char* dqkv, float* qkv_gb,
                         ReduceList& rl, bool* fused) {
  const BwdLayout& L = c.L;
  const int64_t D = c.D, heads = c.heads, hd = c.hd;
  int64_t rows_q = 0, rows_kv = 0;
  bool cs = qkv_gb != nullptr;
  for (int64_t s = 0; s < c.n_segs && cs; s++) {
    int64_t rq = 0, rkv = 0;
    if (c.segs[s].B * c.segs[s].S != 0) CH(vj_attn_bwd_colsum_rows(c.segs[s].B, c.segs[s].S, hd, &rq, &rkv));
    rows_q += rq;
    rows_kv += rkv;
  }
  if (rows_q > L.colp_attn_rows || rows_kv > L.colp_attn_rows) cs = false;
  float* const colp_q = cs ? (float*)(c.tmp + L.colp_q) : nullptr;
  float* const colp_kv = cs ? (float*)(c.tmp + L.colp_kv) : nullptr;
  if (merge_segs(c.n_segs)) {
    ProfScope ps = attn_prof(c.main, 2, 8.0, c.segs, c.n_segs, heads, hd);
    CH(vj_attn_bwd_segs(qkv, o, dob, lse, dqkv, c.segs, c.n_segs, heads, hd, c.ascale, c.tmp + L.delta, L.delta_bytes, colp_q, colp_kv,
                        c.main));
  } else {
    float *cq = colp_q, *ckv = colp_kv;
    for (int64_t s = 0; s < c.n_segs; s++) {
      const vj_seg_t one = {0, c.segs[s].B, c.segs[s].S};
      if (one.B * one.S == 0) continue;
      const int64_t r0 = c.segs[s].row0, r3 = r0 * 3 * D * 2, r1 = r0 * D * 2;
      ProfScope ps = attn_prof(c.main, 2, 8.0, &one, 1, heads, hd);
      CH(vj_attn_bwd_segs(qkv + r3, o + r1, dob + r1, lse + heads * r0, dqkv + r3, &one, 1, heads, hd, c.ascale, c.tmp + L.delta,
                          L.delta_bytes, cq, ckv, c.main));
      if (cs) {
        int64_t rq = 0, rkv = 0;
        CH(vj_attn_bwd_colsum_rows(one.B, one.S, hd, &rq, &rkv));
        cq += rq * D;
        ckv += rkv * 2 * D;
      }
    }
  }
  if (cs) {
    rl.add(colp_q, qkv_gb, rows_q, D, D);
    rl.add(colp_kv, qkv_gb + D, rows_kv, 2 * D, 2 * D);
  }
  *fused = cs;
  return 0;
}

// Backward of block li: dx = d loss / d (block input) from dx2 = d loss / d (block output); x = the block's input
static int block_backward(const BwdCtx& c, int64_t li, const char* x, const char* dx2, char* dx) {
  const vj_block_t& b = c.blocks[li];
  const FwdLayout& F = c.F;
  const BwdLayout& L = c.L;
  const char* w = c.sv + li * F.total;
  char* tmp = c.tmp;
  const int p = (int)(li & 1);   // du / dx1 / dqkv alternate between two buffers: block li+1's weight gradients may still read theirs
  char* du = tmp + L.du[p];
  char* dx1 = tmp + L.dx1[p];
  char* dqkv = tmp + L.dqkv[p];
  // dx2 of every block but the last is the dx of block li+1's norm1 backward, which also produced its column sums; dx1 is the dY of proj:
  // its column sums come out of the norm2 backward
  const bool fc2_done = c.tn && (li + 1 < c.n_blocks || c.last_fc2_bias_done);
  WgradItem items[4] = {{dx2, w + F.g, &b.fc2, fc2_done}, {du, w + F.y2, &b.fc1, false},   // (fc1 / qkv: set by the stage that
                        {dx1, w + F.o, &b.proj, c.tn}, {dqkv, w + F.y1, &b.qkv, false}};    //  may produce the column sums of du / dqkv)
  ReduceList rl;
  CH(mlp_backward(c, items, w + F.u, du, tmp + L.dy2, rl));
  CH(ln_backward(c, tmp + L.dy2, w + F.x1, b.norm2, w + F.mean2, w + F.rstd2, dx2, dx1, b.proj.gb, tmp + (c.bfuse ? L.ln_ws2 : L.ln_ws), rl));
  CH(linear_backward(c, items[2], tmp + L.dob));
  CH(attn_backward(c, w + F.qkv, w + F.o, tmp + L.dob, (const float*)(w + F.lse), dqkv, c.bfuse ? b.qkv.gb : nullptr, rl, &items[3].bias_done));
  if (c.grouped) CH(wgrad_group(c, items, 4));
  CH(linear_backward(c, items[3], tmp + L.dy1));
  // dx is the dY of the previous block's fc2 (its dx2): that bias gradient comes out of this pass
  CH(ln_backward(c, tmp + L.dy1, x, b.norm1, w + F.mean1, w + F.rstd1, dx1, dx, li > 0 ? c.blocks[li - 1].fc2.gb : nullptr, tmp + L.ln_ws, rl));
  if (c.bfuse) CH(vj_reduce_segments(rl.seg, rl.n, c.alpha, c.beta, c.main));   // the block's ONE reduction launch
  return 0;
}

extern "C" int vj_blocks_bwd(const vj_block_t* blocks, int64_t n_blocks, const void* x_in, const void* dout, void* dx_out,
                             int64_t M, int64_t D, int64_t heads, const vj_seg_t* segs, int64_t n_segs, float alpha,
                             float beta_acc, const void* save_ws, int64_t save_ws_bytes, void* tmp_ws,
                             int64_t tmp_ws_bytes, int flags, hipStream_t stream, hipStream_t side,
                             vj_layer_cb_t on_layer_done, void* user) {
  CH(check_shapes(blocks, n_blocks, D, heads, segs, n_segs, M, "vj_blocks_bwd"));
  if (M == 0) return 0;
  const int64_t Dh = blocks[0].fc1.n_out, hd = D / heads;
  const float scale = (float)pow((double)hd, -0.5);   // head_dim ** -0.5 exactly as Attention.scale (modules.py:53) is computed on the host
  BwdCtx c{blocks, n_blocks, stream, side ? side : stream, (const char*)save_ws, (char*)tmp_ws, fwd_layout(M, D, Dh, heads),
           bwd_layout(M, D, Dh, heads), M, D, Dh, heads, hd, segs, n_segs, alpha, beta_acc};
  const FwdLayout& F = c.F;
  const BwdLayout& L = c.L;
  VJ_CHECK_ARG(save_ws != nullptr && save_ws_bytes >= F.total * n_blocks, "vj_blocks_bwd: saved-activation workspace too small");
  VJ_CHECK_ARG(tmp_ws != nullptr && tmp_ws_bytes >= L.total, "vj_blocks_bwd: temporary workspace too small (%ld < %ld)",
               (long)tmp_ws_bytes, (long)L.total);
  VJ_CHECK_ARG((((uintptr_t)save_ws | (uintptr_t)tmp_ws) & 255) == 0, "vj_blocks_bwd: workspaces must be 256-byte aligned");
  for (int64_t i = 0; i < n_blocks; i++) {
    const vj_block_t& b = blocks[i];
    VJ_CHECK_ARG(b.qkv.wT && b.proj.wT && b.fc1.wT && b.fc2.wT && b.qkv.gw && b.proj.gw && b.fc1.gw && b.fc2.gw &&
                     b.norm1.gg && b.norm1.gb && b.norm2.gg && b.norm2.gb,
                 "vj_blocks_bwd: block %ld lacks transposed weights / gradient views", (long)i);
  }
  constexpr int MAX_BLOCKS = 256;
  VJ_CHECK_ARG(n_blocks <= MAX_BLOCKS, "vj_blocks_bwd: more than %d blocks", MAX_BLOCKS);
  if (L.n_gap) CH(guard_begin(c.tmp, L.total));   // option ws_guard
  CH(poison_gaps(L, c.tmp, stream));
  // the options, read once: they change only between steps
  c.dgrad_flags = vj_opt(VJ_OPT_GEMM_DGRAD_FLAGS);
  c.tn = (flags & VJ_BWD_FORCE_TN) || vj_opt(VJ_OPT_WGRAD_TN);
  c.grouped = c.tn && vj_opt(VJ_OPT_WGRAD_GROUP) != 0 && D % 8 == 0 && Dh % 8 == 0;
  c.bfuse = c.tn && vj_opt(VJ_OPT_BIAS_FUSE) != 0;
  c.last_fc2_bias_done = (flags & VJ_BWD_LAST_FC2_BIAS_DONE) != 0;
  // as the FORWARD stored q: the caller recorded the mode its vj_blocks_fwd call used (VJ_BWD_Q_PRESCALED_VALID); otherwise the
  // option is read again, which is only right if it did not change since that forward
  const bool qpre = (flags & VJ_BWD_Q_PRESCALED_VALID) ? (flags & VJ_BWD_Q_PRESCALED) != 0
                                                       : (vj_opt(VJ_OPT_ATTN_SOFTMAX) == 2 && (3 * D) % 12 == 0);
  c.ascale = qpre ? -scale : scale;
  const bool two_streams = c.side != c.main;
  hipEvent_t side_done[MAX_BLOCKS];   // block li's weight gradients have been enqueued on the side stream
  const char* dx2 = (const char*)dout;
  for (int64_t li = n_blocks - 1; li >= 0; li--) {
    // the buffers this block is about to overwrite were last read by the weight gradients of block li+2
    if (two_streams && li + 2 < n_blocks) HIPCH(hipStreamWaitEvent(stream, side_done[li + 2], 0), "vj_blocks_bwd");
    char* dx = li == 0 ? (char*)dx_out : c.tmp + L.dx[li % 3];
    CH(block_backward(c, li, li == 0 ? (const char*)x_in : c.sv + li * F.total + F.x, dx2, dx));
    if (two_streams) {
      side_done[li] = next_event();
      HIPCH(hipEventRecord(side_done[li], c.side), "vj_blocks_bwd");
    }
    if (on_layer_done) on_layer_done(user, (int)li);
    dx2 = dx;
  }
  return 0;
}
