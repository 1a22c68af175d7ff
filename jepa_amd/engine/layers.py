"""Hand-written forward / backward chains of the V-JEPA encoder and predictor over the C-ABI kernels.

No autograd graph: every chain saves exactly the activations its backward needs and the backward walks the layers
in reverse, writing weight gradients (fp32) straight into the gradient-arena views.  Both masks of a step run
through ONE chain: their token rows are concatenated along M (bigger GEMMs, each weight gradient produced in one
piece -- which is also what makes a layer's gradient bucket final as soon as that layer's backward is done), and
only attention, which is per-sequence, is launched per mask segment.

Reference semantics restated (never copied):
  Block / Attention / MLP        src/models/utils/modules.py:13-120
  VisionTransformer.forward      src/models/vision_transformer.py:159-195
  VisionTransformerPredictor     src/models/predictor.py:174-239
  MultiMask wrappers             src/models/utils/multimask.py:11-48
"""
import os
from dataclasses import dataclass
from typing import List, Optional

import numpy as np
import torch

from ..hip import ops, ops_still
from ..hip.lib import get_option
from . import chain
from .streams import (SideStream, _INDEP_LOG, independent_stream, low_priority_stream, side_stream,  # noqa: F401  (re-exported)
                      streams_concurrent)
from .weights import BlockW, EncoderW, LinearW, PredictorW

LN_EPS = 1e-6  # partial(nn.LayerNorm, eps=1e-6), vision_transformer.py:252-281 / predictor.py:242-246
LOG2E = 1.4426950408889634

# The C launch chains (vj_blocks_fwd / vj_blocks_bwd) are the default for the Trainer; VJ_PY_CHAIN=1 keeps the
# per-kernel Python chain below (same kernels, same order: bit-identical results, ~10x the host time).
USE_C_CHAIN = os.environ.get("VJ_PY_CHAIN", "0") != "1"


@dataclass
class Seg:
    """A group of B equal-length sequences occupying rows [row0, row0 + B*S) of the token matrix."""
    row0: int
    B: int
    S: int

    @property
    def rows(self):
        return self.B * self.S

    @classmethod
    def table(cls, B, lengths):
        """One segment of B sequences per length, each starting at the row where the one before it ends."""
        segs, r = [], 0
        for S in lengths:
            segs.append(cls(r, B, S))
            r += B * S
        return segs


def _rows(t, seg):
    return t[seg.row0:seg.row0 + seg.rows]


def _total_rows(segs):
    return segs[-1].row0 + segs[-1].rows if segs else 0


def _q_prescaled(D: int) -> bool:
    return get_option("attn_softmax") == 2 and D % 4 == 0


def _f32_mul(a: float, b: float) -> float:
    """a * b rounded as the C chain rounds it (float * float)."""
    return float(np.float32(np.float32(a) * np.float32(b)))


# =============================================================================================== block
def _drop_residual(x, y, s, segs):
    """y <- x + s[b] * y in place (stochastic depth: s fp32 [B], 0 or 1 / keep per sample; vj_drop_path_add).  A clip keeps its
    scale in every segment: s is indexed by b within each Seg."""
    for sg in segs:
        ops.drop_path_add(_rows(x, sg), _rows(y, sg), s, sg.B, sg.S)
    return y


def _drop_grad(dx, s, segs):
    """bf16(s[b] * dx): the gradient of a dropped branch's output, the dY of its last Linear (vj_drop_path_scale)."""
    out = torch.empty_like(dx)
    for sg in segs:
        ops.drop_path_scale(_rows(dx, sg), s, sg.B, sg.S, out=_rows(out, sg))
    return out


def block_forward(x, bw: BlockW, segs: List[Seg], heads: int, save: bool, fold=None, drop=None):
    """x [M, D] bf16 -> x2 [M, D]; returns (x2, saved).  fold (FoldW, only with save = False): both LayerNorms folded into the
    GEMMs that consume them -- the kernels and their order are those of vj_blocks_fwd_lnfold (bit-identical results).
    drop (stochastic depth): None, or (s_attn, s_mlp), each None or an fp32 [B] tensor of per-sample scales.  A branch with a scale
    leaves its last GEMM without the fused residual (the branch is rounded to bf16 once) and _drop_residual finishes it in place
    (the sum is rounded once); a branch without one issues exactly the launches of drop = None."""
    s_attn, s_mlp = drop if drop is not None else (None, None)
    D = x.shape[1]
    hd = D // heads
    scale = hd ** -0.5
    if fold is not None and save:
        raise ValueError("block_forward: folded LayerNorms keep nothing for a backward")
    epi, q_alpha = ops.EPI_BF16, 1.0
    if _q_prescaled(D):   # option attn_softmax = 2 (as vj_blocks_fwd): the q third of qkv carries scale * log2(e)
        epi, q_alpha = ops.EPI_QKV, _f32_mul(scale, LOG2E)
        scale = -scale    # "q is pre-scaled" for the attention entry points
    y1 = mean1 = rstd1 = None
    if fold is not None:
        qkv = ops.gemm_nt_lnfold(x, fold.w_qkv, fold.b_qkv, ops.ln_rowstats(x, LN_EPS), fold.c_qkv, epilogue=epi, alpha=q_alpha)
    else:
        y1, mean1, rstd1 = ops.layernorm_fwd(x, bw.norm1.g, bw.norm1.b, LN_EPS, save_stats=save)
        qkv = ops.gemm_nt(y1, bw.qkv.w, bias=bw.qkv.b, epilogue=epi, alpha=q_alpha)
    o = torch.empty_like(x)
    lses = []
    for sg in segs:
        _, lse = ops.attn_fwd(_rows(qkv, sg), sg.B, sg.S, heads, hd, scale, save_lse=save, out=_rows(o, sg))
        lses.append(lse)
    if s_attn is None:
        x1 = ops.gemm_nt(o, bw.proj.w, bias=bw.proj.b, residual=x)
    else:
        x1 = _drop_residual(x, ops.gemm_nt(o, bw.proj.w, bias=bw.proj.b), s_attn, segs)
    y2 = mean2 = rstd2 = u = None
    if fold is not None:
        g = ops.gemm_nt_lnfold(x1, fold.w_fc1, fold.b_fc1, ops.ln_rowstats(x1, LN_EPS), fold.c_fc1, epilogue=ops.EPI_GELU)
    else:
        y2, mean2, rstd2 = ops.layernorm_fwd(x1, bw.norm2.g, bw.norm2.b, LN_EPS, save_stats=save)
        # u: the fc1 epilogue saves gelu'(pre-activation) here (not the pre-activation): all the backward needs from it
        u = torch.empty((x.shape[0], bw.fc1.w.shape[0]), dtype=torch.bfloat16, device=x.device) if save else None
        g = ops.gemm_nt(y2, bw.fc1.w, bias=bw.fc1.b, aux_out=u, epilogue=ops.EPI_GELU)
    if s_mlp is None:
        x2 = ops.gemm_nt(g, bw.fc2.w, bias=bw.fc2.b, residual=x1)
    else:
        x2 = _drop_residual(x1, ops.gemm_nt(g, bw.fc2.w, bias=bw.fc2.b), s_mlp, segs)
    saved = (x, y1, mean1, rstd1, qkv, o, lses, x1, y2, mean2, rstd2, u, g) if save else None
    return x2, saved


# Weight gradients: transpose-free by default (vj_gemm_bf16_tn_splitk reads dY and X token-major as the backward produced
# them; round-3 interleaved A/B at ViT-L B=24: 86.38 vs 86.83 ms/step, faster in 8 of 8 rounds, -25 W, and the 294
# transpose launches / 35 GB per step of the NT route are gone -- profiles/r03_abab_switches.md).  The run-time option
# "wgrad_tn" = 0 (VJ_WGRAD_TN=0) selects the transposes + NT split-K route, kept as the cross-check of the TN kernel.
def _tn_ok(n_out: int, k_in: int) -> bool:
    return get_option("wgrad_tn") != 0 and n_out % 8 == 0 and k_in % 8 == 0   # as chain.hip: any non-zero value is "on"


def _wgrad(dy, x_in, lw: LinearW, alpha: float, beta: float = 0.0, bias_done: bool = False):
    """bias_done: the bias gradient (column sums of dy) was produced by the LayerNorm backward that produced dy."""
    acc = beta != 0.0
    if _tn_ok(dy.shape[1], x_in.shape[1]):
        if lw.gb is not None and not bias_done:
            ops.colsum(dy, lw.gb, alpha=alpha, accumulate=acc)
        ops.gemm_wgrad_tn(dy, x_in, lw.gw, alpha=alpha, beta=beta)
        return
    # (bias_done: the LayerNorm backward already wrote lw.gb -- no second column sum, exactly as chain.hip wgrad() nulls gb)
    need_cs = lw.gb is not None and not bias_done
    dyT = ops.transpose_colsum(dy, lw.gb, alpha=alpha, accumulate=acc) if need_cs else ops.transpose(dy)
    xT = ops.transpose(x_in)
    ops.gemm_wgrad(dyT, xT, lw.gw, alpha=alpha, beta=beta)


def _group_ok(bw) -> bool:
    """Option wgrad_group: the four weight gradients of a block as one vj_gemm_bf16_tn_grouped launch (as vj_blocks_bwd)."""
    return (get_option("wgrad_tn") != 0 and get_option("wgrad_group") != 0 and
            all(d % 8 == 0 for lw in (bw.qkv, bw.proj, bw.fc1, bw.fc2) for d in lw.gw.shape))


def _on_side(fn, *tensors):
    """fn() on the side stream, behind everything enqueued so far on this one (tensors: what it reads there); inline when the
    side stream is disabled.  The caller joins before the results are consumed."""
    side = side_stream(tensors[0].device)
    if side.enabled:
        side.fork(*tensors)
        with torch.cuda.stream(side.stream):
            fn()
    else:
        fn()


def _wgrad_group(items, alpha: float, beta: float):
    """items: [(dy, x_in, lw, bias_done)] in the order fc2, fc1, proj, qkv: bias column sums first, then one launch."""
    def run():
        for dy, x_in, lw, bias_done in items:
            if lw.gb is not None and not bias_done:
                ops.colsum(dy, lw.gb, alpha=alpha, accumulate=beta != 0.0)
        ops.gemm_wgrad_tn_grouped([(dy, x_in, lw.gw) for dy, x_in, lw, _ in items], alpha=alpha, beta=beta)
    _on_side(run, *[t for dy, x_in, _, _ in items for t in (dy, x_in)])


def _linear_backward(dy, x_in, lw: LinearW, alpha: float, need_dx=True, dgelu_aux=None, beta: float = 0.0,
                     bias_done: bool = False, defer=None):
    """dW (fp32, into lw.gw) = alpha * dy^T x_in + beta * dW ; db likewise ; returns dx = dy W (bf16).
    The weight-gradient half goes to the side stream; the caller joins before the gradients are consumed.
    defer (list): only record the weight-gradient problem; the caller launches the block's group (_wgrad_group)."""
    if defer is not None:
        defer.append((dy, x_in, lw, bias_done))
    else:
        _on_side(lambda: _wgrad(dy, x_in, lw, alpha, beta, bias_done), dy, x_in)
    if not need_dx:
        return None
    if dgelu_aux is not None:
        return ops.gemm_nt(dy, lw.wT, aux_in=dgelu_aux, epilogue=ops.EPI_DGELU)
    return ops.gemm_nt(dy, lw.wT)


def block_backward(dx2, saved, bw: BlockW, segs: List[Seg], heads: int, alpha: float, beta: float = 0.0,
                   fc2_bias_done: bool = False, prev_fc2_gb=None, drop=None):
    """With transpose-free weight gradients the bias gradients of proj and of the PREVIOUS block's fc2 are the column
    sums of the two LayerNorm backward outputs and come out of those passes (vj_layernorm_bwd_colsum); `fc2_bias_done`
    says that this block's fc2 bias gradient was produced that way by the block above.  Same kernels, same order as
    vj_blocks_bwd (csrc/chain.hip): bit-identical results.
    drop = (s_attn, s_mlp) of the forward.  The dY of a scaled branch's last Linear is the scaled copy of the stream's gradient
    (_drop_grad), which feeds its dgrad, weight and bias gradient, while the LayerNorm backward below still adds the unscaled
    gradient as dres.  That Linear's bias gradient is then NOT the column sum of a LayerNorm backward's output: a scaled MLP branch
    ignores fc2_bias_done (and the caller passes prev_fc2_gb = None to the block above it), a scaled attention branch takes
    proj.gb from ops.colsum."""
    s_attn, s_mlp = drop if drop is not None else (None, None)
    x, y1, mean1, rstd1, qkv, o, lses, x1, y2, mean2, rstd2, u, g = saved
    D = x.shape[1]
    hd = D // heads
    scale = hd ** -0.5
    if _q_prescaled(D):
        scale = -scale       # the forward stored q pre-scaled (option attn_softmax = 2)
    acc = beta != 0.0
    fuse = _tn_ok(8, 8)
    defer = [] if _group_ok(bw) else None
    dfc2 = dx2 if s_mlp is None else _drop_grad(dx2, s_mlp, segs)
    du = _linear_backward(dfc2, g, bw.fc2, alpha, dgelu_aux=u, beta=beta, bias_done=fuse and fc2_bias_done and s_mlp is None,
                          defer=defer)   # fc2 dgrad fused with GELU'
    dy2 = _linear_backward(du, y2, bw.fc1, alpha, beta=beta, defer=defer)
    dx1 = ops.layernorm_bwd(dy2, x1, bw.norm2.g, mean2, rstd2, bw.norm2.gg, bw.norm2.gb, dres=dx2, alpha=alpha,
                            accumulate=acc, dxsum=bw.proj.gb if fuse and s_attn is None else None)
    dproj = dx1 if s_attn is None else _drop_grad(dx1, s_attn, segs)
    do = _linear_backward(dproj, o, bw.proj, alpha, beta=beta, bias_done=fuse and s_attn is None, defer=defer)
    dqkv = torch.empty_like(qkv)
    for sg, lse in zip(segs, lses):
        ops.attn_bwd(_rows(qkv, sg), _rows(o, sg), _rows(do, sg), lse, sg.B, sg.S, heads, hd, scale,
                     out=_rows(dqkv, sg))
    if defer is not None:
        defer.append((dqkv, y1, bw.qkv, False))
        _wgrad_group(defer, alpha, beta)
        dy1 = ops.gemm_nt(dqkv, bw.qkv.wT)
    else:
        dy1 = _linear_backward(dqkv, y1, bw.qkv, alpha, beta=beta)
    return ops.layernorm_bwd(dy1, x, bw.norm1.g, mean1, rstd1, bw.norm1.gg, bw.norm1.gb, dres=dx1, alpha=alpha,
                             accumulate=acc, dxsum=prev_fc2_gb if fuse else None)


# =============================================================================================== encoder
def _wait_gates(gates, chained):
    """gates [(first_block, event)]: the weights of blocks >= first_block are final after the event (the previous step's
    range-by-range update, engine/step.py).  The entry gate (block 0: embedding + first range) is waited for here; with the
    C chain the later ones are waited for between the ranges of the trunk (chain.blocks_forward), otherwise all of them now."""
    if not gates:
        return
    cur = torch.cuda.current_stream()
    for b, ev in gates:
        if b == 0 or not chained:
            cur.wait_event(ev)


def _pack_masked(pack, clips, tubelet, patch, masks, kdim):
    """The patch rows every mask keeps, mask after mask: (tok bf16 [sum_i B*K_i, kdim], segs)."""
    segs = Seg.table(clips.shape[0], [m.shape[1] for m in masks])
    tok = torch.empty((_total_rows(segs), kdim), dtype=torch.bfloat16, device=clips.device)
    for sg, m in zip(segs, masks):
        pack(clips, tubelet, patch, idx=m, out=_rows(tok, sg))
    return tok, segs


def _chained(ws_tag) -> bool:
    """The trunk goes out as C launch chains: the caller owns a workspace (ws_tag, engine/chain.py) and the switch is on.
    USE_C_CHAIN is read at call time (tests flip it between two trainers)."""
    return ws_tag is not None and USE_C_CHAIN


def _scaled_mlp(drop, li) -> bool:
    """Block li's MLP branch carries a stochastic-depth scale: its fc2 bias gradient takes no fused route."""
    return bool(drop) and drop[li] is not None and drop[li][1] is not None


def _check_drop(drop, n_blocks, B, ws_tag):
    """A non-empty stochastic-depth list: one (s_attn, s_mlp) entry per block, each scale None or fp32 [B] on the device, and no
    C launch chain (a caller with a workspace, ws_tag, is the Trainer, which has no stochastic depth)."""
    if not drop:
        return
    if ws_tag is not None:
        raise ValueError("stochastic depth runs on the per-kernel block chain only: the C launch chains (ws_tag) serve the "
                         "Trainer, which has none")
    if len(drop) != n_blocks:
        raise ValueError(f"stochastic depth: {len(drop)} scale entries for {n_blocks} blocks")
    for d in drop:
        for s in (d or ()):
            if s is not None and (s.dtype != torch.float32 or tuple(s.shape) != (B,)):
                raise ValueError(f"stochastic depth: a scale is {s.dtype} {tuple(s.shape)}, expected float32 ({B},): one per clip")


def _trunk_forward(x, views, segs, save, ws_tag, gemm_flags=0, gates=None, drop=None):
    """x through every block of `views` (EncoderW / PredictorW) -> (x, saved blocks): one C call per gated range, else the
    per-kernel Python chain.  drop: None, or one entry per block (block_forward's drop); the per-kernel chain only."""
    _check_drop(drop, len(views.blocks), segs[0].B if segs else 0, ws_tag)
    if _chained(ws_tag):
        return chain.blocks_forward(x, views, segs, save, ws_tag, LN_EPS, gemm_flags=gemm_flags, gates=gates)
    folds = None if save else getattr(views, "folds", None)
    saved_blocks = []
    for bi, bw in enumerate(views.blocks):
        x, sv = block_forward(x, bw, segs, views.heads, save, fold=None if folds is None else folds[bi],
                              drop=drop[bi] if drop else None)
        saved_blocks.append(sv)
    return x, saved_blocks


def _trunk_backward(dx, saved_blocks, views, segs, tag, alpha, beta, on_layer_done, ws_tag, last_fc2_bias_done, drop=None):
    """The blocks of `views` in reverse, whichever chain the forward took; on_layer_done(tag, layer) after every block.
    drop: the forward's per-block list; a block whose MLP branch is scaled gets its fc2 bias gradient from no LayerNorm backward."""
    done = None if on_layer_done is None else (lambda li: on_layer_done(tag, li))
    if isinstance(saved_blocks, chain.TrunkCtx):
        side = side_stream(dx.device)
        return chain.blocks_backward(dx, saved_blocks, views, alpha, side.stream.cuda_stream if side.enabled else None, done,
                                     beta_acc=beta, tag=ws_tag, last_fc2_bias_done=last_fc2_bias_done)
    nb = len(views.blocks)
    for li in range(nb - 1, -1, -1):
        dx = block_backward(dx, saved_blocks[li], views.blocks[li], segs, views.heads, alpha, beta,
                            fc2_bias_done=(li + 1 < nb or last_fc2_bias_done) and not _scaled_mlp(drop, li),
                            prev_fc2_gb=views.blocks[li - 1].fc2.gb if li > 0 and not _scaled_mlp(drop, li - 1) else None,
                            drop=drop[li] if drop else None)
        saved_blocks[li] = None
        if done is not None:
            done(li)      # bucket launch waits on the side stream's event, not on this stream
    return dx


def _image_model_tokens(ew: EncoderW, clips, masks, N, kdim):
    """Patch rows of the image model's input (tok bf16 [rows, 3*p*p], segs): images [B,3,H,W], or frames given as one clip tensor
    [B,3,T,H,W] or a list of such tensors of one frame size.  vj_tubelet_pack with tubelet 1 emits a clip's rows in (b,t,h,w) order,
    which is frame-major: every frame becomes its own sequence of N tokens, the frames of a list following one another part by part,
    and no [B*T,3,H,W] copy of the pixels is made.  Masks address one image's token grid and go with images only.  The shapes were
    validated by VisionTransformer.forward / forward_frames; this only packs."""
    parts = list(clips) if isinstance(clips, (list, tuple)) else [clips]
    parts = [c.unsqueeze(2) if c.dim() == 4 else c for c in parts]      # a view: an image is its own one-frame clip
    p = ew.patch_size
    if (parts[0].shape[-2] // p) * (parts[0].shape[-1] // p) != N:     # the callers checked that the parts share one frame size
        raise ValueError(f"encoder_forward: position table of {N} rows does not fit images of "
                         f"{parts[0].shape[-2] // p}x{parts[0].shape[-1] // p} cells")
    frames = [c.shape[0] * c.shape[2] for c in parts]
    if masks is None:
        segs = [Seg(0, sum(frames), N)]
        if len(parts) == 1:
            return ops.tubelet_pack(parts[0], 1, p), segs
        tok = torch.empty((sum(frames) * N, kdim), dtype=torch.bfloat16, device=parts[0].device)
        r = 0
        for c, f in zip(parts, frames):
            ops.tubelet_pack(c, 1, p, out=tok[r:r + f * N])
            r += f * N
        return tok, segs
    if len(parts) != 1 or parts[0].shape[2] != 1:
        raise ValueError("encoder_forward: masks address one image's token grid; frames [B,C,T,H,W] take none")
    return _pack_masked(ops.tubelet_pack, parts[0], 1, p, masks, kdim)


def encoder_forward(ew: EncoderW, clips, masks: Optional[List[torch.Tensor]], save: bool, final_norm=True, ws_tag=None,
                    gemm_flags=0, gates=None, pos=None, drop=None):
    """clips fp32 [B,3,T,H,W], or still images [B,3,H,W] standing for the clip that repeats each image along time; for the image
    model (ew.image) images [B,3,H,W], or frames [B,3,T,H,W] (or a list of such clips) each encoded on its own (_image_model_tokens); masks:
    None (all N tokens) or a list of int64 [B,K_i] index tensors.  pos (fp32 [N, D], default ew.pos): the position table of
    the input's token grid (gt, gh, gw), N = gt*gh*gw; the grid is taken from the input (and, for a still image, gt from N).
    Returns (out [sum_i B*K_i, D] bf16, segs, saved).  With final_norm=False the last residual stream is returned
    (the target path fuses the final norm into vj_target_rows).  gates: see _wait_gates.  drop: stochastic depth, None or one
    (s_attn, s_mlp) entry per block (block_forward); the scales are per clip, [B], shared by every mask segment -- per image for a
    video encoder's still images, whose repeated clip is one sequence like any clip.  save: keep what encoder_backward needs; the
    saved tuple ends with the still front end's fan-out (B, cells, gt), None for every other input.

    Still images: only the gh*gw distinct tubelets are packed and embedded (vj_image_pack, a GEMM on B*gh*gw rows) and the gt
    temporal slices differ only in their position rows (vj_add_pos_bcast); with masks, the kept rows are packed one by one
    (vj_image_pack with idx) and go through the same GEMM and vj_add_pos as a clip's.  Both equal the materialised repeated
    clip bit for bit: the packed rows hold the same bf16 pixels, the NT GEMM accumulates a row's dot product in the same K
    order in every execution form, and the position add is the same single fp32 rounding."""
    D = ew.patch.w.shape[0]
    kdim = ew.patch.w.shape[1]
    pos = ew.pos if pos is None else pos
    N = pos.shape[0]
    if drop:
        if ew.image or clips.dim() not in (4, 5):
            raise ValueError("encoder_forward: stochastic depth goes with a video encoder's clips [B,3,T,H,W] or still images [B,3,H,W]")
        _check_drop(drop, len(ew.blocks), clips.shape[0], ws_tag)
    if ew.image:
        if save:
            raise ValueError("encoder_forward: the image model is a frozen (save=False) path")
        still = False
        tok, segs = _image_model_tokens(ew, clips, masks, N, kdim)
    else:
        B = clips.shape[0]
        still = clips.dim() == 4
        cells = (clips.shape[-2] // ew.patch_size) * (clips.shape[-1] // ew.patch_size)
        if still:
            if cells == 0 or N % cells != 0:
                raise ValueError(f"encoder_forward: position table of {N} rows does not fit images of {cells} cells")
        elif (clips.shape[2] // ew.tubelet) * cells != N:
            raise ValueError(f"encoder_forward: position table of {N} rows does not fit the input's token grid "
                             f"{clips.shape[2] // ew.tubelet}x{clips.shape[-2] // ew.patch_size}x{clips.shape[-1] // ew.patch_size}")
        pack = ops.image_pack if still else ops.tubelet_pack
        if masks is None:
            segs = [Seg(0, B, N)]
            tok = pack(clips, ew.tubelet, ew.patch_size)
        else:
            tok, segs = _pack_masked(pack, clips, ew.tubelet, ew.patch_size, masks, kdim)
    _wait_gates(gates, _chained(ws_tag))
    x = ops.gemm_nt(tok, ew.patch.w, bias=ew.patch.b, flags=(gemm_flags & 0xffff if not gemm_flags >> 16 else 0) or None)
    if still and masks is None:
        x = ops.add_pos_bcast(x, pos, B, cells, N // cells)
    else:
        for i, sg in enumerate(segs):
            ops.add_pos(_rows(x, sg), pos, sg.B, sg.S, idx=None if masks is None else masks[i])
    x, saved_blocks = _trunk_forward(x, ew, segs, save, ws_tag, gemm_flags, gates, drop=drop or None)
    if not final_norm:
        return x, segs, None
    out, mean, rstd = ops.layernorm_fwd(x, ew.norm.g, ew.norm.b, LN_EPS, save_stats=save)
    fan = (B, cells, N // cells) if still and masks is None else None
    saved = (tok, saved_blocks, x, mean, rstd, drop or None, fan) if save else None
    return out, segs, saved


def encoder_backward(dout, saved, ew: EncoderW, segs, alpha: float, on_layer_done=None, beta: float = 0.0,
                     ws_tag="bwd_tmp"):
    """dout [M, D] bf16: gradient of the encoder output rows.  Pixels need no gradient.  Parameter gradients are written
    as alpha * grad + beta * old (beta = 1 accumulates micro-batches).

    Still images without masks (the saved fan-out (B, cells, gt)): the forward embedded B*cells packed rows and fanned them out
    over the gt temporal slices (vj_add_pos_bcast), so the gradient of those embeddings is the sum of the trunk's input gradient
    over the slices (vj_slice_sum, rounded to bf16 once) and the patch embedding's weight and bias gradients come from B*cells
    rows.  Still images with masks packed their kept rows one by one: tok has one row per gradient row, as a clip's, and the
    plain backward below is already right."""
    tok, saved_blocks, xl, mean, rstd, drop, fan = saved
    # dx of the final norm's backward is the dY of the last block's fc2: with the transpose-free route its bias gradient (the
    # column sums of dx) comes out of this pass like every other block's (round 4: no stand-alone column sum left in a trunk)
    # (not for a last block whose MLP branch is scaled by stochastic depth: its fc2's dY is the scaled copy of dx)
    last_gb = ew.blocks[-1].fc2.gb if _tn_ok(8, 8) and not _scaled_mlp(drop, len(ew.blocks) - 1) else None
    dx = ops.layernorm_bwd(dout, xl, ew.norm.g, mean, rstd, ew.norm.gg, ew.norm.gb, alpha=alpha, accumulate=beta != 0.0,
                           dxsum=last_gb)
    dx = _trunk_backward(dx, saved_blocks, ew, segs, "enc", alpha, beta, on_layer_done, ws_tag, last_gb is not None, drop=drop)
    if fan is not None:
        dx = ops_still.slice_sum(dx, *fan)
    _linear_backward(dx, tok, ew.patch, alpha, need_dx=False, beta=beta)
    side_stream(dout.device).join()
    if on_layer_done is not None:
        on_layer_done("enc", -1)


# =============================================================================================== predictor
def predictor_forward(pw: PredictorW, z, enc_segs: List[Seg], masks_enc, masks_pred, save: bool, ws_tag=None,
                      gemm_flags=0, gates=None):
    """z [sum_i B*Ke_i, D] bf16 (context-encoder output rows, per-mask segments enc_segs).
    Returns (zhat [sum_i B*Kp_i, D] bf16, tgt_segs, saved).  gates: [(0, event)] -- the predictor's weights are one range."""
    Dp = pw.embed.w.shape[0]
    dev = z.device
    _wait_gates(gates, False)
    e = ops.gemm_nt(z, pw.embed.w, bias=pw.embed.b)
    n_tok = len(pw.mask_tokens)
    B = enc_segs[0].B     # the segments of one batch: the callers build them with one B
    tsegs = Seg.table(B, [mp.shape[1] for _, mp in zip(enc_segs, masks_pred)])     # target rows
    segs = Seg.table(B, [sg.S + tsg.S for sg, tsg in zip(enc_segs, tsegs)])        # whole sequences: context + target rows
    x = torch.empty((_total_rows(segs), Dp), dtype=torch.bfloat16, device=dev)
    for i, (sg, psg) in enumerate(zip(enc_segs, segs)):
        # mask_index = i % num_mask_tokens (predictor.py:206; PredictorMultiMaskWrapper passes mask_index=i)
        ops.pred_assemble(_rows(e, sg), pw.mask_tokens[i % n_tok], pw.pos, masks_enc[i], masks_pred[i],
                          out=_rows(x, psg))
    x, saved_blocks = _trunk_forward(x, pw, segs, save, ws_tag, gemm_flags)
    # predictor_norm is row-wise and only target rows are projected (x[:, N_ctxt:], predictor.py:233-237):
    # normalise just those rows.
    t = torch.empty((_total_rows(tsegs), Dp), dtype=torch.bfloat16, device=dev)
    for sg, psg, tsg in zip(enc_segs, segs, tsegs):
        ops.copy_rows(_rows(x, psg), _rows(t, tsg), psg.B, psg.S, sg.S, tsg.S, 0, tsg.S, Dp)
    tn, mean, rstd = ops.layernorm_fwd(t, pw.norm.g, pw.norm.b, LN_EPS, save_stats=save)
    zhat = ops.gemm_nt(tn, pw.proj.w, bias=pw.proj.b)
    saved = (z, e.shape, segs, tsegs, saved_blocks, t, tn, mean, rstd) if save else None
    return zhat, tsegs, saved


def predictor_backward(dzhat, saved, pw: PredictorW, enc_segs, alpha: float, on_layer_done=None, beta: float = 0.0,
                       ws_tag="bwd_tmp"):
    """dzhat [sum_i B*Kp_i, D] bf16 -> returns dz [sum_i B*Ke_i, D] bf16 (gradient of the encoder output)."""
    z, e_shape, segs, tsegs, saved_blocks, t, tn, mean, rstd = saved
    Dp = pw.embed.w.shape[0]
    n_tok = len(pw.mask_tokens)
    acc = beta != 0.0
    dtn = _linear_backward(dzhat, tn, pw.proj, alpha, beta=beta)
    # the trunk's output gradient is dt on the target rows and zero on the context rows, so the last block's fc2 bias gradient
    # (column sums over ALL rows of that gradient) is the column sum of dt: it comes out of this LayerNorm backward
    last_gb = pw.blocks[-1].fc2.gb if _tn_ok(8, 8) else None
    dt = ops.layernorm_bwd(dtn, t, pw.norm.g, mean, rstd, pw.norm.gg, pw.norm.gb, alpha=alpha, accumulate=acc, dxsum=last_gb)
    dx = torch.empty((_total_rows(segs), Dp), dtype=torch.bfloat16, device=dzhat.device)
    for sg, psg, tsg in zip(enc_segs, segs, tsegs):
        ops.copy_rows(None, _rows(dx, psg), psg.B, 0, 0, psg.S, 0, sg.S, Dp)   # context rows start at zero grad (no ATen fill on the step)
        ops.copy_rows(_rows(dt, tsg), _rows(dx, psg), psg.B, tsg.S, 0, psg.S, sg.S, tsg.S, Dp)
    if on_layer_done is not None:
        on_layer_done("pred", len(pw.blocks))
    dx = _trunk_backward(dx, saved_blocks, pw, segs, "pred", alpha, beta, on_layer_done, ws_tag, last_gb is not None)
    # token assembly backward: mask-token grads = sum of the target rows; context rows flow to predictor_embed
    de = torch.empty(e_shape, dtype=torch.bfloat16, device=dzhat.device)
    used = set()
    for i, (sg, psg) in enumerate(zip(enc_segs, segs)):
        ti = i % n_tok
        ops.colsum(_rows(dx, psg), pw.g_mask_tokens[ti], alpha=alpha, accumulate=(ti in used) or acc, group=psg.S,
                   row_lo=sg.S, row_hi=psg.S)
        used.add(ti)
        ops.copy_rows(_rows(dx, psg), _rows(de, sg), psg.B, psg.S, 0, sg.S, 0, sg.S, Dp)
    for ti in range(n_tok):
        if ti not in used and not acc:
            pw.g_mask_tokens[ti].zero_()
    dz = _linear_backward(de, z, pw.embed, alpha, beta=beta)
    side_stream(dzhat.device).join()
    if on_layer_done is not None:
        on_layer_done("pred", -1)
    return dz
