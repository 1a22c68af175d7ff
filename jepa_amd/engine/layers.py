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
from typing import Any, List, NamedTuple, Optional

import numpy as np
import torch

from ..hip import ops
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


# =============================================================================================== saved state
# What a forward with save=True hands its backward.  Built by keyword, read by name; opaque to everything outside this module.
class BlockSaved(NamedTuple):
    x: Any          # the block's input [M, D]
    y1: Any         # norm1(x), with its row statistics
    mean1: Any
    rstd1: Any
    qkv: Any
    o: Any          # attention output, before proj
    lses: Any       # one log-sum-exp tensor per segment
    x1: Any         # x + attention branch
    y2: Any         # norm2(x1), with its row statistics
    mean2: Any
    rstd2: Any
    u: Any          # gelu'(fc1 pre-activation)
    g: Any          # gelu(fc1 pre-activation), the input of fc2


class EncoderSaved(NamedTuple):
    tok: Any        # the packed patch rows, the patch GEMM's input
    blocks: Any     # [BlockSaved] (each dropped as soon as its backward has run), or the C chain's TrunkCtx
    x: Any          # the last residual stream, the final norm's input, with its row statistics
    mean: Any
    rstd: Any
    drop: Any       # the forward's drop-path plan (_drop_plan)
    fan: Any        # the still front end's fan-out (B, cells, gt); None for every other input
    recompute: Any = None   # the forward's activation-recomputation mode (_recompute_mode): None (every record kept), "mlp" or "block"


class PredictorSaved(NamedTuple):
    z: Any          # the context-encoder output rows, predictor_embed's input
    e_shape: Any    # shape of the embedded context rows
    segs: Any       # whole sequences: context + target rows
    tsegs: Any      # target rows
    blocks: Any     # as EncoderSaved.blocks
    t: Any          # the trunk's target rows, the predictor norm's input, with its output and row statistics
    tn: Any
    mean: Any
    rstd: Any


# =============================================================================================== block
_UNSCALED = (None, None)    # a block's entry of a drop-path plan when neither branch carries a stochastic-depth scale


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


def block_forward(x, bw: BlockW, segs: List[Seg], heads: int, save: bool, fold=None, drop=_UNSCALED):
    """x [M, D] bf16 -> x2 [M, D]; returns (x2, saved).  fold (FoldW, only with save = False): both LayerNorms folded into the
    GEMMs that consume them -- the kernels and their order are those of vj_blocks_fwd_lnfold (bit-identical results).
    drop (stochastic depth): the block's entry of a drop-path plan, (s_attn, s_mlp), each None or an fp32 [B] tensor of per-sample
    scales.  A branch with a scale leaves its last GEMM without the fused residual (the branch is rounded to bf16 once) and
    _drop_residual finishes it in place (the sum is rounded once); a branch without one issues exactly the launches of no drop."""
    s_attn, s_mlp = drop
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
    saved = BlockSaved(x=x, y1=y1, mean1=mean1, rstd1=rstd1, qkv=qkv, o=o, lses=lses, x1=x1, y2=y2, mean2=mean2, rstd2=rstd2, u=u,
                       g=g) if save else None
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
                   fc2_bias_done: bool = False, prev_fc2_gb=None, drop=_UNSCALED):
    """With transpose-free weight gradients the bias gradients of proj and of the PREVIOUS block's fc2 are the column
    sums of the two LayerNorm backward outputs and come out of those passes (vj_layernorm_bwd_colsum); `fc2_bias_done`
    says that this block's fc2 bias gradient was produced that way by the block above, and `prev_fc2_gb` is what this block's
    last pass fills for the block below.  Both are final: _fc2_gb_route decided them (_trunk_backward).  Same kernels, same order
    as vj_blocks_bwd (csrc/chain.hip): bit-identical results.
    drop = (s_attn, s_mlp) of the forward.  The dY of a scaled branch's last Linear is the scaled copy of the stream's gradient
    (_drop_grad), which feeds its dgrad, weight and bias gradient, while the LayerNorm backward below still adds the unscaled
    gradient as dres.  That Linear's bias gradient is then NOT the column sum of a LayerNorm backward's output: for a scaled MLP
    branch the caller passes fc2_bias_done = False (and prev_fc2_gb = None to the block above it), a scaled attention branch takes
    proj.gb from ops.colsum."""
    s_attn, s_mlp = drop
    D = saved.x.shape[1]
    hd = D // heads
    scale = hd ** -0.5
    if _q_prescaled(D):
        scale = -scale       # the forward stored q pre-scaled (option attn_softmax = 2)
    acc = beta != 0.0
    proj_gb = bw.proj.gb if _tn_ok(8, 8) and s_attn is None else None    # the attention branch's route: a one-block fact
    defer = [] if _group_ok(bw) else None
    dfc2 = dx2 if s_mlp is None else _drop_grad(dx2, s_mlp, segs)
    du = _linear_backward(dfc2, saved.g, bw.fc2, alpha, dgelu_aux=saved.u, beta=beta, bias_done=fc2_bias_done,
                          defer=defer)   # fc2 dgrad fused with GELU'
    dy2 = _linear_backward(du, saved.y2, bw.fc1, alpha, beta=beta, defer=defer)
    dx1 = ops.layernorm_bwd(dy2, saved.x1, bw.norm2.g, saved.mean2, saved.rstd2, bw.norm2.gg, bw.norm2.gb, dres=dx2, alpha=alpha,
                            accumulate=acc, dxsum=proj_gb)
    dproj = dx1 if s_attn is None else _drop_grad(dx1, s_attn, segs)
    do = _linear_backward(dproj, saved.o, bw.proj, alpha, beta=beta, bias_done=proj_gb is not None, defer=defer)
    dqkv = torch.empty_like(saved.qkv)
    for sg, lse in zip(segs, saved.lses):
        ops.attn_bwd(_rows(saved.qkv, sg), _rows(saved.o, sg), _rows(do, sg), lse, sg.B, sg.S, heads, hd, scale,
                     out=_rows(dqkv, sg))
    if defer is not None:
        defer.append((dqkv, saved.y1, bw.qkv, False))
        _wgrad_group(defer, alpha, beta)
        dy1 = ops.gemm_nt(dqkv, bw.qkv.wT)
    else:
        dy1 = _linear_backward(dqkv, saved.y1, bw.qkv, alpha, beta=beta)
    return ops.layernorm_bwd(dy1, saved.x, bw.norm1.g, saved.mean1, saved.rstd1, bw.norm1.gg, bw.norm1.gb, dres=dx1, alpha=alpha,
                             accumulate=acc, dxsum=prev_fc2_gb)


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


_DROP_ON_C_CHAIN = ("stochastic depth runs on the per-kernel block chain only: the C launch chains (ws_tag) serve the Trainer, which "
                    "has none")


def _check_drop(drop, n_blocks, B, ws_tag):
    """A non-empty stochastic-depth list: one (s_attn, s_mlp) entry per block, each scale None or fp32 [B] on the device, and no
    C launch chain (a caller with a workspace, ws_tag, is the Trainer, which has no stochastic depth)."""
    if not drop:
        return
    if ws_tag is not None:
        raise ValueError(_DROP_ON_C_CHAIN)
    if len(drop) != n_blocks:
        raise ValueError(f"stochastic depth: {len(drop)} scale entries for {n_blocks} blocks")
    for d in drop:
        for s in (d or ()):
            if s is not None and (s.dtype != torch.float32 or tuple(s.shape) != (B,)):
                raise ValueError(f"stochastic depth: a scale is {s.dtype} {tuple(s.shape)}, expected float32 ({B},): one per clip")


def _drop_plan(ew: EncoderW, clips, drop, ws_tag):
    """The caller's stochastic-depth list, validated and normalised once per encoder call: None (no list, or an empty one), or one
    (s_attn, s_mlp) pair per block, _UNSCALED standing for a block whose entry is None.  The scales are per clip, [B], shared by
    every mask segment -- per image for a video encoder's still images, whose repeated clip is one sequence like any clip.  The
    trunk walkers, block_forward, block_backward and _fc2_gb_route take this form as it is."""
    if not drop:
        return None
    if ew.image or clips.dim() not in (4, 5):
        raise ValueError("encoder_forward: stochastic depth goes with a video encoder's clips [B,3,T,H,W] or still images [B,3,H,W]")
    _check_drop(drop, len(ew.blocks), clips.shape[0], ws_tag)
    return [_UNSCALED if d is None else d for d in drop]


def _fc2_gb_route(views, li, plan):
    """The one owner of "which LayerNorm backward writes block li's fc2 bias gradient": the tensor that the LayerNorm backward
    producing block li's fc2 dY (norm1 of block li + 1; the final norm for the last block) must fill as `dxsum`, or None when that
    bias gradient takes the column-sum route of _wgrad instead (and for li = -1: block 0 has no block below it).  It is fc2.gb
    when the weight gradients are transpose-free and the block's MLP branch carries no stochastic-depth scale: a scaled branch's
    fc2 dY is the scaled copy of that dx (block_backward), not the dx whose columns the pass sums.  A wrong answer doubles the bias
    gradient or leaves it unwritten, so nobody else decides this."""
    if li < 0 or not _tn_ok(8, 8) or (plan is not None and plan[li][1] is not None):
        return None
    return views.blocks[li].fc2.gb


RECOMPUTE_MODES = ("none", "mlp", "block")
_RECOMPUTE_ON_C_CHAIN = ("activation recomputation runs on the per-kernel block chain only: the C launch chains (ws_tag) serve the "
                         "Trainer, which keeps every record")


def recompute_mode(mode, what="recompute"):
    """The activation-recomputation mode as the chain carries it: None for off (None or "none"), else "mlp" or "block".  Anything
    else, a bool or a number included, raises and names the three."""
    if mode is None or (isinstance(mode, str) and mode == "none"):
        return None
    if isinstance(mode, str) and mode in RECOMPUTE_MODES:
        return mode
    raise ValueError(f"{what}={mode!r}: activation recomputation is one of 'none', 'mlp', 'block'")


def _recompute_mode(mode, save, ws_tag):
    """recompute_mode for one encoder call: a mode goes with a forward that keeps a record (save=True) and with no workspace."""
    mode = recompute_mode(mode, "encoder_forward: recompute")
    if mode is None:
        return None
    if ws_tag is not None:
        raise ValueError(_RECOMPUTE_ON_C_CHAIN)
    if not save:
        raise ValueError(f"encoder_forward: recompute={mode!r} with save=False: a forward that keeps nothing has nothing to recompute")
    return mode


def _slim(sv: BlockSaved, mode):
    """What of a block's record survives the forward under a recomputation mode.  "block": the input x alone.  "mlp": everything but
    u and g, the two [M, 4D] tensors -- half of the record."""
    if mode == "block":
        return BlockSaved(*(sv.x if f == "x" else None for f in BlockSaved._fields))
    return sv._replace(u=None, g=None)


def _refill(sv: BlockSaved, bw: BlockW, segs, heads, mode, drop):
    """The full record of a block from its slimmed one, by the forward's own launches on the forward's own inputs: the same bits.
    "block": block_forward again on the saved x with the block's plan entry (its output, the next block's x, is not kept).
    "mlp": the fc1 GEMM on the saved y2, which writes g and, through aux_out, u."""
    if mode == "block":
        return block_forward(sv.x, bw, segs, heads, True, drop=drop)[1]
    u = torch.empty((sv.y2.shape[0], bw.fc1.w.shape[0]), dtype=torch.bfloat16, device=sv.y2.device)
    g = ops.gemm_nt(sv.y2, bw.fc1.w, bias=bw.fc1.b, aux_out=u, epilogue=ops.EPI_GELU)
    return sv._replace(u=u, g=g)


def _trunk_forward(x, views, segs, save, ws_tag, gemm_flags=0, gates=None, drop=None, recompute=None):
    """x through every block of `views` (EncoderW / PredictorW) -> (x, saved blocks): one C call per gated range, else the
    per-kernel Python chain.  drop: None, or a drop-path plan as _drop_plan returns it -- a plan only: a caller's raw list is
    neither validated nor normalised here.  A plan goes with the per-kernel chain only; the guard below keeps one from being
    dropped silently in front of the C chain.  recompute: None, "mlp" or "block" (_recompute_mode), under the same guard: every
    block runs its plain save=True forward -- the unfolded LayerNorms, the same epilogues, the same bits -- and its record is slimmed at
    once (_slim), so at most one full record is alive."""
    if drop is not None and ws_tag is not None:
        raise ValueError(_DROP_ON_C_CHAIN)
    if recompute is not None and (ws_tag is not None or not save):
        raise ValueError(_RECOMPUTE_ON_C_CHAIN if ws_tag is not None else "activation recomputation goes with save=True")
    if _chained(ws_tag):
        return chain.blocks_forward(x, views, segs, save, ws_tag, LN_EPS, gemm_flags=gemm_flags, gates=gates)
    folds = None if save else getattr(views, "folds", None)
    saved_blocks = []
    for bi, bw in enumerate(views.blocks):
        x, sv = block_forward(x, bw, segs, views.heads, save, fold=None if folds is None else folds[bi],
                              drop=_UNSCALED if drop is None else drop[bi])
        saved_blocks.append(sv if recompute is None else _slim(sv, recompute))
        del sv
    return x, saved_blocks


def _trunk_backward(dx, saved_blocks, views, segs, tag, alpha, beta, on_layer_done, ws_tag, drop=None, recompute=None):
    """The blocks of `views` in reverse, whichever chain the forward took; on_layer_done(tag, layer) after every block.  The caller's
    LayerNorm backward, which produced dx, filled _fc2_gb_route(views, last block, drop).  drop: the forward's drop-path plan.
    recompute: the forward's mode; directly before a block's backward its slimmed record is refilled (_refill), and the refilled
    tensors go as a saved record goes, right after the block's backward: block_backward hands what the weight gradients read to
    the side stream through side.fork like any saved tensor, so the allocator keeps that memory until the side stream is past it.
    That alone is safe but saves nothing: the host issues the whole backward long before the GPU runs it, and every refilled record
    would still be held back for the side stream when the next one is allocated (measured: the allocator's peak did not move).  So
    under a mode the host waits, before refilling block i, for the side stream to be past block i + 2: at most three records exist,
    the one being refilled and two awaiting their weight gradients, and the GPU always has two blocks of work queued."""
    done = None if on_layer_done is None else (lambda li: on_layer_done(tag, li))
    nb = len(views.blocks)
    fc2_gb = _fc2_gb_route(views, nb - 1, drop)
    if isinstance(saved_blocks, chain.TrunkCtx):
        side = side_stream(dx.device)
        return chain.blocks_backward(dx, saved_blocks, views, alpha, side.stream.cuda_stream if side.enabled else None, done,
                                     beta_acc=beta, tag=ws_tag, last_fc2_bias_done=fc2_gb is not None)
    side = side_stream(dx.device) if recompute is not None else None
    behind = [] if side is not None and side.enabled else None      # events on the side stream, one per block whose backward is issued
    for li in range(nb - 1, -1, -1):
        prev_fc2_gb = _fc2_gb_route(views, li - 1, drop)
        entry = _UNSCALED if drop is None else drop[li]
        rec = saved_blocks[li]
        if recompute is not None:
            if behind is not None and len(behind) == 2:
                behind.pop(0).synchronize()
            rec = _refill(rec, views.blocks[li], segs, views.heads, recompute, entry)
        dx = block_backward(dx, rec, views.blocks[li], segs, views.heads, alpha, beta,
                            fc2_bias_done=fc2_gb is not None, prev_fc2_gb=prev_fc2_gb, drop=entry)
        saved_blocks[li] = rec = None     # the block's record goes as soon as its backward has run
        if behind is not None:
            behind.append(side.stream.record_event())     # (after the release: behind what the allocator recorded for it)
        fc2_gb = prev_fc2_gb
        if done is not None:
            done(li)      # bucket launch waits on the side stream's event, not on this stream
    return dx


def _pack_tokens(ew: EncoderW, clips, masks, N):
    """The front end of encoder_forward: (ew, input, masks, rows N of the position table) -> (tok bf16 [rows, kdim], segs, fan): the
    packed patch rows, the segment table and, for a video encoder's still images without masks, the fan-out (B, cells, gt) of the
    B*cells packed rows over the gt temporal slices (None for every other input).  All shape validation of the three input kinds is
    here, and nothing but the packing kernels is launched.

    The image model (ew.image): images [B,3,H,W], or frames given as one clip tensor [B,3,T,H,W] or a list of such tensors of one
    frame size (VisionTransformer.forward_frames checked that they share it).  vj_tubelet_pack with tubelet 1 emits a clip's rows in
    (b,t,h,w) order, which is frame-major: every frame becomes its own sequence of N tokens, the frames of a list following one
    another part by part, and no [B*T,3,H,W] copy of the pixels is made.  Masks address one image's token grid and go with images
    only.

    A video encoder's clips [B,3,T,H,W]: vj_tubelet_pack, every row or the rows each mask keeps, mask after mask.

    A video encoder's still images [B,3,H,W], standing for the clip that repeats each image along time (gt is taken from N): only
    the gh*gw distinct tubelets are packed (vj_image_pack); with masks, the kept rows are packed one by one (vj_image_pack with idx)
    and tok has one row per output row, as a clip's."""
    p, kdim = ew.patch_size, ew.patch.w.shape[1]
    if ew.image:
        parts = list(clips) if isinstance(clips, (list, tuple)) else [clips]
        parts = [c.unsqueeze(2) if c.dim() == 4 else c for c in parts]      # a view: an image is its own one-frame clip
        if (parts[0].shape[-2] // p) * (parts[0].shape[-1] // p) != N:
            raise ValueError(f"encoder_forward: position table of {N} rows does not fit images of "
                             f"{parts[0].shape[-2] // p}x{parts[0].shape[-1] // p} cells")
        if masks is not None:
            if len(parts) != 1 or parts[0].shape[2] != 1:
                raise ValueError("encoder_forward: masks address one image's token grid; frames [B,C,T,H,W] take none")
            return (*_pack_masked(ops.tubelet_pack, parts[0], 1, p, masks, kdim), None)
        frames = [c.shape[0] * c.shape[2] for c in parts]
        segs = [Seg(0, sum(frames), N)]
        if len(parts) == 1:
            return ops.tubelet_pack(parts[0], 1, p), segs, None
        tok = torch.empty((sum(frames) * N, kdim), dtype=torch.bfloat16, device=parts[0].device)
        r = 0
        for c, f in zip(parts, frames):
            ops.tubelet_pack(c, 1, p, out=tok[r:r + f * N])
            r += f * N
        return tok, segs, None
    B, still = clips.shape[0], clips.dim() == 4
    cells = (clips.shape[-2] // p) * (clips.shape[-1] // p)
    if still:
        if cells == 0 or N % cells != 0:
            raise ValueError(f"encoder_forward: position table of {N} rows does not fit images of {cells} cells")
    elif (clips.shape[2] // ew.tubelet) * cells != N:
        raise ValueError(f"encoder_forward: position table of {N} rows does not fit the input's token grid "
                         f"{clips.shape[2] // ew.tubelet}x{clips.shape[-2] // p}x{clips.shape[-1] // p}")
    pack = ops.image_pack if still else ops.tubelet_pack
    if masks is not None:
        return (*_pack_masked(pack, clips, ew.tubelet, p, masks, kdim), None)
    return pack(clips, ew.tubelet, p), [Seg(0, B, N)], (B, cells, N // cells) if still else None


def _add_positions(x, pos, segs, masks, fan):
    """The position rows onto the embedded tokens x.  With a fan-out (still images without masks) x holds B*cells rows and the gt
    temporal slices differ only in their position rows: vj_add_pos_bcast writes the B*gt*cells rows of the trunk's input.  Every other
    input has its rows already and takes vj_add_pos in place, segment by segment, through its mask's indices."""
    if fan is not None:
        return ops.add_pos_bcast(x, pos, *fan)
    for i, sg in enumerate(segs):
        ops.add_pos(_rows(x, sg), pos, sg.B, sg.S, idx=None if masks is None else masks[i])
    return x


def encoder_forward(ew: EncoderW, clips, masks: Optional[List[torch.Tensor]], save: bool, final_norm=True, ws_tag=None,
                    gemm_flags=0, gates=None, pos=None, drop=None, recompute=None):
    """clips fp32 [B,3,T,H,W], or still images [B,3,H,W] standing for the clip that repeats each image along time; for the image
    model (ew.image) images [B,3,H,W], or frames [B,3,T,H,W] (or a list of such clips) each encoded on its own (_pack_tokens); masks:
    None (all N tokens) or a list of int64 [B,K_i] index tensors.  pos (fp32 [N, D], default ew.pos): the position table of
    the input's token grid (gt, gh, gw), N = gt*gh*gw; the grid is taken from the input (and, for a still image, gt from N).
    Returns (out [sum_i B*K_i, D] bf16, segs, saved).  With final_norm=False the last residual stream is returned
    (the target path fuses the final norm into vj_target_rows).  gates: see _wait_gates.  drop: stochastic depth, None or one
    (s_attn, s_mlp) entry per block, each entry or scale possibly None (_drop_plan).  save: keep what encoder_backward needs, an
    EncoderSaved whose `fan` is the still front end's fan-out (B, cells, gt), None for every other input.  recompute: None or
    "none" (keep every block's record, the default), "mlp" (keep all but u and g; one fc1 GEMM refills them before the block's backward)
    or "block" (keep the block's input alone; block_forward runs again before the block's backward).  The per-kernel chain only, with
    save=True; outputs and gradients are the same bits in every mode.

    Still images: only the gh*gw distinct tubelets are packed and embedded (_pack_tokens, then a GEMM on B*gh*gw rows) and the gt
    temporal slices differ only in their position rows (_add_positions); with masks, the kept rows are packed one by one and go
    through the same GEMM and vj_add_pos as a clip's.  Both equal the materialised repeated clip bit for bit: the packed rows hold
    the same bf16 pixels, the NT GEMM accumulates a row's dot product in the same K order in every execution form (DESIGN.md
    section 5), and the position add is the same single fp32 rounding."""
    pos = ew.pos if pos is None else pos
    plan = _drop_plan(ew, clips, drop, ws_tag)
    recompute = _recompute_mode(recompute, save, ws_tag)
    if ew.image and save:
        raise ValueError("encoder_forward: the image model is a frozen (save=False) path")
    tok, segs, fan = _pack_tokens(ew, clips, masks, pos.shape[0])     # (the packing launches go out before the gates are waited for)
    _wait_gates(gates, _chained(ws_tag))
    x = ops.gemm_nt(tok, ew.patch.w, bias=ew.patch.b, flags=(gemm_flags & 0xffff if not gemm_flags >> 16 else 0) or None)
    x = _add_positions(x, pos, segs, masks, fan)
    x, saved_blocks = _trunk_forward(x, ew, segs, save, ws_tag, gemm_flags, gates, drop=plan, recompute=recompute)
    if not final_norm:
        return x, segs, None
    out, mean, rstd = ops.layernorm_fwd(x, ew.norm.g, ew.norm.b, LN_EPS, save_stats=save)
    saved = EncoderSaved(tok=tok, blocks=saved_blocks, x=x, mean=mean, rstd=rstd, drop=plan, fan=fan,
                         recompute=recompute) if save else None
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
    # dx of the final norm's backward is the dY of the last block's fc2: with the transpose-free route its bias gradient (the
    # column sums of dx) comes out of this pass like every other block's (round 4: no stand-alone column sum left in a trunk)
    # (not for a last block whose MLP branch is scaled by stochastic depth: its fc2's dY is the scaled copy of dx)
    dx = ops.layernorm_bwd(dout, saved.x, ew.norm.g, saved.mean, saved.rstd, ew.norm.gg, ew.norm.gb, alpha=alpha,
                           accumulate=beta != 0.0, dxsum=_fc2_gb_route(ew, len(ew.blocks) - 1, saved.drop))
    dx = _trunk_backward(dx, saved.blocks, ew, segs, "enc", alpha, beta, on_layer_done, ws_tag, drop=saved.drop,
                         recompute=saved.recompute)
    if saved.fan is not None:
        dx = ops.slice_sum(dx, *saved.fan)
    _linear_backward(dx, saved.tok, ew.patch, alpha, need_dx=False, beta=beta)
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
    saved = PredictorSaved(z=z, e_shape=e.shape, segs=segs, tsegs=tsegs, blocks=saved_blocks, t=t, tn=tn, mean=mean,
                           rstd=rstd) if save else None
    return zhat, tsegs, saved


def predictor_backward(dzhat, saved, pw: PredictorW, enc_segs, alpha: float, on_layer_done=None, beta: float = 0.0,
                       ws_tag="bwd_tmp"):
    """dzhat [sum_i B*Kp_i, D] bf16 -> returns dz [sum_i B*Ke_i, D] bf16 (gradient of the encoder output)."""
    segs, tsegs = saved.segs, saved.tsegs
    Dp = pw.embed.w.shape[0]
    n_tok = len(pw.mask_tokens)
    acc = beta != 0.0
    dtn = _linear_backward(dzhat, saved.tn, pw.proj, alpha, beta=beta)
    # the trunk's output gradient is dt on the target rows and zero on the context rows, so the last block's fc2 bias gradient
    # (column sums over ALL rows of that gradient) is the column sum of dt: it comes out of this LayerNorm backward
    dt = ops.layernorm_bwd(dtn, saved.t, pw.norm.g, saved.mean, saved.rstd, pw.norm.gg, pw.norm.gb, alpha=alpha, accumulate=acc,
                           dxsum=_fc2_gb_route(pw, len(pw.blocks) - 1, None))
    dx = torch.empty((_total_rows(segs), Dp), dtype=torch.bfloat16, device=dzhat.device)
    for sg, psg, tsg in zip(enc_segs, segs, tsegs):
        ops.copy_rows(None, _rows(dx, psg), psg.B, 0, 0, psg.S, 0, sg.S, Dp)   # context rows start at zero grad (no ATen fill on the step)
        ops.copy_rows(_rows(dt, tsg), _rows(dx, psg), psg.B, tsg.S, 0, psg.S, sg.S, tsg.S, Dp)
    if on_layer_done is not None:
        on_layer_done("pred", len(pw.blocks))
    dx = _trunk_backward(dx, saved.blocks, pw, segs, "pred", alpha, beta, on_layer_done, ws_tag)
    # token assembly backward: mask-token grads = sum of the target rows; context rows flow to predictor_embed
    de = torch.empty(saved.e_shape, dtype=torch.bfloat16, device=dzhat.device)
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
    dz = _linear_backward(de, saved.z, pw.embed, alpha, beta=beta)
    side_stream(dzhat.device).join()
    if on_layer_done is not None:
        on_layer_done("pred", -1)
    return dz
