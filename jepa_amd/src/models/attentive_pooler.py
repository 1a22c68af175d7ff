"""Attentive probe on frozen V-JEPA features with the reference's classes, constructor arguments and state-dict names
(src/models/attentive_pooler.py:21-136; CrossAttention / CrossAttentionBlock from src/models/utils/modules.py:123-181), TRAINABLE:
forward and backward run on the gfx950 kernels behind the C ABI (bf16 MFMA GEMMs with fused bias / GELU / residual epilogues,
fp32-statistics LayerNorm, transpose-free weight gradients, the few-query cross-attention of csrc/xattn.hip) inside two autograd
nodes, so `loss.backward()` + any torch optimizer of the reference's eval loop (evals/video_classification_frozen/eval.py:298-352)
work unchanged.  Features that require grad (an encoder fine-tuned through the probe, evals/video_classification_finetune) get their
gradient from the same backward: norm1's LayerNorm backward already forms it.  Parameters stay fp32 nn.Parameters (the reference's layout); every step casts the five matrices to bf16.
Any number of feature tokens: attend_across_segments feeds all segments at once (36 864 tokens for ViT-H/16-384 K400 16x8x3), and the
cross-attention runs split-key kernels where one workgroup cannot hold every score (ops.xattn_fwd / xattn_bwd pick the kernel).

What is supported is what the reference's evals instantiate: AttentiveClassifier(embed_dim, num_heads, depth=1, num_classes)
(eval.py:205-210) -- one query token, complete_block=True, no extra self-attention blocks; other settings raise.

Reference behaviours kept on purpose: CrossAttention owns a `proj` Linear that its forward never applies (modules.py:156-157), so
`xattn.proj.*` exist in the state dict, receive no gradient and do not influence the output; nn.LayerNorm default eps 1e-5.
"""
import math
import operator

import torch
import torch.nn as nn

from ...hip import ops
from ..utils.tensors import trunc_normal_
from .utils.modules import MLP


class CrossAttention(nn.Module):
    """Parameter container of modules.py:123-138 (q, kv, proj -- proj is never applied by the reference's forward)."""

    def __init__(self, dim, num_heads=12, qkv_bias=False, use_sdpa=True):
        super().__init__()
        self.num_heads = num_heads
        self.scale = (dim // num_heads) ** -0.5
        self.q = nn.Linear(dim, dim, bias=qkv_bias)
        self.kv = nn.Linear(dim, int(dim * 2), bias=qkv_bias)
        self.proj = nn.Linear(dim, dim)
        self.use_sdpa = use_sdpa


class CrossAttentionBlock(nn.Module):
    """Parameter container of modules.py:160-175 (norm1, xattn, norm2, mlp)."""

    def __init__(self, dim, num_heads, mlp_ratio=4., qkv_bias=False, act_layer=nn.GELU, norm_layer=nn.LayerNorm):
        super().__init__()
        self.norm1 = norm_layer(dim)
        self.xattn = CrossAttention(dim, num_heads=num_heads, qkv_bias=qkv_bias)
        self.norm2 = norm_layer(dim)
        self.mlp = MLP(in_features=dim, hidden_features=int(dim * mlp_ratio), act_layer=act_layer)


def _bf(t):
    return t.detach().to(torch.bfloat16).contiguous()


def _f32(t):
    return None if t is None else t.detach().float().contiguous()


def _wT(w_bf16):
    """[N_out, N_in] bf16 -> the dgrad operand W^T as a [N_in, N_out] view of the 64-padded transposed copy."""
    return ops.transpose(w_bf16)[:, :w_bf16.shape[0]]


def _zeros_like_param(p):
    return torch.zeros(p.shape, dtype=torch.float32, device=p.device)


# The lone probe's sequence around the cross-attention, shared by its two autograd nodes (_PoolerFn, _LinearFn) and the bank's one
def _tail_fwd(q1, tail, eps):
    """q1 bf16 [B, D] -> q2 = q1 + mlp(norm2(q1)) and what _tail_bwd needs; tail = (n2w, n2b, f1w, f1b, f2w, f2b)."""
    n2w, n2b, f1w, f1b, f2w, f2b = tail
    w1, w2 = _bf(f1w), _bf(f2w)
    q1n, mean2, rstd2 = ops.layernorm_fwd(q1, _f32(n2w), _f32(n2b), eps)
    dgelu = torch.empty((q1.shape[0], w1.shape[0]), dtype=torch.bfloat16, device=q1.device)
    g = ops.gemm_nt(q1n, w1, bias=_f32(f1b), aux_out=dgelu, epilogue=ops.EPI_GELU)
    q2 = ops.gemm_nt(g, w2, bias=_f32(f2b), residual=q1)
    return q2, (q1, q1n, mean2, rstd2, dgelu, g, w1, w2)


def _tail_bwd(dq2, saved, tail):
    """mlp.fc2 (+ residual), mlp.fc1 (fused GELU backward), norm2: dq1 and the gradients of `tail` in its order."""
    (q1, q1n, mean2, rstd2, dgelu, g, w1, w2), (n2w, n2b, f1w, f1b, f2w, f2b) = saved, tail
    g_f2w = ops.gemm_wgrad_tn(dq2, g, _zeros_like_param(f2w))
    g_f2b = ops.colsum(dq2, _zeros_like_param(f2b))
    du = ops.gemm_nt(dq2, _wT(w2), aux_in=dgelu, epilogue=ops.EPI_DGELU)
    g_f1w = ops.gemm_wgrad_tn(du, q1n, _zeros_like_param(f1w))
    g_f1b = ops.colsum(du, _zeros_like_param(f1b))
    dq1n = ops.gemm_nt(du, _wT(w1))
    g_n2w, g_n2b = _zeros_like_param(n2w), _zeros_like_param(n2b)
    dq1 = ops.layernorm_bwd(dq1n, q1, _f32(n2w), mean2, rstd2, g_n2w, g_n2b, dres=dq2)   # + the residual path of q1
    return dq1, (g_n2w, g_n2b, g_f1w, g_f1b, g_f2w, g_f2b)


def _head_fwd(xb, w, b):
    """nn.Linear on bf16 [R, D] rows (the classifier head, attentive_pooler.py:130-135) -> fp32 [R, C] and the padded weight: the
    classes are padded to a multiple of 64 (zero rows / zero bias), so any num_classes meets the GEMM's N % 4 and the dgrad's K % 32."""
    (C, D), Cp = w.shape, ops.pad64(w.shape[0])
    wp = torch.zeros((Cp, D), dtype=torch.bfloat16, device=xb.device)
    wp[:C] = w.detach().to(torch.bfloat16)
    bp = torch.zeros(Cp, dtype=torch.float32, device=xb.device)
    if b is not None:
        bp[:C] = b.detach().float()
    return ops.gemm_nt(xb, wp, bias=bp)[:, :C].float(), wp


def _head_bwd(dy, xb, wp, has_b=True):
    """dy [R, C] -> dx bf16 [R, D], the weight gradient [C, D] and the bias gradient [C] (None without a bias)."""
    C, (Cp, D) = dy.shape[1], wp.shape
    dl = torch.zeros((xb.shape[0], Cp), dtype=torch.bfloat16, device=xb.device)
    dl[:, :C] = dy.to(torch.bfloat16)
    gw = ops.gemm_wgrad_tn(dl, xb, torch.zeros((Cp, D), dtype=torch.float32, device=xb.device))[:C].contiguous()
    gb = ops.colsum(dl, torch.zeros(Cp, dtype=torch.float32, device=xb.device))[:C].contiguous() if has_b else None
    return ops.gemm_nt(dl, _wT(wp)), gw, gb


def _qproj_bwd(dqh1, q0, wq, qw, g_qt):
    """q = Linear(q0), dqh1 bf16 [1, D]: returns g_qw (the outer product dqh^T q0) and adds the path through Wq^T into g_qt."""
    g_qw = ops.gemm_wgrad_tn(dqh1, q0, _zeros_like_param(qw))
    ops.colsum(ops.gemm_nt(dqh1, _wT(wq)), g_qt, accumulate=True)
    return g_qw


def _probe_params(pooler, head=()):
    """A probe's parameter tensors in _PoolerFn.NAMES order, then those of its linear head where the caller has one."""
    blk = pooler.cross_attention_block
    return [pooler.query_tokens, *(operator.attrgetter(n)(blk) for n in _PoolerFn.NAMES[1:]), *head]


class _PoolerFn(torch.autograd.Function):
    """AttentivePooler.forward (attentive_pooler.py:96-102) for one query token:  q0 -> q0 + xattn(q0, norm1(x)) -> + mlp(norm2(.))."""

    NAMES = ("query_tokens", "norm1.weight", "norm1.bias", "xattn.q.weight", "xattn.q.bias", "xattn.kv.weight", "xattn.kv.bias",
             "norm2.weight", "norm2.bias", "mlp.fc1.weight", "mlp.fc1.bias", "mlp.fc2.weight", "mlp.fc2.bias")

    @staticmethod
    def forward(ctx, x, heads, eps, *params):
        qt, n1w, n1b, qw, qb, kvw, kvb = params[:7]
        B, N, D = x.shape
        hd = D // heads
        x2 = x.detach().reshape(B * N, D).to(torch.bfloat16).contiguous()
        q0 = _bf(qt).reshape(1, D)
        wq, wkv = _bf(qw), _bf(kvw)
        qh = ops.gemm_nt(q0, wq, bias=_f32(qb))                                                 # [1, D]: the same row for every sample
        xn, mean1, rstd1 = ops.layernorm_fwd(x2, _f32(n1w), _f32(n1b), eps)
        kv = ops.gemm_nt(xn, wkv, bias=_f32(kvb))                                              # packed [B, N, 2, H, hd]
        q1, lse = ops.xattn_fwd(qh, kv, B, 1, N, heads, hd, hd ** -0.5, resid=q0, shared_q=True)   # q0 + softmax(q k^T) v
        q2, tail = _tail_fwd(q1, params[7:], eps)
        ctx.saved = (x2, xn, mean1, rstd1, kv, qh, q0, lse, wq, wkv, tail)
        ctx.meta = (B, N, D, heads, hd, eps)
        ctx.params = params
        ctx.x_like = (x.shape, x.dtype)
        return q2.float().view(B, 1, D)

    @staticmethod
    def backward(ctx, dout):
        x2, xn, mean1, rstd1, kv, qh, q0, lse, wq, wkv, tail = ctx.saved
        B, N, D, heads, hd, eps = ctx.meta
        qt, n1w, n1b, qw, qb, kvw, kvb = ctx.params[:7]
        dev = x2.device
        with torch.no_grad():
            dq2 = dout.reshape(B, D).to(torch.bfloat16).contiguous()
            dq1, g_tail = _tail_bwd(dq2, tail, ctx.params[7:])
            # q1 = q0 + y: the query token collects the batch sum; y goes back through the cross-attention
            g_qt = ops.colsum(dq1, torch.zeros(D, dtype=torch.float32, device=dev))
            dqh, dkv = ops.xattn_bwd(qh, kv, dq1, lse, B, N, heads, hd, hd ** -0.5, shared_q=True)
            g_qb = ops.colsum(dqh, torch.zeros(D, dtype=torch.float32, device=dev))              # the projected query is shared: batch sum
            dqh1 = torch.empty((1, D), dtype=torch.bfloat16, device=dev)
            ops.cast_bf16(g_qb, dqh1.view(-1))
            g_qw = _qproj_bwd(dqh1, q0, wq, qw, g_qt)
            # kv = Linear(norm1(x)): weight / bias gradients, then norm1's affine parameters and, from the same launch, dx: x reaches
            # the output through norm1 -> kv only, so this is its whole gradient (kept only where x asks for one: fine-tuning)
            g_kvw = ops.gemm_wgrad_tn(dkv, xn, _zeros_like_param(kvw))
            g_kvb = ops.colsum(dkv, _zeros_like_param(kvb))
            dxn = ops.gemm_nt(dkv, _wT(wkv))
            g_n1w, g_n1b = _zeros_like_param(n1w), _zeros_like_param(n1b)
            dx = ops.layernorm_bwd(dxn, x2, _f32(n1w), mean1, rstd1, g_n1w, g_n1b)
            dx = dx.view(ctx.x_like[0]).to(ctx.x_like[1]) if ctx.needs_input_grad[0] else None
        return (dx, None, None, g_qt.view_as(qt), g_n1w, g_n1b, g_qw, None if qb is None else g_qb, g_kvw,
                None if kvb is None else g_kvb, *g_tail)


class _LinearFn(torch.autograd.Function):
    """nn.Linear on [B, D] rows: _head_fwd / _head_bwd as an autograd node of its own."""

    @staticmethod
    def forward(ctx, x, w, b):
        xb = x.detach().reshape(-1, w.shape[1]).to(torch.bfloat16).contiguous()
        y, wp = _head_fwd(xb, w, b)
        ctx.saved = (xb, wp, x.shape, b is not None)
        return y.reshape(*x.shape[:-1], w.shape[0])

    @staticmethod
    def backward(ctx, dy):
        xb, wp, xshape, has_b = ctx.saved
        with torch.no_grad():
            dx, gw, gb = _head_bwd(dy.reshape(xb.shape[0], -1), xb, wp, has_b)
        return dx.float().reshape(xshape), gw, gb


class AttentivePooler(nn.Module):
    """ Attentive Pooler (attentive_pooler.py:21-102) """

    def __init__(self, num_queries=1, embed_dim=768, num_heads=12, mlp_ratio=4.0, depth=1, norm_layer=nn.LayerNorm,
                 init_std=0.02, qkv_bias=True, complete_block=True):
        super().__init__()
        if num_queries != 1 or depth != 1 or not complete_block:
            raise NotImplementedError(
                "jepa_amd builds the probe the reference's evals instantiate: num_queries=1, depth=1, complete_block=True "
                "(evals/video_classification_frozen/eval.py:205-210)")
        if embed_dim % 32 != 0 or (embed_dim // num_heads) % 8 != 0 or embed_dim // num_heads > 128:
            raise NotImplementedError("embed_dim must be a multiple of 32 and head_dim a multiple of 8, at most 128")
        self.query_tokens = nn.Parameter(torch.zeros(1, num_queries, embed_dim))
        self.complete_block = complete_block
        self.cross_attention_block = CrossAttentionBlock(dim=embed_dim, num_heads=num_heads, mlp_ratio=mlp_ratio,
                                                         qkv_bias=qkv_bias, norm_layer=norm_layer)
        self.blocks = None
        self.init_std = init_std
        trunc_normal_(self.query_tokens, std=self.init_std)
        self.apply(self._init_weights)
        self._rescale_blocks()

    def _rescale_blocks(self):
        # attentive_pooler.py:68-81 with layer_id = 1: proj (never applied, but rescaled all the same) and fc2 / sqrt(2)
        self.cross_attention_block.xattn.proj.weight.data.div_(math.sqrt(2.0))
        self.cross_attention_block.mlp.fc2.weight.data.div_(math.sqrt(2.0))

    def _init_weights(self, m):
        if isinstance(m, nn.Linear):
            trunc_normal_(m.weight, std=self.init_std)
            if m.bias is not None:
                nn.init.constant_(m.bias, 0)
        elif isinstance(m, nn.LayerNorm):
            nn.init.constant_(m.bias, 0)
            nn.init.constant_(m.weight, 1.0)

    def forward(self, x):
        """x: [B, N, D] encoder tokens (any float dtype, GPU) -> [B, 1, D] fp32.  Where x requires grad (an encoder that is being
        fine-tuned), the backward also returns its gradient, in x's shape and dtype."""
        if not x.is_cuda:
            raise ValueError("AttentivePooler: jepa_amd computes only on the GPU through libvjepa_hip.so (no CPU fallback)")
        blk = self.cross_attention_block
        return _PoolerFn.apply(x, blk.xattn.num_heads, blk.norm1.eps, *_probe_params(self))


def _spread_heads(v, H):
    """v [R, H*hd] -> [R*H, H*hd]: row (r, h) keeps head h's slice of v[r] and zeros elsewhere, so that one GEMM against a [D, D]
    weight applies each head's own block of it."""
    R, D = v.shape
    out = torch.zeros((R, H, H, D // H), dtype=v.dtype, device=v.device)
    i = torch.arange(H, device=v.device)
    out[:, i, i] = v.view(R, H, D // H)
    return out.view(R * H, D)


def _pick_heads(m, H):
    """m [R*H, H*hd] -> [R, H*hd]: head h's slice of row (r, h) -- the block diagonal of what _spread_heads spreads."""
    R, D = m.shape[0] // H, m.shape[1]
    return m.view(R, H, H, D // H).diagonal(dim1=1, dim2=2).permute(0, 2, 1).reshape(R, D)


class _BankFn(torch.autograd.Function):
    """P attentive classifiers on ONE pass over the frozen features.  Each probe has one query token shared by the batch, so with
    x_hat = LayerNorm(x) without affine, q = Wq q0 + bq, t_h = Wk_h^T q_h and u_h = scale * gamma * t_h:
        scores  S[b,n,(p,h)] = x_hat[b,n] . u_h       (norm1.bias and the key bias shift every key alike: the soft-max drops them)
        A = softmax over n,   Z[b,(p,h)] = sum_n A x_hat[b,n],   y[b,h] = Wv_h (gamma * Z + beta) + bv_h
    which is CrossAttention.forward (modules.py:140-157) on norm1(x) without K or V: two GEMM-shaped passes over x_hat forward
    (scores, pooling) and two backward (dA, dU), all probes' heads as columns.  The tail (q0 + y, norm2, MLP, linear) runs per probe
    on the lone probe's kernels.  The key half of kv.bias cannot influence the output: its gradient is exactly zero."""

    PER = 15   # tensors per probe: _PoolerFn.NAMES + linear.weight, linear.bias

    @staticmethod
    def forward(ctx, x, heads, eps, P, *params):
        B, N, D = x.shape
        H, hd, dev = heads, D // heads, x.device
        s = hd ** -0.5
        C = ops.pad64(P * H)                                        # zero rows of U: uniform columns nothing reads
        x2 = x.detach().reshape(B * N, D).to(torch.bfloat16).contiguous()
        xh, _, _ = ops.layernorm_fwd(x2, torch.ones(D, dtype=torch.float32, device=dev),
                                     torch.zeros(D, dtype=torch.float32, device=dev), eps, save_stats=False)
        del x2
        U = torch.zeros((C, D), dtype=torch.bfloat16, device=dev)
        pre = []
        for p in range(P):
            qt, n1w, n1b, qw, qb, kvw, kvb = params[p * _BankFn.PER:p * _BankFn.PER + 7]
            q0 = _bf(qt).reshape(1, D)
            wq, wkv = _bf(qw), _bf(kvw)
            qh = ops.gemm_nt(q0, wq, bias=_f32(qb))                                             # [1, D]
            qblk = _spread_heads(qh, H)                                                         # [H, D]
            t = ops.gemm_nt(qblk, _wT(wkv[:D]), epilogue=ops.EPI_F32)                           # t_h = Wk_h^T q_h, fp32 [H, D]
            U[p * H:(p + 1) * H] = (s * n1w.detach().float() * t).to(torch.bfloat16)
            pre.append((q0, wq, wkv, qblk, t))
        S = ops.gemm_nt(xh, U, epilogue=ops.EPI_F32).view(B, N, C)
        A, _ = ops.pool_softmax_fwd(S)
        del S
        Z = torch.empty((B, C, D), dtype=torch.float32, device=dev)
        for b in range(B):
            ops.gemm_wgrad_tn(A[b], xh[b * N:(b + 1) * N], Z[b])                                # Z[b] = A[b]^T x_hat[b]
        logits, saved = [], []
        for p in range(P):
            pp = params[p * _BankFn.PER:(p + 1) * _BankFn.PER]
            (qt, n1w, n1b, qw, qb, kvw, kvb), (q0, wq, wkv, qblk, t) = pp[:7], pre[p]
            R = (n1w.detach().float() * Z[:, p * H:(p + 1) * H] + n1b.detach().float()).to(torch.bfloat16).reshape(B * H, D)
            y = _pick_heads(ops.gemm_nt(R, wkv[D:], epilogue=ops.EPI_F32), H)                   # y[b,h] = Wv_h R[b,h]
            if kvb is not None:
                y = y + kvb.detach().float()[D:]
            q1 = (y + q0.float()).to(torch.bfloat16)                                            # q0 + xattn(q0, norm1(x))
            q2, tail = _tail_fwd(q1, pp[7:13], eps)
            lg, lwp = _head_fwd(q2, pp[13], pp[14])
            logits.append(lg)
            saved.append((q0, wq, wkv, qblk, t, R, tail, q2, lwp))
        ctx.saved = (xh, A, Z, saved)
        ctx.meta = (B, N, D, H, hd, eps, P, C)
        ctx.params = params
        return torch.stack(logits)

    @staticmethod
    def backward(ctx, dlogits):
        (xh, A, Z, saved), params = ctx.saved, ctx.params
        B, N, D, H, hd, eps, P, C = ctx.meta
        s, dev = hd ** -0.5, xh.device
        grads = [None] * (P * _BankFn.PER)
        zf = lambda *shape: torch.zeros(shape, dtype=torch.float32, device=dev)   # noqa: E731
        with torch.no_grad():
            dZ = zf(B, C, D)
            for p in range(P):
                pp = params[p * _BankFn.PER:(p + 1) * _BankFn.PER]
                (qt, n1w, n1b, qw, qb, kvw, kvb), (q0, wq, wkv, qblk, t, R, tail, q2, lwp) = pp[:7], saved[p]
                dq2, g_lw, g_lb = _head_bwd(dlogits[p], q2, lwp)
                dq1, g_tail = _tail_bwd(dq2, tail, pp[7:13])
                g_qt = ops.colsum(dq1, zf(D))
                # value path: y[b,h] = Wv_h R[b,h] + bv_h, R = gamma * Z + beta
                g_kvw = _zeros_like_param(kvw)
                g_kvb = None if kvb is None else _zeros_like_param(kvb)                          # the key half stays exactly zero
                if kvb is not None:
                    ops.colsum(dq1, g_kvb[D:])
                dyblk = _spread_heads(dq1, H)                                                    # [B*H, D]
                ops.gemm_wgrad_tn(dyblk, R, g_kvw[D:])                                           # dWv_h = sum_b dy_h R_h^T
                G = ops.gemm_nt(dyblk, _wT(wkv[D:]), epilogue=ops.EPI_F32).view(B, H, D)         # G = Wv_h^T dy_h
                g_n1b = G.sum(dim=(0, 1))
                g_n1w = (G * Z[:, p * H:(p + 1) * H]).sum(dim=(0, 1))
                dZ[:, p * H:(p + 1) * H] = n1w.detach().float() * G
                grads[p * _BankFn.PER:(p + 1) * _BankFn.PER] = [g_qt, g_n1w, g_n1b, None, None, g_kvw, g_kvb, *g_tail, g_lw, g_lb]
            # score path, every probe's heads at once: dA = x_hat . dZ, dS = A (dA - delta), dU = dS^T x_hat
            dZb = dZ.to(torch.bfloat16)
            dA = torch.empty((B, N, C), dtype=torch.float32, device=dev)
            for b in range(B):
                ops.gemm_nt(xh[b * N:(b + 1) * N], dZb[b], out=dA[b], epilogue=ops.EPI_F32)
            delta = (dZ * Z).sum(dim=-1)
            dS = ops.pool_softmax_bwd(A, dA, delta)
            del dA
            dU = ops.gemm_wgrad_tn(dS.view(B * N, C), xh, zf(C, D))
            for p in range(P):
                qt, n1w, n1b, qw, qb, kvw, kvb = params[p * _BankFn.PER:p * _BankFn.PER + 7]
                q0, wq, wkv, qblk, t = saved[p][:5]
                o = p * _BankFn.PER
                dUp = dU[p * H:(p + 1) * H]
                grads[o + 1] += (dUp * t).sum(dim=0) * s                                         # u_h = scale * gamma * t_h
                e = (s * n1w.detach().float() * dUp).to(torch.bfloat16)                          # d t_h, [H, D]
                ops.gemm_wgrad_tn(qblk, e, grads[o + 5][:D])                                     # dWk_h = q_h e_h^T
                dq = _pick_heads(ops.gemm_nt(e, wkv[:D], epilogue=ops.EPI_F32), H)               # dq_h = Wk_h e_h, [1, D]
                if qb is not None:
                    grads[o + 4] = dq.reshape(D).clone()
                grads[o + 3] = _qproj_bwd(dq.to(torch.bfloat16), q0, wq, qw, grads[o])
                grads[o] = grads[o].view_as(qt)
        return (None, None, None, None, *grads)


class AttentiveClassifierBank(nn.Module):
    """A bank of `num_probes` AttentiveClassifier heads trained at once on one frozen forward pass: the grid of probe learning
    rates / weight decays of a frozen evaluation costs one encoder pass per iteration instead of one per grid point.  The
    parameters live in `.probes` (an nn.ModuleList of the lone classifier, the reference's names under `probes.{p}.`), built in
    index order from the global generator: probe 0 equals a lone AttentiveClassifier built under the same seed.

    forward(x [B, N, D]) -> logits fp32 [P, B, num_classes] through ONE autograd node over all probes' parameters (_BankFn); the
    probes share no parameter, so the backward of the summed per-probe losses gives each probe its own gradient.  The key half
    of every `xattn.kv.bias` receives an exactly-zero gradient (it cannot influence the output) and stays where it was initialised."""

    def __init__(self, embed_dim=768, num_heads=12, num_classes=1000, num_probes=1, mlp_ratio=4.0, init_std=0.02, qkv_bias=True):
        super().__init__()
        if num_probes < 1:
            raise ValueError("AttentiveClassifierBank: num_probes must be at least 1")
        self.num_heads = num_heads
        self.probes = nn.ModuleList([
            AttentiveClassifier(embed_dim=embed_dim, num_heads=num_heads, mlp_ratio=mlp_ratio, depth=1, init_std=init_std,
                                qkv_bias=qkv_bias, num_classes=num_classes) for _ in range(num_probes)])

    def probe_state_dict(self, p):
        """The reference-format state dict of probe p: loads strictly into a lone AttentiveClassifier (here or the reference's)."""
        return self.probes[p].state_dict()

    def forward(self, x):
        if not x.is_cuda:
            raise ValueError("AttentiveClassifierBank: jepa_amd computes only on the GPU through libvjepa_hip.so (no CPU fallback)")
        if x.requires_grad and torch.is_grad_enabled():
            raise NotImplementedError("AttentiveClassifierBank: the features come from a FROZEN encoder (eval.py:330-337 runs it "
                                      "under torch.no_grad()); no gradient is propagated into them -- a bank of probes over one "
                                      "trainable encoder is not a protocol (fine-tuning takes the lone AttentiveClassifier)")
        flat = [t for m in self.probes for t in _probe_params(m.pooler, (m.linear.weight, m.linear.bias))]
        return _BankFn.apply(x, self.num_heads, self.probes[0].pooler.cross_attention_block.norm1.eps, len(self.probes), *flat)


class AttentiveClassifier(nn.Module):
    """ Attentive Classifier (attentive_pooler.py:105-136) """

    def __init__(self, embed_dim=768, num_heads=12, mlp_ratio=4.0, depth=1, norm_layer=nn.LayerNorm, init_std=0.02,
                 qkv_bias=True, num_classes=1000, complete_block=True):
        super().__init__()
        self.pooler = AttentivePooler(num_queries=1, embed_dim=embed_dim, num_heads=num_heads, mlp_ratio=mlp_ratio, depth=depth,
                                      norm_layer=norm_layer, init_std=init_std, qkv_bias=qkv_bias, complete_block=complete_block)
        self.linear = nn.Linear(embed_dim, num_classes, bias=True)

    def forward(self, x):
        x = self.pooler(x).squeeze(1)
        return _LinearFn.apply(x, self.linear.weight, self.linear.bias)
