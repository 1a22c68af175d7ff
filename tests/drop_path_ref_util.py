"""The fp32 reference of stochastic depth: oracle.vjepa_oracle.block / encoder_forward restated with the two per-sample scales of
every block, x + s[:, None, None] * branch(x), from the oracle's own helpers (patchify) and the torch functions it calls, in its
order of operations.  With every scale equal to 1 the products are exact and the result is the oracle's encoder_forward bit for bit
(tests/test_drop_path_host.py).  Shared by the host and the GPU tests; nothing here touches a GPU."""
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import vjepa_oracle as O  # noqa: E402


def block(x, w, pre, heads, s_attn, s_mlp, eps=1e-6):
    """O.block (fp32, emu=False) with the attention branch scaled by s_attn [B] and the MLP branch by s_mlp [B]."""
    B, S, D = x.shape
    y = F.layer_norm(x, (D,), w[pre + "norm1.weight"], w[pre + "norm1.bias"], eps)
    qkv = F.linear(y, w[pre + "attn.qkv.weight"], w[pre + "attn.qkv.bias"])
    q, k, v = qkv.reshape(B, S, 3, heads, D // heads).permute(2, 0, 3, 1, 4)
    att = F.scaled_dot_product_attention(q, k, v)
    att = att.transpose(1, 2).reshape(B, S, D)
    x = x + s_attn[:, None, None] * F.linear(att, w[pre + "attn.proj.weight"], w[pre + "attn.proj.bias"])
    y = F.layer_norm(x, (D,), w[pre + "norm2.weight"], w[pre + "norm2.bias"], eps)
    y = F.gelu(F.linear(y, w[pre + "mlp.fc1.weight"], w[pre + "mlp.fc1.bias"]))
    return x + s_mlp[:, None, None] * F.linear(y, w[pre + "mlp.fc2.weight"], w[pre + "mlp.fc2.bias"])


def encoder_forward(w, clips, cfg, scales):
    """O.encoder_forward (fp32, masks=None) with scales fp32 [depth, 2, B]: scales[i, 0] on the attention branch of block i,
    scales[i, 1] on its MLP branch.  Returns [B, N, D] after the final norm."""
    D = cfg["embed_dim"]
    tok = O.patchify(clips, cfg["tubelet"], cfg["patch"])
    x = tok @ w["patch_embed.proj.weight"].reshape(D, -1).t() + w["patch_embed.proj.bias"]
    x = x + w["pos_embed"]
    for i in range(cfg["depth"]):
        x = block(x, w, f"blocks.{i}.", cfg["heads"], scales[i, 0], scales[i, 1])
    return F.layer_norm(x, (D,), w["norm.weight"], w["norm.bias"], 1e-6)

