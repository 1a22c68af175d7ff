"""Tensor-level wrapper of the still-image backward's kernel (include/vjepa_hip.h: vj_slice_sum), beside .ops: the same checks
(`ops._req`), the same tensor-to-pointer spelling (`ops._ptr`, which refuses a host tensor) and the same launch path
(`ops._launch`, which raises HipKernelError under the symbol's name).
"""
import torch

from . import ops


def slice_sum(dx, B, S, Gt, out=None, stream=None):
    """out[b, s] = bf16(sum_{t<Gt} dx[b, t*S+s]) in fp32, slice 0 first and then ascending t, one rounding; dx bf16 [B*Gt*S, D] ->
    bf16 [B*S, D].  The adjoint of ops.add_pos_bcast: the gradient of a still image's S distinct patch embeddings."""
    ops._req(dx, ops.BF16, "dx")
    ops._opt(out, ops.BF16, "out")
    D = dx.shape[-1]
    if dx.numel() != B * Gt * S * D or (out is not None and out.numel() != B * S * D):
        raise ValueError(f"slice_sum: dx {tuple(dx.shape)} / out {None if out is None else tuple(out.shape)} do not match B={B} S={S} "
                         f"Gt={Gt}")
    if out is None:
        out = torch.empty((B * S, D), dtype=ops.BF16, device=dx.device)
    ops._launch("vj_slice_sum", ops._ptr(dx), ops._ptr(out), B, S, Gt, D, stream=stream)
    return out
