"""Clip aggregation of the frozen video-classification eval (evals/video_classification_frozen/utils.py:22-159).

ClipAggregation keeps the reference's constructor, attributes and forward contract: the input is a list over segments of lists
over views of [B,C,T,H,W] clips; the output is a list over views of [B, S*N, D] (attend_across_segments) or a list over views of
lists over segments of [B, N, D].  The frozen encoder runs on every clip in the reference's order (segment-major, then view, then
sample) and the per-view concatenation is written by the bit-exact row copy (vj_copy_rows) straight into one bf16 buffer per
view.  The reference's video transforms (make_transforms and the decord loader behind them) are not part of this package.
"""
import torch
import torch.nn as nn

from ...hip import ops


def max_clips_per_call(width, tokens_per_clip):
    """Clips per encoder call that keep the widest activation (M token rows x `width` columns: fc1's output) below 2^31
    elements."""
    return max(1, (2 ** 31 - 1) // (width * tokens_per_clip))


def _widest(model):
    """Widest activation row of the encoder: fc1's output features (4 D for L / H, 48/11 D for ViT-g), at least 3 D (qkv)."""
    blocks = getattr(model, "blocks", None)
    fc1 = blocks[0].mlp.fc1.out_features if blocks is not None and len(blocks) else 4 * model.embed_dim
    return max(fc1, 3 * model.embed_dim)


class FrameAggregation(nn.Module):
    """Image encoders (evals/video_classification_frozen/utils.py:22-81): not supported, as image ViTs are not."""

    def __init__(self, model, max_frames=10000, use_pos_embed=False, attend_across_segments=False):
        raise NotImplementedError("FrameAggregation runs an image (num_frames=1) encoder frame by frame; image ViTs are "
                                  "outside this package (see jepa_amd/src/models/vision_transformer.py)")


class ClipAggregation(nn.Module):
    """Process each clip independently and concatenate all tokens (utils.py:84-159)."""

    def __init__(self, model, tubelet_size=2, max_frames=10000, use_pos_embed=False, attend_across_segments=False):
        super().__init__()
        self.model = model
        self.tubelet_size = tubelet_size
        self.embed_dim = model.embed_dim
        self.num_heads = model.num_heads
        self.attend_across_segments = attend_across_segments
        if use_pos_embed:
            raise NotImplementedError("ClipAggregation(use_pos_embed=True): the temporal position embedding is not "
                                      "implemented; no shipped eval config sets it (eval.py:172-176)")
        self.pos_embed = None
        # encoder call size: fc1's output of one call stays below 2^31 elements (91 clips for ViT-H/16 at 384)
        self.max_clips_per_call = max_clips_per_call(_widest(model), model.num_patches)

    def _features(self, x):
        """x: [S*V*B, C, T, H, W] -> list of (first clip, bf16 [m, N, D]) over encoder calls of at most max_clips_per_call."""
        out, M = [], x.shape[0]
        for c0 in range(0, M, self.max_clips_per_call):
            f = self.model(x[c0:c0 + self.max_clips_per_call])
            out.append((c0, f if f.dtype == torch.bfloat16 else f.to(torch.bfloat16)))
        return out

    def forward(self, x, clip_indices=None):
        num_clips = len(x)
        num_views_per_clip = len(x[0])
        B = x[0][0].shape[0]
        eff_B = B * num_views_per_clip
        # all spatial and temporal views along the batch dimension, in the reference's order
        feats = self._features(torch.cat([torch.cat(xi, dim=0) for xi in x], dim=0))
        N, D = feats[0][1].shape[1], feats[0][1].shape[2]
        if not self.attend_across_segments:
            if len(feats) == 1:
                f = feats[0][1]
                return [[f[i * eff_B + j * B:i * eff_B + (j + 1) * B] for i in range(num_clips)] for j in range(num_views_per_clip)]
            allf = torch.empty((num_clips * eff_B, N, D), dtype=torch.bfloat16, device=feats[0][1].device)
            for c0, f in feats:
                ops.copy_rows(f, allf, 1, f.shape[0] * N, 0, allf.shape[0] * N, c0 * N, f.shape[0] * N, D)
            return [[allf[i * eff_B + j * B:i * eff_B + (j + 1) * B] for i in range(num_clips)] for j in range(num_views_per_clip)]
        # segment i of view j of sample b is clip i*eff_B + j*B + b; its tokens go to rows [i*N, (i+1)*N) of sample b of view j
        outs = [torch.empty((B, num_clips * N, D), dtype=torch.bfloat16, device=feats[0][1].device)
                for _ in range(num_views_per_clip)]
        for c0, f in feats:
            k, m = 0, f.shape[0]
            while k < m:   # runs of consecutive clips of one (segment, view)
                g = c0 + k
                i, j, b = g // eff_B, (g % eff_B) // B, g % B
                n = min(B - b, m - k)
                ops.copy_rows(f[k:k + n], outs[j][b:b + n], n, N, 0, num_clips * N, i * N, N, D)
                k += n
        return outs
