"""Inputs and model of tests/golden/image_vit_micro.npz, regenerated from the recorded seeds on the CPU (imported, never collected).
The layout and order are those of tools/make_golden_image_vit.py; the fixture's sha256 values pin them."""
import hashlib
import os
from functools import partial

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def fixture():
    return np.load(os.path.join(GOLDEN, "image_vit_micro.npz"))


def _check(sha256, *tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.contiguous().numpy().tobytes())
    assert np.array_equal(np.frombuffer(h.digest(), dtype=np.uint8), np.asarray(sha256)), "image_vit_micro inputs do not regenerate"


def micro_image_vit(z, load=True):
    """The micro image ViT of the fixture (img_size 32, patch 8, D 64, depth 2, 2 heads, eps 1e-6), on the CPU."""
    from jepa_amd.src.models.vision_transformer import VisionTransformer
    B, img, patch, dim, depth, heads, keep = (int(x) for x in z["dims"])
    enc = VisionTransformer(img_size=img, patch_size=patch, num_frames=1, embed_dim=dim, depth=depth, num_heads=heads, mlp_ratio=4,
                            qkv_bias=True, norm_layer=partial(torch.nn.LayerNorm, eps=1e-6))
    if load:
        enc.load_state_dict({str(k): torch.from_numpy(z["w/" + str(k)]) for k in z["keys"]}, strict=True)
    enc.eval()
    for p in enc.parameters():
        p.requires_grad = False
    return enc


def micro_images(z, size):
    """(images [B, 3, size, size], mask [B, keep] sorted int64 token indices of the image's grid)."""
    B, img, patch, dim, depth, heads, keep = (int(x) for x in z["dims"])
    g = torch.Generator().manual_seed(int(z["image_seed"]) + size)
    images = torch.randn(B, 3, size, size, generator=g)
    n = (size // patch) ** 2
    mask = torch.stack([torch.randperm(n, generator=g)[:min(keep, n)].sort().values for _ in range(B)])
    _check(z[f"sha256/{size}x{size}"], images, mask)
    return images, mask


def micro_frames(z):
    """(clips: [S] of [V] of [B, 3, T, 32, 32]; clip_indices: [S] of int64 [B, T])."""
    B, img = int(z["dims"][0]), int(z["dims"][1])
    S, V, T, max_frames = (int(x) for x in z["agg_dims"])
    g = torch.Generator().manual_seed(int(z["frame_seed"]))
    clips = [[torch.randn(B, 3, T, img, img, generator=g) for _ in range(V)] for _ in range(S)]
    indices = [torch.randint(0, max_frames, (B, T), generator=g) for _ in range(S)]
    _check(z["frames_sha256"], *[c for seg in clips for c in seg], *indices)
    assert np.array_equal(torch.stack(indices).numpy(), z["clip_indices"])
    return clips, indices
