"""GPU: the still-image front end of the video encoder is bit-identical to the materialised path -- vj_image_pack against
vj_tubelet_pack of the repeated clip, vj_add_pos_bcast against vj_add_pos on the repeated rows, and encoder(images) against
encoder(images.unsqueeze(2).repeat(1, 1, T, 1, 1)) for the micro model and a randomly initialised ViT-L/16 at 16 x 224 x 224."""
from functools import partial

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _repeat(images, T):
    return images.unsqueeze(2).repeat(1, 1, T, 1, 1)


def _masks(B, N, K, n, seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.stack([torch.randperm(N, generator=g)[:K].sort().values for _ in range(B)]).to(DEV) for _ in range(n)]


@pytest.mark.parametrize("B,H,W,tub,p,T", [(3, 64, 64, 2, 16, 8), (2, 48, 80, 2, 16, 4), (2, 32, 64, 4, 8, 8)])
def test_image_pack_equals_tubelet_pack_of_the_repeated_clip(B, H, W, tub, p, T):
    from jepa_amd.hip import ops
    g = torch.Generator().manual_seed(B * 1000 + H)
    images = torch.randn(B, 3, H, W, generator=g).to(DEV)
    cells, gt = (H // p) * (W // p), T // tub
    ref = ops.tubelet_pack(_repeat(images, T).contiguous(), tub, p).view(B, gt, cells, -1)
    mine = ops.image_pack(images, tub, p).view(B, cells, -1)
    for t in range(gt):
        assert torch.equal(mine, ref[:, t]), t
    # with idx: indices into the (t, h, w) grid of the repeated clip and their spatial parts name the same rows
    N, K = gt * cells, max(1, (gt * cells) // 3)
    idx = _masks(B, N, K, 1, seed=H + W)[0]
    ref_k = ops.tubelet_pack(_repeat(images, T).contiguous(), tub, p, idx=idx)
    assert torch.equal(ops.image_pack(images, tub, p, idx=(idx % cells).contiguous()), ref_k)
    assert torch.equal(ops.image_pack(images, tub, p, idx=idx), ref_k)


@pytest.mark.parametrize("B,S,Gt,D", [(2, 16, 4, 64), (3, 196, 8, 1024), (1, 15, 3, 1280), (2, 7, 1, 72)])
def test_add_pos_bcast_equals_add_pos_on_the_repeated_rows(B, S, Gt, D):
    from jepa_amd.hip import ops
    g = torch.Generator().manual_seed(S * 10 + Gt)
    y = torch.randn(B, S, D, generator=g).to(torch.bfloat16).to(DEV)
    pos = torch.randn(Gt * S, D, generator=g).to(DEV)
    ref = y.unsqueeze(1).repeat(1, Gt, 1, 1).reshape(B * Gt * S, D).contiguous()
    ops.add_pos(ref, pos, B, Gt * S)
    mine = ops.add_pos_bcast(y.view(B * S, D), pos, B, S, Gt)
    assert mine.shape == ref.shape and torch.equal(mine, ref)


def _micro():
    from jepa_amd.src.models.vision_transformer import VisionTransformer
    from tests.golden_util import load_micro, micro_weights
    enc = VisionTransformer(img_size=64, patch_size=16, num_frames=8, tubelet_size=2, embed_dim=64, depth=2, num_heads=2,
                            mlp_ratio=4, qkv_bias=True, norm_layer=partial(torch.nn.LayerNorm, eps=1e-6), uniform_power=True)
    enc.load_state_dict(micro_weights(load_micro())[0], strict=True)
    return enc


def _vit_large():
    from jepa_amd.src.models import vision_transformer as vit
    torch.manual_seed(3)
    return vit.vit_large(img_size=224, patch_size=16, num_frames=16, tubelet_size=2, uniform_power=True)


@pytest.mark.parametrize("model,B,res,T,K", [("micro", 2, 64, 8, 24), ("vit_large", 4, 224, 16, 600)])
def test_encoder_on_still_images_is_bit_identical_to_the_repeated_clip(model, B, res, T, K):
    enc = (_micro() if model == "micro" else _vit_large()).to(DEV).eval()
    for p in enc.parameters():
        p.requires_grad = False
    g = torch.Generator().manual_seed(11)
    images = torch.randn(B, 3, res, res, generator=g).to(DEV)
    masks = _masks(B, enc.num_patches, K, 2, seed=5)
    with torch.no_grad():
        ref = enc(_repeat(images, T))
        mine = enc(images)
        assert mine.shape == ref.shape == (B, enc.num_patches, enc.embed_dim) and torch.equal(mine, ref)
        assert bool(torch.isfinite(mine.float()).all()) and float(mine.float().abs().max()) > 0
        ref_m = enc(_repeat(images, T), masks)
        mine_m = enc(images, masks)
        assert mine_m.shape == ref_m.shape == (2 * B, K, enc.embed_dim) and torch.equal(mine_m, ref_m)
        one = enc(images, masks[0])                                   # a bare index tensor, as the reference accepts
        assert torch.equal(one, enc(_repeat(images, T), masks[0]))


def test_still_images_with_gradients_enabled_raise():
    enc = _micro().to(DEV)
    images = torch.randn(2, 3, 64, 64, device=DEV)
    with pytest.raises(NotImplementedError, match="frozen"):
        enc(images)
    with torch.no_grad():
        assert enc(images).shape == (2, 64, 64)
