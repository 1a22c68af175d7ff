"""GPU: vj_pos_interp3d and the encoder at off-native input sizes, against tests/golden/image_eval_micro.npz (the reference's
interpolate_pos_encoding and encoder features, tools/make_golden_image_eval.py) and against F.interpolate on the CPU for the
ViT-L/16 and ViT-H/16-384 tables."""
import os
from functools import partial

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TABLE_TOL = 1e-5     # the project's fp32 tolerance against a fixture: 8 table values in [-1, 1], seven fp32 lerps, coordinates < 32
FEATURE_TOL = 2e-2   # rel-L2, the project's feature bound


def rel_l2(a, b):
    a, b = torch.as_tensor(a).detach().float().cpu().reshape(-1), torch.as_tensor(b).detach().float().cpu().reshape(-1)
    return float((a - b).norm() / (b.norm() + 1e-12))


def _fixture():
    return np.load(os.path.join(GOLDEN, "image_eval_micro.npz"))


def _micro(frozen=True):
    from jepa_amd.src.models.vision_transformer import VisionTransformer
    from tests.golden_util import load_micro, micro_weights
    enc = VisionTransformer(img_size=64, patch_size=16, num_frames=8, tubelet_size=2, embed_dim=64, depth=2, num_heads=2,
                            mlp_ratio=4, qkv_bias=True, norm_layer=partial(torch.nn.LayerNorm, eps=1e-6), uniform_power=True)
    enc.load_state_dict(micro_weights(load_micro())[0], strict=True)
    enc.to(DEV).eval()
    if frozen:
        for p in enc.parameters():
            p.requires_grad = False
    return enc


def _sizes(z):
    return [tuple(int(s) for s in sz) for sz in z["sizes"]]


def test_interpolated_tables_match_the_reference():
    z = _fixture()
    enc = _micro()
    sizes = _sizes(z)
    assert {(8, 96, 96), (16, 64, 64), (4, 32, 32), (12, 80, 48)} <= set(sizes)
    for t, h, w in sizes:
        ref = torch.from_numpy(z[f"interp/{t}x{h}x{w}"])
        tab = enc.interpolate_pos_encoding(torch.empty(1, 3, t, h, w, device=DEV), enc.pos_embed)
        assert tab.dtype == torch.float32 and tuple(tab.shape) == (1,) + tuple(ref.shape), (t, h, w, tab.shape)
        err = float((tab[0].cpu() - ref).abs().max())
        print(f"pos_interp {t}x{h}x{w}: max abs err {err:.3e}")
        assert err <= TABLE_TOL, (t, h, w, err)


def test_native_size_returns_the_parameter_and_tables_are_cached_until_reload():
    enc = _micro()
    assert enc.interpolate_pos_encoding(torch.empty(1, 3, 8, 64, 64, device=DEV), enc.pos_embed) is enc.pos_embed
    x = torch.empty(1, 3, 8, 96, 96, device=DEV)
    t1 = enc.interpolate_pos_encoding(x, enc.pos_embed)
    assert enc.interpolate_pos_encoding(x, enc.pos_embed) is t1                      # one computation per (T, H, W)
    other = enc.interpolate_pos_encoding(torch.empty(1, 3, 16, 64, 64, device=DEV), enc.pos_embed)
    assert other.shape == (1, 128, 64) and enc.interpolate_pos_encoding(x, enc.pos_embed) is t1
    sd = {k: v.clone() for k, v in enc.state_dict().items()}
    sd["pos_embed"] = sd["pos_embed"] * 0.5
    enc.load_state_dict(sd)                                                           # a reloaded table invalidates the cache
    t2 = enc.interpolate_pos_encoding(x, enc.pos_embed)
    assert t2 is not t1 and torch.allclose(t2, 0.5 * t1, atol=1e-6)
    enc.to("cpu").to(DEV)                                                             # so does moving the module
    t3 = enc.interpolate_pos_encoding(x, enc.pos_embed)
    assert t3 is not t2 and torch.equal(t3, t2)


@pytest.mark.parametrize("name,D,src,dst", [("vit_large_16x384", 1024, (8, 14, 14), (8, 24, 24)),
                                            ("vit_huge_384_to_224", 1280, (8, 24, 24), (8, 14, 14)),
                                            ("vit_huge_384_32_frames", 1280, (8, 24, 24), (16, 24, 24))])
def test_full_size_tables_against_f_interpolate(name, D, src, dst):
    from jepa_amd.hip import ops
    from jepa_amd.src.models.utils.pos_embs import get_3d_sincos_pos_embed
    Nt, Nh, Nw = src
    table = torch.from_numpy(get_3d_sincos_pos_embed(D, Nh, Nt, cls_token=False, uniform_power=True)).float()
    assert table.shape == (Nt * Nh * Nw, D)
    scale = (dst[0] / Nt, dst[1] / Nh, dst[2] / Nw)                     # as interpolate_pos_encoding computes them
    ref = F.interpolate(table.reshape(1, Nt, Nh, Nw, D).permute(0, 4, 1, 2, 3), scale_factor=scale, mode='trilinear')
    ref = ref.permute(0, 2, 3, 4, 1)[0]
    out = ops.pos_interp3d(table.view(Nt, Nh, Nw, D).to(DEV), scale)
    assert tuple(out.shape) == tuple(ref.shape) == dst + (D,)
    err = float((out.cpu() - ref).abs().max())
    print(f"pos_interp {name}: max abs err {err:.3e}")
    assert err <= TABLE_TOL, (name, err)


def test_encoder_features_at_off_native_sizes_match_the_reference():
    """One encoder called at every recorded size in turn (and at the native size in between): the inference workspace follows the
    row count of each launch.  The 8-token 4 x 32 x 32 clip is shorter than any sequence of the attention tests."""
    from tests.image_eval_golden_util import off_native_clips
    z = _fixture()
    enc = _micro()
    native = torch.randn(2, 3, 8, 64, 64, generator=torch.Generator().manual_seed(1)).to(DEV)
    with torch.no_grad():
        base = enc(native)
        for rnd in range(2):
            for t, h, w in _sizes(z):
                clips, mask = off_native_clips(z, (t, h, w))
                ref = z[f"off/{t}x{h}x{w}"]
                out = enc(clips.to(DEV))
                assert tuple(out.shape) == ref.shape
                e = rel_l2(out, ref)
                print(f"off-native features {t}x{h}x{w} ({ref.shape[1]} tokens): rel-L2 {e:.3e}")
                assert e <= FEATURE_TOL, (t, h, w, e)
                key = f"off_masked/{t}x{h}x{w}"
                if key in z.files:
                    assert np.array_equal(z[f"off_mask/{t}x{h}x{w}"], mask.numpy())
                    out_m = enc(clips.to(DEV), [mask.to(DEV)])
                    assert tuple(out_m.shape) == z[key].shape
                    e = rel_l2(out_m, z[key])
                    print(f"off-native masked features {t}x{h}x{w}: rel-L2 {e:.3e}")
                    assert e <= FEATURE_TOL, (t, h, w, "masked", e)
            assert torch.equal(enc(native), base)
    assert "off_masked/12x80x48" in z.files


def test_off_native_input_with_gradients_enabled_raises():
    enc = _micro(frozen=False)
    clips = torch.randn(1, 3, 8, 96, 96, device=DEV)
    with pytest.raises(NotImplementedError, match="frozen"):
        enc(clips)
    with torch.no_grad():
        assert enc(clips).shape == (1, 144, 64)
    out = enc(torch.randn(1, 3, 8, 64, 64, device=DEV))            # the native size keeps its autograd path
    assert out.requires_grad
