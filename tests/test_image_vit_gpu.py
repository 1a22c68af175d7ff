"""GPU: the image (num_frames=1) VisionTransformer, vj_pos_interp2d_bicubic, vj_add_pos_frames and FrameAggregation against
tests/golden/image_vit_micro.npz (the reference's image ViT and FrameAggregation on the CPU, tools/make_golden_image_vit.py) and
against F.interpolate(mode='bicubic') on the CPU for the ViT-L/16 and ViT-H/16-384 tables."""
import math

import pytest
import torch
import torch.nn.functional as F

from tests.image_vit_golden_util import fixture, micro_frames, micro_image_vit, micro_images

pytestmark = pytest.mark.gpu
DEV = "cuda"
TABLE_TOL = 1e-5     # the bound tests/test_pos_interp_gpu.py holds the trilinear kernel to; bicubic weights reach ~1.3 in magnitude
                     # on tables bounded by 1, 16 fp32 products per value: error of order 1e-6
FEATURE_TOL = 2e-2   # rel-L2, the project's bound for micro-model features against the reference


def rel_l2(a, b):
    a, b = torch.as_tensor(a).detach().float().cpu().reshape(-1), torch.as_tensor(b).detach().float().cpu().reshape(-1)
    return float((a - b).norm() / (b.norm() + 1e-12))


@pytest.fixture(scope="module")
def z():
    return fixture()


@pytest.fixture(scope="module")
def enc(z):
    return micro_image_vit(z).to(DEV)


def test_bicubic_kernel_against_the_reference_tables(z):
    from jepa_amd.hip import ops
    table = torch.from_numpy(z["pos2d"]).view(4, 4, 64).to(DEV)
    for side in (6, 2, 7, 5):
        ref = torch.from_numpy(z[f"interp/{side * 8}x{side * 8}"])
        out = ops.pos_interp2d_bicubic(table, math.sqrt(side * side / 16))      # the reference's scale factor
        assert out.dtype == torch.float32 and tuple(out.shape) == (side, side, 64)
        err = float((out.cpu().view(-1, 64) - ref).abs().max())
        print(f"pos_interp2d_bicubic 4x4 -> {side}x{side}: max abs err {err:.3e}")
        assert err <= TABLE_TOL, (side, err)


@pytest.mark.parametrize("name,D,src,dst", [("vit_large_224_to_384", 1024, 14, 24), ("vit_huge_384_to_224", 1280, 24, 14)])
def test_bicubic_kernel_against_f_interpolate(name, D, src, dst):
    from jepa_amd.hip import ops
    from jepa_amd.src.models.utils.pos_embs import get_2d_sincos_pos_embed
    table = torch.from_numpy(get_2d_sincos_pos_embed(D, src, cls_token=False)).float()
    scale = math.sqrt(dst * dst / (src * src))                                   # as interpolate_pos_encoding computes it
    ref = F.interpolate(table.reshape(1, src, src, D).permute(0, 3, 1, 2), scale_factor=scale, mode='bicubic').permute(0, 2, 3, 1)[0]
    out = ops.pos_interp2d_bicubic(table.view(src, src, D).to(DEV), scale)
    assert tuple(out.shape) == tuple(ref.shape) == (dst, dst, D)
    err = float((out.cpu() - ref).abs().max())
    print(f"pos_interp2d_bicubic {name}: max abs err {err:.3e}")
    assert err <= TABLE_TOL, (name, err)


def test_model_tables_native_is_the_parameter_and_others_are_cached(z, enc):
    assert enc.interpolate_pos_encoding(torch.empty(1, 3, 32, 32, device=DEV), enc.pos_embed) is enc.pos_embed
    x = torch.empty(1, 3, 48, 48, device=DEV)
    t1 = enc.interpolate_pos_encoding(x, enc.pos_embed)
    assert t1.shape == (1, 36, 64) and enc.interpolate_pos_encoding(x, enc.pos_embed) is t1
    assert float((t1[0].cpu() - torch.from_numpy(z["interp/48x48"])).abs().max()) <= TABLE_TOL


def test_encoder_features_at_five_sizes_and_masked_match_the_reference(z, enc):
    """One encoder object called at the five sizes and at the native size in turn, twice: the native result never changes."""
    native, mask = micro_images(z, 32)
    native = native.to(DEV)
    with torch.no_grad():
        base = enc(native)
        for rnd in range(2):
            for size in (int(s) for s in z["sizes"]):
                images, _ = micro_images(z, size)
                ref = z[f"feat/{size}x{size}"]
                out = enc(images.to(DEV))
                assert tuple(out.shape) == ref.shape and out.dtype == torch.bfloat16
                e = rel_l2(out, ref)
                print(f"image ViT features {size}x{size} ({ref.shape[1]} tokens): rel-L2 {e:.3e}")
                assert e <= FEATURE_TOL, (size, e)
                assert torch.equal(enc(native), base)
            for masks in ([mask.to(DEV)], mask.to(DEV)):          # a list of one mask, and the bare tensor
                out = enc(native, masks)
                assert tuple(out.shape) == z["feat_masked/32x32"].shape == (2, 5, 64)
                e = rel_l2(out, z["feat_masked/32x32"])
                print(f"image ViT masked features 32x32: rel-L2 {e:.3e}")
                assert e <= FEATURE_TOL, e
    assert (z["mask/32x32"] == mask.numpy()).all()


def test_shape_errors_on_the_gpu(enc):
    with torch.no_grad():
        with pytest.raises(ValueError, match="4x8"):
            enc(torch.zeros(1, 3, 32, 64, device=DEV))
        with pytest.raises(ValueError, match="FrameAggregation"):
            enc(torch.zeros(1, 3, 4, 32, 32, device=DEV))


@pytest.mark.parametrize("D", [64, 72, 1024])
@pytest.mark.parametrize("N", [1, 16])
@pytest.mark.parametrize("Fr", [1, 8])
def test_add_pos_frames_is_the_single_rounded_add(D, N, Fr):
    from jepa_amd.hip import ops
    B, max_frames = 3, 11
    g = torch.Generator().manual_seed(D * 100 + N * 10 + Fr)
    x = torch.randn(B, Fr * N, D, generator=g).to(torch.bfloat16).to(DEV)
    pos = torch.randn(max_frames, D, generator=g).to(DEV)
    idx = torch.randint(0, max_frames, (B, Fr), generator=g)
    if Fr == 8:
        idx[0] = torch.tensor([10, 0, 10, 3, 3, 2, 9, 0])          # repeated and out of order, both ends of the table
    idx = idx.to(DEV)
    ref = (x.float().view(B, Fr, N, D) + pos[idx][:, :, None, :]).to(torch.bfloat16).view(B, Fr * N, D)
    out = ops.add_pos_frames(x.clone(), pos, idx, N)
    assert torch.equal(out, ref)


def _to_dev(clips, indices):
    return [[c.to(DEV) for c in seg] for seg in clips], [i.to(DEV) for i in indices]


@pytest.mark.parametrize("use_pos", [False, True])
def test_frame_aggregation_against_the_reference(z, enc, use_pos):
    from jepa_amd.evals.video_classification_frozen.utils import FrameAggregation
    S, V, T, max_frames = (int(v) for v in z["agg_dims"])
    clips, indices = _to_dev(*micro_frames(z))
    agg = FrameAggregation(enc, max_frames=max_frames, use_pos_embed=use_pos).to(DEV)
    with torch.no_grad():
        outs = agg(clips, indices)
    assert isinstance(outs, list) and len(outs) == V
    for j, o in enumerate(outs):
        ref = z[("agg_pos" if use_pos else "agg") + f"/view{j}"]
        assert tuple(o.shape) == ref.shape == (2, S * T * 16, 64) and o.dtype == torch.bfloat16
        e = rel_l2(o, ref)
        print(f"FrameAggregation use_pos_embed={use_pos} view {j}: rel-L2 {e:.3e}")
        assert e <= FEATURE_TOL, (j, e)
    if use_pos:                                   # without clip_indices the table is not applied, as in the reference
        with torch.no_grad():
            plain = FrameAggregation(enc).to(DEV)(clips, indices)
            none = agg(clips, None)
        assert all(torch.equal(a, b) for a, b in zip(none, plain)) and not torch.equal(outs[0], plain[0])


def test_frames_route_equals_the_model_on_the_permuted_batch(z, enc):
    clips, _ = micro_frames(z)
    x = clips[0][0].to(DEV)                                       # [B, 3, T, 32, 32]
    B, C, T, H, W = x.shape
    with torch.no_grad():
        direct = enc.forward_frames(x)
        permuted = enc(x.permute(0, 2, 1, 3, 4).reshape(B * T, C, H, W))
        both = enc.forward_frames([x, clips[1][1].to(DEV)])
    assert tuple(direct.shape) == (B, T * 16, 64) and torch.equal(direct, permuted.reshape(B, T * 16, 64))
    assert torch.equal(both[0], direct) and tuple(both[1].shape) == (B, T * 16, 64)


def test_forced_chunking_equals_the_single_call(z, enc, monkeypatch):
    from jepa_amd.evals.video_classification_frozen.utils import FrameAggregation
    clips, indices = _to_dev(*micro_frames(z))
    agg = FrameAggregation(enc, max_frames=32, use_pos_embed=True).to(DEV)
    calls = []
    real = enc.forward_frames
    monkeypatch.setattr(enc, "forward_frames", lambda parts: calls.append(sum(c.shape[0] * c.shape[2] for c in parts)) or real(parts))
    with torch.no_grad():
        whole = agg(clips, indices)
        assert calls == [32]                                       # 2 segments x 2 views x 2 samples x 4 frames in one call
        for tokens, expect in ((12 * 16, [8, 8, 8, 8]), (4 * 16, [4] * 8), (3 * 16, [3, 1] * 8)):
            del calls[:]
            agg.max_tokens_per_call = tokens                       # whole tensors, runs of samples, runs of frames of one sample
            split = agg(clips, indices)
            assert calls == expect, (tokens, calls)
            assert all(torch.equal(a, b) for a, b in zip(split, whole)), tokens


def test_segments_of_different_length_follow_one_another_along_time(z, enc):
    """The reference concatenates the segments along time, whatever their lengths: frame offsets are the running sum."""
    from jepa_amd.evals.video_classification_frozen.utils import FrameAggregation
    clips, _ = micro_frames(z)
    x = [[c.to(DEV) for c in clips[0]], [c[:, :, :2].contiguous().to(DEV) for c in clips[1]]]      # 4 frames, then 2
    idx = [torch.tensor([[5, 1, 7, 0], [2, 2, 9, 31]], device=DEV), torch.tensor([[3, 30], [0, 8]], device=DEV)]
    agg = FrameAggregation(enc, max_frames=32, use_pos_embed=True).to(DEV)
    with torch.no_grad():
        outs = agg(x, idx)
        for j, o in enumerate(outs):
            assert tuple(o.shape) == (2, 6 * 16, 64)
            both = torch.cat([enc.forward_frames(x[0][j]), enc.forward_frames(x[1][j])], dim=1)
            pos = agg.pos_embed[0][torch.cat(idx, dim=1)]                                        # [B, 6, D]
            ref = (both.float().view(2, 6, 16, 64) + pos[:, :, None, :]).to(torch.bfloat16).view(2, 96, 64)
            assert torch.equal(o, ref), j
        agg.max_tokens_per_call = 3 * 16
        assert all(torch.equal(a, b) for a, b in zip(agg(x, idx), outs))
