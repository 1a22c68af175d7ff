"""CPU checks of the image (num_frames=1) VisionTransformer, FrameAggregation and the host side of vj_pos_interp2d_bicubic and
vj_add_pos_frames, against tests/golden/image_vit_micro.npz (tools/make_golden_image_vit.py).  No launch: there is no GPU here."""
import os
from functools import partial

import numpy as np
import pytest
import torch

from tests.image_vit_golden_util import GOLDEN, fixture, micro_frames, micro_image_vit, micro_images


def test_fixture_holds_arrays_and_name_lists_only():
    path = os.path.join(GOLDEN, "image_vit_micro.npz")
    assert os.path.getsize(path) <= 1_000_000
    z = np.load(path, allow_pickle=False)            # an object array (pickled code) would refuse to load
    for k in z.files:
        assert z[k].dtype.kind in "fiuU", (k, z[k].dtype)
    assert [int(s) for s in z["sizes"]] == [32, 48, 16, 56, 40]
    assert {f"interp/{s}x{s}" for s in (48, 16, 56, 40)} <= set(z.files) and "feat_masked/32x32" in z.files
    for s in (32, 48, 16, 56, 40):
        micro_images(z, s)                            # the recorded seeds regenerate the recorded inputs
    micro_frames(z)


def test_image_vit_constructs_with_the_reference_state_dict_and_tables():
    from jepa_amd.evals.video_classification_frozen.utils import FrameAggregation
    from jepa_amd.src.models import vision_transformer as vit
    z = fixture()
    enc = micro_image_vit(z, load=False)
    sd = enc.state_dict()
    assert list(sd) == [str(k) for k in z["keys"]]
    for k, v in sd.items():
        assert tuple(v.shape) == z["w/" + k].shape, k
    assert tuple(sd["patch_embed.proj.weight"].shape) == (64, 3, 8, 8) and tuple(sd["pos_embed"].shape) == (1, 16, 64)
    assert not enc.is_video and enc.num_patches == 16 and not enc.pos_embed.requires_grad
    assert np.array_equal(enc.pos_embed[0].numpy(), z["pos2d"])                       # bit-equal 2-D sincos table
    agg = FrameAggregation(enc, max_frames=int(z["agg_dims"][3]), use_pos_embed=True)
    assert np.array_equal(agg.pos_embed[0].numpy(), z["pos1d"]) and not agg.pos_embed.requires_grad
    assert agg.model is enc and agg.embed_dim == 64 and agg.num_heads == 2 and agg.attend_across_segments is False
    assert FrameAggregation(enc).pos_embed is None
    micro_image_vit(z)                                                                # the recorded state loads strictly
    large = vit.vit_large()                                                           # the reference's default: num_frames=1
    assert not large.is_video and large.num_patches == 196 and tuple(large.patch_embed.proj.weight.shape) == (1024, 3, 16, 16)


def test_limits_raise_value_errors():
    from jepa_amd.evals.video_classification_frozen.utils import FrameAggregation
    from jepa_amd.src.models import vision_transformer as vit
    z = fixture()
    enc = micro_image_vit(z)
    with torch.no_grad():
        with pytest.raises(ValueError, match="no CPU fallback"):
            enc(torch.zeros(1, 3, 32, 32))                                            # there is no CPU path
        with pytest.raises(ValueError, match="4x8"):
            enc(torch.zeros(1, 3, 32, 64))                                            # non-square: both grids are named
        with pytest.raises(ValueError, match="2x8"):
            enc(torch.zeros(1, 3, 16, 64))                                            # 16 tokens, as the native grid has, but not 4x4
        with pytest.raises(ValueError, match="FrameAggregation"):
            enc(torch.zeros(1, 3, 4, 32, 32))                                         # a clip: frames go through FrameAggregation
        with pytest.raises(ValueError, match="divisible"):
            enc(torch.zeros(1, 3, 36, 36))
        assert enc.interpolate_pos_encoding(torch.zeros(1, 3, 32, 32), enc.pos_embed) is enc.pos_embed
        with pytest.raises(ValueError):
            enc.interpolate_pos_encoding(torch.zeros(1, 3, 48, 48), enc.pos_embed)    # the table is computed on the GPU only
    with pytest.raises(ValueError, match="multiple of 8"):
        vit.vit_gigantic()                                                            # patch 14
    for p in enc.parameters():
        p.requires_grad = True
    with pytest.raises(NotImplementedError, match="frozen"):
        enc(torch.zeros(1, 3, 32, 32))
    video = vit.VisionTransformer(img_size=32, patch_size=8, num_frames=4, tubelet_size=2, embed_dim=64, depth=1, num_heads=2,
                                  norm_layer=partial(torch.nn.LayerNorm, eps=1e-6))
    with pytest.raises(NotImplementedError):
        FrameAggregation(video)
    with pytest.raises(ValueError):
        video.forward_frames(torch.zeros(1, 3, 4, 32, 32))


def test_frame_aggregation_rejects_indices_outside_the_table():
    from jepa_amd.evals.video_classification_frozen.utils import FrameAggregation
    z = fixture()
    agg = FrameAggregation(micro_image_vit(z), max_frames=8, use_pos_embed=True)
    clips = [[torch.zeros(1, 3, 2, 32, 32)]]
    with torch.no_grad():
        for bad in ([[0, 8]], [[-1, 0]], [[0, 1, 2]]):
            with pytest.raises(ValueError, match="clip_indices"):
                agg(clips, [torch.tensor(bad)])


def test_frame_aggregation_rejects_clips_that_cannot_be_concatenated():
    from jepa_amd.evals.video_classification_frozen.utils import FrameAggregation
    agg = FrameAggregation(micro_image_vit(fixture()))
    a, short, wide, small = (torch.zeros(2, 3, 4, 32, 32), torch.zeros(2, 3, 2, 32, 32), torch.zeros(2, 3, 4, 32, 64),
                             torch.zeros(1, 3, 4, 32, 32))
    with torch.no_grad():
        for bad in ([[a, short]], [[a], [wide]], [[a], [small]], [[a, a], [a]], [[a[0]]]):
            with pytest.raises(ValueError, match="differ in T"):
                agg(bad)


def test_pieces_cover_every_frame_once_within_the_call_limit():
    from jepa_amd.evals.video_classification_frozen.utils import FrameAggregation
    z = fixture()
    agg = FrameAggregation(micro_image_vit(z))
    V, B, lengths = 3, 5, (4, 2, 5)                     # segments of different lengths: offsets are the running sum
    x = [[torch.zeros(B, 3, T, 8, 8) for _ in range(V)] for T in lengths]
    for cap in (1, 3, 4, 7, 8, 20, 1000):
        seen = set()
        for c, j, b0, f0 in agg._pieces(x, cap):
            assert c.shape[0] * c.shape[2] <= cap
            for b in range(b0, b0 + c.shape[0]):
                for f in range(f0, f0 + c.shape[2]):
                    assert (j, b, f) not in seen
                    seen.add((j, b, f))
        assert seen == {(j, b, f) for j in range(V) for b in range(B) for f in range(sum(lengths))}, cap


def test_new_entry_points_reject_bad_arguments_before_any_launch():
    from jepa_amd.hip.lib import load_library
    lib = load_library()
    rc = lib.vj_pos_interp2d_bicubic(None, None, 4, 4, 62, 1.5, 6, 6, None)
    assert rc < 0 and b"multiple of 4" in lib.vj_last_error()
    for scale in (0.0, -1.5):
        rc = lib.vj_pos_interp2d_bicubic(None, None, 4, 4, 64, scale, 6, 6, None)
        assert rc < 0 and b"positive" in lib.vj_last_error()
    rc = lib.vj_pos_interp2d_bicubic(None, None, 4, 4, 64, 1.5, 7, 6, None)
    assert rc < 0 and b"floor" in lib.vj_last_error()
    rc = lib.vj_pos_interp2d_bicubic(None, None, 4, 4, 64, 1.5, 6, 7, None)
    assert rc < 0 and b"floor" in lib.vj_last_error()
    rc = lib.vj_pos_interp2d_bicubic(None, None, 4, 0, 64, 1.5, 6, 0, None)
    assert rc < 0 and b"bad table dims" in lib.vj_last_error()
    rc = lib.vj_pos_interp2d_bicubic(None, None, 4, 4, 64, 1.5, 6, 6, None)          # all sizes right: the null table is refused
    assert rc < 0 and b"null" in lib.vj_last_error()
    rc = lib.vj_add_pos_frames(None, None, None, 2, 4, 16, 60, 32, None)
    assert rc < 0 and b"multiple of 8" in lib.vj_last_error()
    for dims in ((-2, 4, 16), (2, -4, 16), (2, 4, -16)):
        rc = lib.vj_add_pos_frames(None, None, None, *dims, 64, 32, None)
        assert rc < 0 and b"bad dims" in lib.vj_last_error()
    rc = lib.vj_add_pos_frames(None, None, None, 2, 4, 16, 64, 0, None)
    assert rc < 0 and b"bad dims" in lib.vj_last_error()
    assert lib.vj_add_pos_frames(None, None, None, 0, 4, 16, 64, 32, None) == 0      # an empty batch launches nothing
    rc = lib.vj_add_pos_frames(None, None, None, 2, 4, 16, 64, 32, None)
    assert rc < 0 and b"null" in lib.vj_last_error()


def test_video_eval_with_an_image_encoder_needs_attend_across_segments(tmp_path):
    """Raised from the configuration, before any device is asked for."""
    from jepa_amd.evals.video_classification_frozen.eval import main
    cfg = {'pretrain': {'model_name': 'vit_tiny', 'patch_size': 16, 'folder': str(tmp_path), 'checkpoint': 'x.pth.tar', 'write_tag': 't'},
           'data': {'dataset_type': 'synthetic', 'num_classes': 4},
           'optimization': {'attend_across_segments': False, 'batch_size': 2, 'num_epochs': 1}}
    with pytest.raises(ValueError, match="concatenated form"):
        main(cfg)
