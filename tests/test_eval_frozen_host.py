"""CPU checks of the frozen video-classification eval (jepa_amd/evals/video_classification_frozen): the synthetic items and their
collation have the reference's layout, the six shipped video eval configs give the probe key counts the split kernels exist for,
and the host side of the workspace entry points (no launch: there is no GPU here)."""
import pytest
import torch

# the six video eval configs of the reference (configs/evals/vit{l16,h16,h16_384}_{k400_16x8x3,ssv2_16x2x3}.yaml): the fields
# that set the probe's key count
CONFIGS = {
    "vitl16_k400_16x8x3": dict(model_name="vit_large", resolution=224, frames_per_clip=16, tubelet_size=2, patch_size=16,
                               num_segments=8, num_views_per_segment=3, attend_across_segments=True, num_classes=400),
    "vith16_k400_16x8x3": dict(model_name="vit_huge", resolution=224, frames_per_clip=16, tubelet_size=2, patch_size=16,
                               num_segments=8, num_views_per_segment=3, attend_across_segments=True, num_classes=400),
    "vith16_384_k400_16x8x3": dict(model_name="vit_huge", resolution=384, frames_per_clip=16, tubelet_size=2, patch_size=16,
                                   num_segments=8, num_views_per_segment=3, attend_across_segments=True, num_classes=400),
    "vitl16_ssv2_16x2x3": dict(model_name="vit_large", resolution=224, frames_per_clip=16, tubelet_size=2, patch_size=16,
                               num_segments=2, num_views_per_segment=3, attend_across_segments=True, num_classes=174),
    "vith16_ssv2_16x2x3": dict(model_name="vit_huge", resolution=224, frames_per_clip=16, tubelet_size=2, patch_size=16,
                               num_segments=2, num_views_per_segment=3, attend_across_segments=True, num_classes=174),
    "vith16_384_ssv2_16x2x3": dict(model_name="vit_huge", resolution=384, frames_per_clip=16, tubelet_size=2, patch_size=16,
                                   num_segments=2, num_views_per_segment=3, attend_across_segments=True, num_classes=174),
}
EXPECTED_N = {"vitl16_k400_16x8x3": 12544, "vith16_k400_16x8x3": 12544, "vith16_384_k400_16x8x3": 36864,
              "vitl16_ssv2_16x2x3": 3136, "vith16_ssv2_16x2x3": 3136, "vith16_384_ssv2_16x2x3": 9216}
DIMS = {"vit_large": (1024, 16), "vit_huge": (1280, 16)}
FWD_MAX, BWD_MAX = 38264, 19132


def _probe_keys(c):
    tokens = (c["frames_per_clip"] // c["tubelet_size"]) * (c["resolution"] // c["patch_size"]) ** 2
    return tokens * (c["num_segments"] if c["attend_across_segments"] else 1), tokens


def test_synthetic_items_have_the_reference_layout():
    from jepa_amd.src.datasets.data_manager import SyntheticVideoClassification
    S, V, T, R, C = 3, 2, 8, 32, 7
    ds = SyntheticVideoClassification(16, C, T, R, num_segments=S, num_views_per_segment=V, frame_step=4, seed=5)
    clips, label, idx = ds[3]
    assert len(clips) == S and all(len(seg) == V for seg in clips)
    assert all(v.shape == (3, T, R, R) and v.dtype == torch.float32 for seg in clips for v in seg)
    assert isinstance(label, int) and 0 <= label < C
    assert len(idx) == S and all(i.dtype == torch.int64 and i.shape == (T,) for i in idx)
    # deterministic per (seed, index); another seed or index gives other clips
    clips2, label2, _ = ds[3]
    assert label2 == label and all(torch.equal(a, b) for sa, sb in zip(clips, clips2) for a, b in zip(sa, sb))
    assert not torch.equal(ds[4][0][0][0], clips[0][0])
    other = SyntheticVideoClassification(16, C, T, R, num_segments=S, num_views_per_segment=V, seed=6)
    assert not torch.equal(other[3][0][0][0], clips[0][0])
    labels = [ds[i][1] for i in range(len(ds))]
    assert all(0 <= lb < C for lb in labels) and len(set(labels)) > 1
    # the default collation: [S] of [V] of [B,3,T,H,W], labels [B], [S] of [B,T]
    batch = torch.utils.data.default_collate([ds[0], ds[1], ds[2], ds[3]])
    assert len(batch[0]) == S and len(batch[0][0]) == V and batch[0][0][0].shape == (4, 3, T, R, R)
    assert batch[1].shape == (4,) and batch[1].dtype == torch.int64
    assert len(batch[2]) == S and batch[2][0].shape == (4, T)


def test_synthetic_clips_carry_a_class_dependent_signal():
    from jepa_amd.src.datasets.data_manager import SyntheticVideoClassification
    ds = SyntheticVideoClassification(64, 3, 4, 16, seed=0)
    by_class = {}
    for i in range(len(ds)):
        clips, label, _ = ds[i]
        by_class.setdefault(label, []).append(clips[0][0])
    means = {k: torch.stack(v).mean(0) for k, v in by_class.items() if len(v) >= 8}
    assert len(means) >= 2
    a, b = list(means.values())[:2]
    assert float((a - b).pow(2).mean()) > 0.2   # noise alone: ~2/8 at most; the patterns differ by far more


@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_shipped_video_configs_give_the_probe_key_counts(name):
    from jepa_amd.evals.video_classification_frozen.utils import max_clips_per_call
    c = CONFIGS[name]
    N, tokens = _probe_keys(c)
    assert N == EXPECTED_N[name]
    D, H = DIMS[c["model_name"]]
    # the frozen forward's call size keeps fc1's output (M x 4D elements) below 2^31
    m = max_clips_per_call(4 * D, tokens)
    assert m * tokens * 4 * D < 2 ** 31 <= (m + 1) * tokens * 4 * D
    if name == "vith16_384_k400_16x8x3":
        assert m == 91 and N > BWD_MAX   # 96 validation clips: two encoder calls; the probe backward needs the split kernels


def test_workspace_sizes_follow_the_limits():
    from jepa_amd.hip.lib import load_library
    lib = load_library()
    for B, H, hd in [(4, 16, 64), (4, 16, 80), (1, 2, 128), (3, 1, 8)]:
        assert lib.vj_xattn_ws_bytes(B, 1, FWD_MAX, H, hd, 0) == 0 and lib.vj_xattn_ws_bytes(B, 1, FWD_MAX + 1, H, hd, 0) > 0
        assert lib.vj_xattn_ws_bytes(B, 1, BWD_MAX, H, hd, 1) == 0 and lib.vj_xattn_ws_bytes(B, 1, BWD_MAX + 1, H, hd, 1) > 0
        assert lib.vj_xattn_ws_bytes(B, 3, 1568, H, hd, 0) == 0
    for name, c in CONFIGS.items():
        N, _ = _probe_keys(c)
        D, H = DIMS[c["model_name"]]
        assert (lib.vj_xattn_ws_bytes(4, 1, N, H, D // H, 1) > 0) == (N > BWD_MAX), name
        assert lib.vj_xattn_ws_bytes(4, 1, N, H, D // H, 0) == 0, name   # every shipped config fits the forward
    # split backward: p and dP (8 bytes per key) dominate
    assert lib.vj_xattn_ws_bytes(4, 1, 36864, 16, 80, 1) >= 4 * 16 * 36864 * 8
    assert lib.vj_xattn_ws_bytes(4, 1, 36864, 16, 60, 1) < 0   # head_dim not a multiple of 8


def test_ws_entry_points_reject_before_any_launch():
    from jepa_amd.hip.lib import load_library
    lib = load_library()
    N = 73728
    need_f, need_b = lib.vj_xattn_ws_bytes(4, 1, N, 16, 64, 0), lib.vj_xattn_ws_bytes(4, 1, N, 16, 64, 1)
    assert need_f > 0 and need_b > 0
    # a short workspace: refused on the host with a negative code (null device pointers are never touched)
    rc = lib.vj_xattn_fwd_ws(None, 0, None, None, None, None, 4, 1, N, 16, 64, 0.125, None, need_f, None)
    assert rc < 0 and b"workspace" in lib.vj_last_error()
    rc = lib.vj_xattn_fwd_ws(None, 0, None, None, None, None, 4, 1, N, 16, 64, 0.125, 16, need_f - 1, None)
    assert rc < 0 and b"workspace" in lib.vj_last_error()
    rc = lib.vj_xattn_bwd_ws(None, 0, None, None, None, None, None, 4, 1, N, 16, 64, 0.125, 16, need_b - 1, None)
    assert rc < 0 and b"workspace" in lib.vj_last_error()
    # a bad head_dim, several queries in the backward, a grid that is too large
    rc = lib.vj_xattn_fwd_ws(None, 0, None, None, None, None, 4, 1, N, 16, 60, 0.125, 16, 1 << 40, None)
    assert rc < 0 and b"head_dim" in lib.vj_last_error()
    rc = lib.vj_xattn_bwd_ws(None, 0, None, None, None, None, None, 4, 2, N, 16, 64, 0.125, 16, 1 << 40, None)
    assert rc < 0 and b"one query" in lib.vj_last_error()
    rc = lib.vj_xattn_fwd_ws(None, 0, None, None, None, None, 1 << 22, 1, N, 16, 64, 0.125, 16, 1 << 62, None)
    assert rc < 0 and b"grid" in lib.vj_last_error()
    # within the limits the single-workgroup validation answers (same messages as vj_xattn_fwd / _bwd)
    rc = lib.vj_xattn_fwd_ws(None, 0, None, None, None, None, 4, 1, 100, 16, 60, 0.125, None, 0, None)
    assert rc < 0 and b"head_dim" in lib.vj_last_error()


def test_unsupported_eval_paths_raise():
    from jepa_amd.evals.video_classification_frozen.eval import make_dataloader
    from jepa_amd.evals.video_classification_frozen.utils import ClipAggregation, FrameAggregation

    class Stub(torch.nn.Module):
        embed_dim, num_heads, num_patches = 64, 2, 64

    for kind in ("VideoDataset", "ImageNet", "webvid"):
        with pytest.raises(NotImplementedError):
            make_dataloader(root_path=["/nonexistent"], batch_size=2, world_size=1, rank=0, dataset_type=kind, num_classes=10)
    with pytest.raises(NotImplementedError):
        ClipAggregation(Stub(), use_pos_embed=True)
    with pytest.raises(NotImplementedError):
        FrameAggregation(Stub())
    agg = ClipAggregation(Stub(), attend_across_segments=True)
    assert agg.embed_dim == 64 and agg.num_heads == 2 and agg.attend_across_segments and agg.tubelet_size == 2
    loader = make_dataloader(root_path=[None], batch_size=2, world_size=1, rank=0, dataset_type="synthetic", resolution=32,
                             frames_per_clip=4, num_segments=2, num_views_per_segment=3, num_classes=10, num_workers=0,
                             synthetic_length=4)
    clips, labels, idx = next(iter(loader))
    assert len(loader) == 2 and len(clips) == 2 and len(clips[0]) == 3 and clips[0][0].shape == (2, 3, 4, 32, 32)


def test_train_and_validation_splits_share_their_classes():
    """The training (seed 0) and validation (seed 1) splits of make_dataloader draw other items but the same class patterns: a
    class's mean clip agrees across the splits, and a nearest-class-mean rule fitted on one split classifies the other."""
    from jepa_amd.evals.video_classification_frozen.eval import make_dataloader
    kw = dict(root_path=[None], batch_size=8, world_size=1, rank=0, dataset_type="synthetic", resolution=16, frames_per_clip=4,
              num_segments=1, num_views_per_segment=1, num_classes=3, num_workers=0, synthetic_length=96)
    tr, va = make_dataloader(training=True, **kw).dataset, make_dataloader(training=False, **kw).dataset
    assert tr.seed != va.seed and not torch.equal(tr[0][0][0][0], va[0][0][0][0])

    def class_means(ds):
        by = {}
        for i in range(len(ds)):
            clips, label, _ = ds[i]
            by.setdefault(label, []).append(clips[0][0].reshape(-1))
        return {k: torch.stack(v).mean(0) for k, v in by.items()}

    mt, mv = class_means(tr), class_means(va)
    assert sorted(mt) == sorted(mv) == [0, 1, 2]
    for k in mt:
        cos = float(torch.nn.functional.cosine_similarity(mt[k], mv[k], dim=0))
        assert cos > 0.8, (k, cos)
    correct = 0
    for i in range(len(va)):
        clips, label, _ = va[i]
        x = clips[0][0].reshape(-1)
        correct += int(min(mt, key=lambda k: float((x - mt[k]).pow(2).sum())) == label)
    assert correct / len(va) > 0.9, correct


def test_eval_micro_fixture_clips_regenerate():
    """tests/golden/eval_micro.npz keeps only the seed and the sha256 of its clips; the CPU generator reproduces them."""
    import os
    import numpy as np
    from tests.eval_golden_util import micro_clips
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "eval_micro.npz"))
    S, V, B, C, iters, T, crop = (int(x) for x in z["dims"])
    train, train_labels, val, val_labels = micro_clips(int(z["clip_seed"]), S, V, B, C, iters, T, crop, z["clips_sha256"])
    assert z["feat"].shape == (S * V * B, 64, 64) and z[f"agg/v{V - 1}"].shape == (B, S * 64, 64)
    assert z["iter_loss"].shape == (iters + 1,) and all(str(k).startswith("pooler.") or str(k).startswith("linear.")
                                                         for k in z["clf_keys"])


def test_ws_entry_points_accept_an_empty_batch_above_the_limits():
    """B == 0 needs no workspace at any N (vj_xattn_ws_bytes says 0) and launches nothing, as vj_xattn_fwd / _bwd do."""
    from jepa_amd.hip.lib import load_library
    lib = load_library()
    N = 73728
    assert lib.vj_xattn_ws_bytes(0, 1, N, 16, 64, 0) == 0 and lib.vj_xattn_ws_bytes(0, 1, N, 16, 64, 1) == 0
    assert lib.vj_xattn_fwd_ws(None, 0, None, None, None, None, 0, 1, N, 16, 64, 0.125, None, 0, None) == 0
    assert lib.vj_xattn_bwd_ws(None, 0, None, None, None, None, None, 0, 1, N, 16, 64, 0.125, None, 0, None) == 0


def test_encoder_call_cap_follows_the_widest_activation():
    """The cap reads fc1's width from the model: ViT-g (mlp_ratio 48/11, fc1 6144 wide) at 384 px gets 75 clips per call, where a
    4 D assumption would allow 82 (82 x 4608 x 6144 > 2^31)."""
    from jepa_amd.evals.video_classification_frozen.utils import ClipAggregation

    class Fc1:
        out_features = 6144

    class Mlp:
        fc1 = Fc1()

    class Blk:
        mlp = Mlp()

    class ViTg(torch.nn.Module):
        embed_dim, num_heads, num_patches = 1408, 16, 4608
        blocks = [Blk()]

    m = ClipAggregation(ViTg()).max_clips_per_call
    assert m == 75 and m * 4608 * 6144 < 2 ** 31 <= (m + 1) * 4608 * 6144
