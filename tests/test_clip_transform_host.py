"""CPU checks of the host half of the device-side clip augmentation (jepa_amd/app/vjepa/transforms.py): the draws against the
reference's (tests/golden/transform_micro.npz, tools/make_golden_transform.py), collation, validation, and the argument checks
of vj_clip_transform (no launch: there is no GPU here)."""
import inspect
import os
import random

import numpy as np
import pytest
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _fixture():
    return np.load(os.path.join(GOLDEN, "transform_micro.npz"))


def test_fixture_holds_the_cases_it_must():
    z = _fixture()
    names = [str(n) for n in z["case_names"]]
    flips = [bool(z[f"{n}/flip"]) for n in names]
    assert any(flips) and not all(flips)
    assert any(bool(z[f"{n}/shift"]) and len({tuple(b) for b in z[f"{n}/boxes"].tolist()}) > 1 for n in names)
    assert any(max(z[f"{n}/frames"].shape[1:3]) < int(z[f"{n}/side"]) for n in names)        # upsampled
    assert any(z[f"{n}/frames"].shape[1] != z[f"{n}/frames"].shape[2] for n in names)        # non-square
    assert any(bool(z[f"{n}/fallback"]) for n in names)
    assert {int(z[f"{n}/side"]) for n in names} == {32, 64}
    assert z["seq/boxes"].shape[0] >= 200 and z["seq/boxes"].shape[0] == z["seq/flip"].shape[0]
    for n in names:
        T, side = z[f"{n}/frames"].shape[0], int(z[f"{n}/side"])
        assert z[f"{n}/ref"].shape == (3, T, side, side) and z[f"{n}/boxes"].shape == (T, 4)


def test_case_draws_equal_the_reference_bit_for_bit():
    from jepa_amd.app.vjepa.transforms import RawClip, VideoTransform
    z = _fixture()
    for n in (str(n) for n in z["case_names"]):
        seed = int(z[f"{n}/seed"])
        random.seed(seed)
        np.random.seed(seed)
        frames = z[f"{n}/frames"]
        clip = VideoTransform(motion_shift=bool(z[f"{n}/shift"]), crop_size=int(z[f"{n}/side"]))(frames)
        assert isinstance(clip, RawClip) and clip.boxes.dtype == torch.int32
        assert np.array_equal(clip.boxes.numpy(), z[f"{n}/boxes"]), n
        assert clip.flip == bool(z[f"{n}/flip"]), n
        assert clip.frames.dtype == torch.uint8 and np.array_equal(clip.frames.numpy(), frames)     # no pixel work
        clip_t = None
        random.seed(seed)
        np.random.seed(seed)
        clip_t = VideoTransform(motion_shift=bool(z[f"{n}/shift"]), crop_size=int(z[f"{n}/side"]))(torch.from_numpy(frames))
        assert torch.equal(clip_t.boxes, clip.boxes) and clip_t.flip == clip.flip                  # tensors as well as arrays


def test_draw_sequence_equals_the_reference_and_leaves_the_generators_where_it_does():
    """>= 200 consecutive draws from one seeding, over mixed source sizes with motion shift on some and central-crop fallbacks
    among them: every box of every frame, every flip; then the next draw of `random` and of `np.random`."""
    from jepa_amd.app.vjepa.transforms import VideoTransform
    z = _fixture()
    T = int(z["T"])
    seed = int(z["seq/seed"])
    random.seed(seed)
    np.random.seed(seed)
    plain, shift = VideoTransform(crop_size=32), VideoTransform(crop_size=32, motion_shift=True)
    n = z["seq/boxes"].shape[0]
    assert n >= 200
    for k in range(n):
        H, W = (int(v) for v in z["seq/hw"][k])
        boxes, flip = (shift if bool(z["seq/shift"][k]) else plain).draw(T, H, W)
        assert np.array_equal(boxes.numpy(), z["seq/boxes"][k]), (k, boxes.tolist(), z["seq/boxes"][k].tolist())
        assert flip == bool(z["seq/flip"][k]), k
    assert [random.random(), np.random.uniform()] == z["seq/next"].tolist()


def test_make_transforms_has_the_reference_signature_and_refuses_what_is_out_of_scope():
    from jepa_amd.app.vjepa.transforms import VideoTransform, make_transforms
    sig = inspect.signature(make_transforms)
    assert list(sig.parameters) == ["random_horizontal_flip", "random_resize_aspect_ratio", "random_resize_scale", "reprob",
                                    "auto_augment", "motion_shift", "crop_size", "normalize"]
    d = {k: p.default for k, p in sig.parameters.items()}
    assert d["random_horizontal_flip"] is True and d["random_resize_aspect_ratio"] == (3 / 4, 4 / 3)
    assert d["random_resize_scale"] == (0.3, 1.0) and d["reprob"] == 0.0 and d["auto_augment"] is False
    assert d["motion_shift"] is False and d["crop_size"] == 224
    assert d["normalize"] == ((0.485, 0.456, 0.406), (0.229, 0.224, 0.225))
    vt = make_transforms()
    assert isinstance(vt, VideoTransform) and vt.crop_size == 224
    # mean / std in 0..255 units, the fp32 values the reference holds
    assert vt.mean == tuple((torch.tensor([0.485, 0.456, 0.406]) * 255.).tolist())
    assert vt.std == tuple((torch.tensor([0.229, 0.224, 0.225]) * 255.).tolist())
    with pytest.raises(NotImplementedError):
        make_transforms(auto_augment=True)
    with pytest.raises(NotImplementedError):
        make_transforms(reprob=0.25)
    with pytest.raises(ValueError):
        make_transforms(crop_size=30)
    with pytest.raises(ValueError):
        vt(np.zeros((4, 8, 8, 3), dtype=np.float32))


def _clips(sizes, T=3, crop=32, seed=5):
    from jepa_amd.app.vjepa.transforms import VideoTransform
    random.seed(seed)
    np.random.seed(seed)
    g = torch.Generator().manual_seed(seed)
    vt = VideoTransform(crop_size=crop, motion_shift=True)
    return [vt(torch.randint(0, 256, (T, h, w, 3), generator=g, dtype=torch.uint8)) for h, w in sizes]


def test_collation_of_mixed_source_sizes():
    from jepa_amd.app.vjepa.transforms import RawClipBatch
    sizes = [(17, 23), (40, 31), (8, 8), (33, 65)]      # 3*h*w*3 bytes: mostly not multiples of 16
    clips = _clips(sizes)
    batch = torch.utils.data.default_collate(clips)
    assert isinstance(batch, RawClipBatch) and len(batch) == 4 and batch.num_frames == 3 and batch.crop_size == 32
    assert batch.frames.dtype == torch.uint8 and batch.desc.dtype == torch.int64 and batch.boxes.dtype == torch.int32
    assert batch.desc.shape == (4, 4) and batch.boxes.shape == (4, 3, 4)
    end = 0
    for b, (c, (h, w)) in enumerate(zip(clips, sizes)):
        off, Hs, Ws, flip = (int(v) for v in batch.desc[b])
        assert off % 16 == 0 and off >= end and (Hs, Ws, flip) == (h, w, int(c.flip))
        end = off + 3 * h * w * 3
        assert torch.equal(batch.clip_frames(b), c.frames)
        assert torch.equal(batch.boxes[b], c.boxes)
    assert batch.frames.numel() >= end and batch.frames.numel() % 16 == 0
    # the VideoDataset item layout through the mask collator's default_collate: ([clips] * num_clips, label, [indices])
    items = [([clips[0], clips[1]], 0, [np.arange(3), np.arange(3)]), ([clips[2], clips[3]], 0, [np.arange(3), np.arange(3)])]
    udata = torch.utils.data.default_collate(items)
    assert len(udata[0]) == 2 and all(isinstance(u, RawClipBatch) and len(u) == 2 for u in udata[0])
    assert torch.equal(udata[0][1].clip_frames(1), clips[3].frames)


def test_mask_collator_passes_raw_clips_through():
    from jepa_amd.app.vjepa.transforms import RawClipBatch
    from jepa_amd.src.masks.multiblock3d import MaskCollator
    mask = dict(aspect_ratio=[0.75, 1.5], num_blocks=2, spatial_scale=[0.15, 0.15], temporal_scale=[1.0, 1.0],
                max_temporal_keep=1.0, max_keep=None)
    coll = MaskCollator(crop_size=64, num_frames=8, patch_size=16, tubelet_size=2, cfgs_mask=[mask])
    clips = _clips([(70, 90), (64, 64)], T=8, crop=64)
    udata, masks_enc, masks_pred = coll([([c], 0, [np.arange(8)]) for c in clips])
    assert isinstance(udata[0][0], RawClipBatch) and len(udata[0][0]) == 2
    assert len(masks_enc) == 1 and masks_enc[0].shape[0] == 2 and masks_pred[0].shape[0] == 2


@pytest.mark.parametrize("bad", [(-1, 0, 4, 4), (0, 0, 0, 4), (0, 0, 4, 0), (5, 0, 4, 4), (0, 7, 4, 4), (0, 0, 9, 4), (0, -2, 4, 4)])
def test_a_box_outside_its_frame_is_refused_on_the_host(bad):
    from jepa_amd.app.vjepa.transforms import RawClip, collate_raw_clips
    T, H, W = 2, 8, 10
    frames = torch.zeros(T, H, W, 3, dtype=torch.uint8)
    good = torch.tensor([[0, 0, 8, 10]] * T, dtype=torch.int32)
    collate_raw_clips([RawClip(frames, good, False, 32, (0., 0., 0.), (1., 1., 1.))])
    boxes = good.clone()
    boxes[1] = torch.tensor(bad, dtype=torch.int32)
    with pytest.raises(ValueError):
        collate_raw_clips([RawClip(frames, boxes, False, 32, (0., 0., 0.), (1., 1., 1.))])


def test_descriptors_outside_the_buffer_are_refused_on_the_host():
    clips = _clips([(12, 12), (9, 20)])
    batch = torch.utils.data.default_collate(clips)
    batch.validate()
    for col, val in ((0, batch.frames.numel()), (0, 8), (0, -16), (1, 13), (2, 0)):
        broken = torch.utils.data.default_collate(clips)
        broken.desc[1, col] = val
        with pytest.raises(ValueError):
            broken.validate()


def test_synthetic_frames_have_the_video_dataset_layout():
    from jepa_amd.app.vjepa.transforms import RawClip, make_transforms
    from jepa_amd.src.datasets.data_manager import SyntheticFrames, init_data
    ds = SyntheticFrames(12, 4, num_clips=2, transform=None, seed=3)
    buf, label, idx = ds[1]
    assert len(buf) == 2 and len(idx) == 2 and label == 0
    assert buf[0].dtype == np.uint8 and buf[0].shape == (4,) + ds.source_size(1) + (3,)
    assert np.array_equal(ds[1][0][0], buf[0]) and not np.array_equal(ds[2][0][0][:, :8, :8], buf[0][:, :8, :8])
    sizes = {ds.source_size(i) for i in range(len(ds))}
    assert any(h != w for h, w in sizes) and any(max(h, w) > 224 for h, w in sizes) and len(sizes) == len(ds.SIZES)
    random.seed(0)
    np.random.seed(0)
    loader, sampler = init_data(data='synthetic_frames', batch_size=3, transform=make_transforms(crop_size=32), clip_len=4,
                                num_workers=0, pin_mem=False, synthetic_length=6, crop_size=32)
    items = [loader.dataset[i] for i in range(2)]
    assert all(isinstance(c, RawClip) for it in items for c in it[0])
    udata, _, _ = next(iter(loader))
    assert len(udata[0]) == 3 and udata[0].boxes.shape == (3, 4, 4)
    with pytest.raises(ValueError):
        init_data(data='synthetic_frames', batch_size=3, transform=None, clip_len=4, num_workers=0, synthetic_length=6)
    with pytest.raises(NotImplementedError, match="uint8"):
        init_data(data='VideoDataset', batch_size=3, transform=None)


def test_entry_point_rejects_bad_arguments_before_any_launch():
    from jepa_amd.hip.lib import load_library
    lib = load_library()
    norm = (123.0, 116.0, 103.0, 58.0, 57.0, 57.0)
    rc = lib.vj_clip_transform(None, 0, None, None, None, 2, 4, 30, *norm, None)
    assert rc < 0 and b"multiple of 4" in lib.vj_last_error()
    for B, T, S in ((2, 0, 32), (2, 4, 0), (-1, 4, 32), (2, -4, 32)):
        rc = lib.vj_clip_transform(None, 0, None, None, None, B, T, S, *norm, None)
        assert rc < 0 and b"bad dims" in lib.vj_last_error(), (B, T, S)
    rc = lib.vj_clip_transform(None, -1, None, None, None, 2, 4, 32, *norm, None)
    assert rc < 0 and b"bad dims" in lib.vj_last_error()
    rc = lib.vj_clip_transform(None, 0, None, None, None, 2, 4, 32, 1.0, 1.0, 1.0, 1.0, 0.0, 1.0, None)
    assert rc < 0 and b"std" in lib.vj_last_error()
    rc = lib.vj_clip_transform(None, 0, None, None, None, 2, 4, 32, *norm, None)
    assert rc < 0 and b"null pointer" in lib.vj_last_error()
    assert lib.vj_clip_transform(None, 0, None, None, None, 0, 4, 32, *norm, None) == 0      # an empty batch launches nothing


def test_clip_transform_op_has_no_cpu_path():
    from jepa_amd.hip import ops
    batch = torch.utils.data.default_collate(_clips([(12, 12), (9, 20)]))
    with pytest.raises(ValueError):
        ops.clip_transform(batch.frames, batch.desc, batch.boxes, batch.crop_size, batch.mean, batch.std)
