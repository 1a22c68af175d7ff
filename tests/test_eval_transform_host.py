"""CPU checks of the host half of the frozen eval's uint8 input path: the draws of the eval's transforms
(jepa_amd/evals/video_classification_frozen/utils.py) and of RandomErasing (jepa_amd/app/vjepa/transforms.py draw_erase) against the
reference's (tests/golden/eval_transform_micro.npz, tools/make_golden_eval_transform.py), the view-major collation, validation, a
float32 restatement of the device arithmetic against the reference's outputs, and the argument checks of vj_clip_transform_pre and
vj_clip_erase (no launch: there is no GPU here)."""
import inspect
import random

import numpy as np
import pytest
import torch

from . import eval_transform_util as U


def test_fixture_holds_the_cases_it_must():
    z = U.fixture()
    tr, ce, vi = U.names("train"), U.names("centre"), U.names("views")
    assert int(z["T"]) == 4
    flips = [bool(z[f"{n}/flip"]) for n in tr]
    assert any(flips) and not all(flips)
    assert any(bool(z[f"{n}/shift"]) and len({tuple(b) for b in z[f"{n}/boxes"].tolist()}) > 1 for n in tr)
    assert any(not bool(z[f"{n}/shift"]) for n in tr)
    assert {float(z[f"{n}/reprob"]) for n in tr} == {0.0, 1.0}
    assert {int(z[f"{n}/side"]) for n in tr} == {16, 32}
    assert any(z[f"{n}/frames"].shape[2] % 2 == 1 for n in tr)                                  # an odd source width
    for n in tr:
        erased = float(z[f"{n}/reprob"]) == 1.0
        top, left, h, w = (int(v) for v in z[f"{n}/ebox"])
        assert (h > 0) == erased and z[f"{n}/noise"].shape == (4, 3, h, w)
    for names in (ce, vi):
        shapes = [z[f"{n}/frames"].shape[1:3] for n in names]
        assert any(h > w for h, w in shapes) and any(h < w for h, w in shapes)                 # portrait and landscape
    assert {int(z[f"{n}/views"]) for n in vi} >= {3} and all(z[f"{n}/ref"].shape[0] == int(z[f"{n}/views"]) for n in vi)


def test_training_draws_equal_the_reference_bit_for_bit():
    """Boxes, flip, erase box and noise of every train case from its seed, the frames untouched, and the three generators left where
    the reference leaves them."""
    from jepa_amd.app.vjepa.transforms import RawClip
    z = U.fixture()
    for n in U.names("train"):
        clip = U.train_clip(n)
        nxt = [random.random(), np.random.uniform(), float(torch.rand(1, dtype=torch.float64))]
        assert isinstance(clip, RawClip) and clip.pre and clip.boxes.dtype == torch.int32
        assert np.array_equal(clip.boxes.numpy(), z[f"{n}/boxes"]), n
        assert clip.flip == bool(z[f"{n}/flip"]), n
        assert list(clip.ebox) == z[f"{n}/ebox"].tolist(), n
        if int(z[f"{n}/ebox"][2]) > 0:
            assert clip.noise.dtype == torch.float32 and np.array_equal(clip.noise.numpy(), z[f"{n}/noise"]), n
        else:
            assert clip.noise is None
        assert clip.frames.dtype == torch.uint8 and np.array_equal(clip.frames.numpy(), z[f"{n}/frames"])      # no pixel work
        assert nxt == z[f"{n}/next"].tolist(), n
        # mean / std: the fp32 values the reference holds, in 0..1 units
        assert clip.mean == tuple(torch.tensor(U.NORMALIZE[0]).tolist()) and clip.std == tuple(torch.tensor(U.NORMALIZE[1]).tolist())


def test_validation_offsets_and_view_starts_equal_the_reference():
    z = U.fixture()
    for n in U.names("centre"):
        clip, S = U.centre_clip(n), int(z[f"{n}/side"])
        y1, x1 = (int(v) for v in z[f"{n}/offsets"])
        assert clip.boxes.shape == (1, 4, 4) and clip.boxes.unique(dim=1).reshape(-1).tolist() == [y1, x1, S, S], n
        assert clip.pre and not clip.flip and clip.noise is None
    for n in U.names("views"):
        clip, S, V = U.views_clip(n), int(z[f"{n}/side"]), int(z[f"{n}/views"])
        H, W = z[f"{n}/frames"].shape[1:3]
        want = [[s, 0, S, S] if H > W else [0, s, S, S] for s in z[f"{n}/starts"].tolist()]
        assert clip.boxes.shape == (V, 4, 4) and clip.num_views == V
        assert all(clip.boxes[v].unique(dim=0).tolist() == [want[v]] for v in range(V)), n
    # Python's rounding of the centre-crop offset: 4.5 -> 4 and 5.5 -> 6
    offs = {tuple(z[f"{n}/frames"].shape[1:3]): z[f"{n}/offsets"].tolist() for n in U.names("centre")}
    assert offs[(25, 18)] == [4, 1] and offs[(18, 27)] == [1, 6]


def test_reprob_zero_consumes_the_generators_exactly_as_before():
    """With reprob == 0 the eval's training transform draws what the pretraining transform draws -- not one call more -- and does
    not touch torch's generator."""
    from jepa_amd.app.vjepa.transforms import VideoTransform as Pretrain
    from jepa_amd.evals.video_classification_frozen.utils import VideoTransform
    frames = np.zeros((4, 40, 56, 3), dtype=np.uint8)
    for shift in (False, True):
        U.seed_all(11)
        state = torch.get_rng_state()
        a = VideoTransform(training=True, reprob=0.0, motion_shift=shift, crop_size=32)(frames)
        after_a = (random.random(), np.random.uniform())
        assert torch.equal(torch.get_rng_state(), state)
        U.seed_all(11)
        b = Pretrain(motion_shift=shift, crop_size=32)(frames)
        assert (random.random(), np.random.uniform()) == after_a
        assert torch.equal(a.boxes, b.boxes) and a.flip == b.flip and a.noise is None and a.ebox == (0, 0, 0, 0)


def test_erase_draw_follows_the_reference_calls():
    """draw_erase on its own: probability 0 consumes one random.random() and nothing else; an erased clip consumes one
    random.random(), two uniforms per try, two randints and one normal_() per frame, in that order."""
    from jepa_amd.app.vjepa.transforms import draw_erase
    U.seed_all(3)
    state = torch.get_rng_state()
    assert draw_erase(0.0, 4, 32, 32) == ((0, 0, 0, 0), None)
    after = random.random()
    random.seed(3)
    random.random()
    assert random.random() == after and torch.equal(torch.get_rng_state(), state)
    U.seed_all(5)
    box, noise = draw_erase(1.0, 2, 64, 64)
    top, left, h, w = box
    assert 0 < h < 64 and 0 < w < 64 and 0 <= top <= 64 - h and 0 <= left <= 64 - w and noise.shape == (2, 3, h, w)
    U.seed_all(5)
    random.random(), random.uniform(0, 1), random.uniform(0, 1), random.randint(0, 64 - h), random.randint(0, 64 - w)
    torch.empty((3, h, w)).normal_(), torch.empty((3, h, w)).normal_()
    nxt = (random.random(), float(torch.rand(1)))
    U.seed_all(5)
    draw_erase(1.0, 2, 64, 64)
    assert (random.random(), float(torch.rand(1))) == nxt


def test_make_transforms_has_the_reference_signature_and_refuses_what_is_out_of_scope():
    from jepa_amd.evals.video_classification_frozen.utils import EvalVideoTransform, VideoTransform, make_transforms
    sig = inspect.signature(make_transforms)
    assert list(sig.parameters) == ["training", "random_horizontal_flip", "random_resize_aspect_ratio", "random_resize_scale", "reprob",
                                    "auto_augment", "motion_shift", "crop_size", "num_views_per_clip", "normalize"]
    d = {k: p.default for k, p in sig.parameters.items()}
    assert d["training"] is True and d["reprob"] == 0.0 and d["auto_augment"] is False and d["num_views_per_clip"] == 1
    assert d["crop_size"] == 224 and d["normalize"] == U.NORMALIZE and d["random_resize_scale"] == (0.3, 1.0)
    assert isinstance(make_transforms(training=False, num_views_per_clip=3), EvalVideoTransform)
    assert isinstance(make_transforms(training=True, num_views_per_clip=3), VideoTransform)
    assert isinstance(make_transforms(training=False), VideoTransform)
    with pytest.raises(NotImplementedError, match="RandAugment"):
        make_transforms(auto_augment=True)
    with pytest.raises(ValueError):
        make_transforms(crop_size=30)
    with pytest.raises(ValueError):
        make_transforms()(np.zeros((4, 8, 8, 3), dtype=np.float32))


def test_a_wrong_short_side_is_refused_with_the_expected_size():
    from jepa_amd.evals.video_classification_frozen.utils import make_transforms
    frames = np.zeros((4, 40, 56, 3), dtype=np.uint8)
    with pytest.raises(ValueError, match=r"short side 36\b.*loader"):
        make_transforms(training=False, crop_size=32)(frames)                   # int(32 * 256 / 224) = 36
    with pytest.raises(ValueError, match=r"short side 32\b.*loader"):
        make_transforms(training=False, crop_size=32, num_views_per_clip=3)(frames)
    make_transforms(training=False, crop_size=32)(np.zeros((4, 36, 56, 3), dtype=np.uint8))
    make_transforms(training=False, crop_size=32, num_views_per_clip=3)(np.zeros((4, 56, 32, 3), dtype=np.uint8))


def test_a_batch_of_three_views_holds_each_clips_bytes_once():
    from jepa_amd.app.vjepa.transforms import RawClipBatch
    from jepa_amd.evals.video_classification_frozen.utils import make_transforms
    tf = make_transforms(training=False, crop_size=16, num_views_per_clip=3)
    g = torch.Generator().manual_seed(2)
    srcs = [torch.randint(0, 256, (4, h, w, 3), generator=g, dtype=torch.uint8) for h, w in ((16, 37), (53, 16))]
    clips = [tf(s) for s in srcs]
    batch = torch.utils.data.default_collate(clips)
    assert isinstance(batch, RawClipBatch) and batch.pre and batch.num_views == 3 and len(batch) == 6 and not batch.erased
    sizes = [s.numel() for s in srcs]
    assert batch.frames.numel() == sum(-(-n // 16) * 16 for n in sizes)         # every byte once (plus alignment), not three times
    for v in range(3):
        for b in range(2):
            r = v * 2 + b                                                       # view-major rows
            assert int(batch.desc[r, 0]) == int(batch.desc[b, 0]) and torch.equal(batch.clip_frames(r), srcs[b])
            assert torch.equal(batch.boxes[r], clips[b].boxes[v])
    # the item layout of the eval's loader: ([RawClip per segment], label, [indices per segment]) -> one batch per segment
    items = [([clips[0], clips[0]], 1, [torch.arange(4), torch.arange(4)]), ([clips[1], clips[1]], 0, [torch.arange(4), torch.arange(4)])]
    segs, labels, idx = torch.utils.data.default_collate(items)
    assert len(segs) == 2 and all(isinstance(s, RawClipBatch) and len(s) == 6 for s in segs) and labels.tolist() == [1, 0]


def _erased_batch(S=16, T=2):
    from jepa_amd.app.vjepa.transforms import RawClip, collate_raw_clips
    frames = torch.zeros(T, 20, 24, 3, dtype=torch.uint8)
    boxes = torch.tensor([[0, 0, 20, 24]] * T, dtype=torch.int32)
    mk = lambda ebox, noise, pre=True: RawClip(frames, boxes, False, S, (0.5,) * 3, (0.25,) * 3, pre=pre, ebox=ebox, noise=noise)   # noqa: E731
    return mk, collate_raw_clips


def test_collated_erase_tables_and_their_validation():
    mk, collate = _erased_batch()
    S, T = 16, 2
    a, b = torch.randn(T, 3, 4, 5), torch.randn(T, 3, 1, 1)
    batch = collate([mk((12, 11, 4, 5), a), mk((0, 0, 0, 0), None), mk((15, 15, 1, 1), b)])       # boxes that END at row / column S
    assert batch.erased and batch.ebox.tolist() == [[12, 11, 4, 5], [0, 0, 0, 0], [15, 15, 1, 1]]
    assert batch.noise_off.tolist() == [0, 0, a.numel()] and batch.noise.numel() == a.numel() + b.numel()
    assert torch.equal(batch.noise[:a.numel()].view(T, 3, 4, 5), a) and torch.equal(batch.noise[a.numel():].view(T, 3, 1, 1), b)
    assert not collate([mk((0, 0, 0, 0), None)]).erased
    # a box that reaches row S or column S (one past the last) is refused
    for bad in ((13, 0, 4, 5), (0, 12, 4, 5), (-1, 0, 4, 5), (0, -1, 4, 5), (0, 0, 17, 1), (0, 0, 4, 0)):
        with pytest.raises(ValueError, match="erase box"):
            collate([mk(bad, torch.randn(T, 3, bad[2], max(bad[3], 0)))])
    # a noise block past the buffer
    for off, drop in ((1, 0), (0, 1), (-1, 0)):
        broken = collate([mk((12, 11, 4, 5), a)])
        broken.noise_off[0] = off
        broken.noise = broken.noise[:broken.noise.numel() - drop]
        with pytest.raises(ValueError, match="noise"):
            broken.validate()
    # mixed normalise-first flags in one batch
    with pytest.raises(ValueError, match="normalise-first"):
        collate([mk((0, 0, 0, 0), None, pre=True), mk((0, 0, 0, 0), None, pre=False)])
    # malformed tables
    broken = collate([mk((12, 11, 4, 5), a)])
    broken.ebox = broken.ebox.to(torch.int64)
    with pytest.raises(ValueError, match="malformed"):
        broken.validate()


def test_restated_device_arithmetic_meets_the_bound_on_every_case():
    """The float32 restatement of vj_clip_transform_pre + vj_clip_erase against the reference's outputs: within the bound on the
    resized training cases (so the reference itself stays inside it), equal bit for bit on the validation crops and inside the
    erased boxes."""
    worst = 0.0
    for n, clip, ref in U.all_cases():
        got = U.restate(clip)
        assert got.shape == ref.shape and got.dtype == np.float32, n
        err = float(np.abs(got - ref).max())
        worst = max(worst, err)
        print(f"restated arithmetic vs reference, case {n}: max abs {err:.3e}")
        assert err <= U.BOUND, (n, err)
        assert float(np.abs(ref).max()) < 2.65 or clip.noise is not None
        if not n.startswith("train"):
            assert np.array_equal(got, ref), n
            for v in range(got.shape[0]):        # and the crop is CPU torch's (u / 255 - m) / s of the same pixels
                i, j, S = int(clip.boxes[v, 0, 0]), int(clip.boxes[v, 0, 1]), clip.crop_size
                plain = U.normalised_plain(clip.frames, clip.mean, clip.std)[:, :, i:i + S, j:j + S]
                assert torch.equal(torch.from_numpy(got[v]), plain), (n, v)
        elif clip.noise is not None:
            t, l, h, w = clip.ebox
            assert np.array_equal(got[0][:, :, t:t + h, l:l + w], ref[0][:, :, t:t + h, l:l + w]), n
    print(f"restated arithmetic vs reference: worst max abs {worst:.3e} (bound {U.BOUND:.0e})")


def test_entry_points_reject_bad_arguments_before_any_launch():
    from jepa_amd.hip.lib import load_library
    lib = load_library()
    norm = (0.485, 0.456, 0.406, 0.229, 0.224, 0.225)
    rc = lib.vj_clip_transform_pre(None, 0, None, None, None, 2, 4, 30, *norm, None)
    assert rc < 0 and b"vj_clip_transform_pre" in lib.vj_last_error() and b"multiple of 4" in lib.vj_last_error()
    rc = lib.vj_clip_transform_pre(None, -1, None, None, None, 2, 4, 32, *norm, None)
    assert rc < 0 and b"bad dims" in lib.vj_last_error()
    rc = lib.vj_clip_transform_pre(None, 0, None, None, None, 2, 4, 32, 0.5, 0.5, 0.5, 1.0, 0.0, 1.0, None)
    assert rc < 0 and b"std" in lib.vj_last_error()
    rc = lib.vj_clip_transform_pre(None, 0, None, None, None, 2, 4, 32, *norm, None)
    assert rc < 0 and b"null pointer" in lib.vj_last_error()
    assert lib.vj_clip_transform_pre(None, 0, None, None, None, 0, 4, 32, *norm, None) == 0       # an empty batch launches nothing
    for B, T, S, n in ((2, 0, 32, 8), (2, 4, 0, 8), (-1, 4, 32, 8), (2, 4, 32, -1), (65536, 4, 32, 8), (2, 4, 1 << 15, 8)):
        rc = lib.vj_clip_erase(None, None, None, n, None, B, T, S, None)
        assert rc < 0 and b"bad dims" in lib.vj_last_error(), (B, T, S, n)
    rc = lib.vj_clip_erase(None, None, None, 8, None, 2, 4, 32, None)
    assert rc < 0 and b"null pointer" in lib.vj_last_error()
    assert lib.vj_clip_erase(None, None, None, 0, None, 2, 4, 32, None) == 0       # no clip of the batch is erased: no launch
    assert lib.vj_clip_erase(None, None, None, 8, None, 0, 4, 32, None) == 0


def test_the_new_ops_have_no_cpu_path():
    from jepa_amd.hip import ops
    batch = torch.utils.data.default_collate([U.train_clip("train_flip_erase")])
    with pytest.raises(ValueError):
        ops.clip_transform(batch.frames, batch.desc, batch.boxes, batch.crop_size, batch.mean, batch.std, pre=True)
    with pytest.raises(ValueError):
        ops.clip_erase(torch.zeros(1, 3, 4, 16, 16), batch.ebox, batch.noise, batch.noise_off)


def test_synthetic_frames_loader_of_the_eval():
    """dataset_type: synthetic_frames -- items in the eval's layout, sources whose short side is what each validation transform
    asks for, the same class patterns in both splits, and `synthetic` untouched next to it."""
    from jepa_amd.app.vjepa.transforms import RawClip, RawClipBatch
    from jepa_amd.evals.video_classification_frozen.eval import make_dataloader
    from jepa_amd.src.datasets.data_manager import SyntheticFramesClassification, SyntheticVideoClassification
    kw = dict(root_path=[None], batch_size=3, world_size=1, rank=0, dataset_type="synthetic_frames", resolution=32, frames_per_clip=4,
              num_segments=2, num_classes=5, synthetic_length=8, num_workers=0)
    tr = make_dataloader(training=True, num_views_per_segment=1, **kw).dataset
    va3 = make_dataloader(training=False, num_views_per_segment=3, **kw).dataset
    va1 = make_dataloader(training=False, num_views_per_segment=1, **kw).dataset
    assert all(isinstance(d, SyntheticFramesClassification) for d in (tr, va3, va1))
    assert tr.transform.reprob == 0.25 and tr.transform.training and not tr.transform.random_horizontal_flip
    assert {min(va3.source_size(i)) for i in range(8)} == {32} and {min(va1.source_size(i)) for i in range(8)} == {36}
    assert len({tr.source_size(i) for i in range(8)}) == 4 and any(h > w for h, w in map(tr.source_size, range(8)))
    U.seed_all(0)
    segs, label, idx = va3[1]
    assert len(segs) == 2 and all(isinstance(c, RawClip) and c.num_views == 3 and c.pre for c in segs) and 0 <= label < 5
    assert len(idx) == 2 and idx[1].tolist() == [16, 20, 24, 28]
    raw, lab = va3.frames_of(1)
    assert lab == label and raw[0].dtype == np.uint8 and raw[0].shape == (4,) + va3.source_size(1) + (3,)
    assert np.array_equal(segs[0].frames.numpy(), raw[0]) and not np.array_equal(raw[0], raw[1])
    # a class's pattern does not depend on the split: per-class mean frames of the two splits correlate
    a, b = tr._pattern(2, 40, 40), va3._pattern(2, 40, 40)
    assert torch.equal(a, b) and a.shape == (4, 40, 40, 3)
    batch = torch.utils.data.default_collate([va3[i] for i in range(3)])
    assert all(isinstance(s, RawClipBatch) and len(s) == 9 for s in batch[0]) and batch[1].shape == (3,)
    kw["dataset_type"] = "synthetic"
    assert isinstance(make_dataloader(training=True, num_views_per_segment=1, **kw).dataset, SyntheticVideoClassification)
