"""Data-loader factory with the reference's `init_data` signature (src/datasets/data_manager.py:15-91).

The reference's CPU video pipeline (decord decode, clip sampling, augmentation: src/datasets/video_dataset.py,
app/vjepa/transforms.py) sits OUTSIDE the accelerated hot path and needs packages that are not part of this
image; `data='synthetic'` provides the seeded synthetic clip stream used by BASELINE.json's configs and the
tests, and `data='synthetic_frames'` seeded uint8 [T,H,W,3] frame buffers of varying size that go through `transform`
(app/vjepa/transforms.py) the way decoded video does.  `data='frame_folder'` reads real videos stored as folders of frame
images or `.npy` frame arrays (frame_folder.py: the reference's index file, clip sampling and item layout, no decoder).  Any
other dataset type raises with an explanation instead of silently degrading.
"""
import numpy as np
import torch


class SyntheticClips(torch.utils.data.Dataset):
    """Seeded N(0,1) clips in the item layout of the reference's VideoDataset (video_dataset.py:156-184):
    ([clip[3,T,H,W]] * num_clips, label, [frame indices])."""

    def __init__(self, length, num_frames, crop_size, num_clips=1, seed=1234):
        self.length, self.num_frames, self.crop_size, self.num_clips, self.seed = length, num_frames, crop_size, num_clips, seed

    def __len__(self):
        return self.length

    def __getitem__(self, i):
        g = torch.Generator().manual_seed(self.seed + i)
        clips = [torch.randn(3, self.num_frames, self.crop_size, self.crop_size, generator=g)
                 for _ in range(self.num_clips)]
        return clips, 0, [torch.arange(self.num_frames) for _ in range(self.num_clips)]


class SyntheticFrames(torch.utils.data.Dataset):
    """Seeded uint8 frame buffers in the item layout of the reference's VideoDataset (video_dataset.py:156-184):
    ([transform(clip[T,Hs,Ws,3] uint8)] * num_clips, label, [frame indices]).  The source size of item i is
    SIZES[(seed + i) % len(SIZES)]: square, non-square, smaller and larger than the usual crops.  Frames depend on (seed, i)
    alone: a smooth pattern that drifts over time plus noise, so that crops of one clip are correlated like video."""

    SIZES = ((96, 128), (120, 90), (64, 64), (144, 256), (48, 56), (100, 400))

    def __init__(self, length, num_frames, num_clips=1, transform=None, seed=1234):
        self.length, self.num_frames, self.num_clips, self.transform, self.seed = length, num_frames, num_clips, transform, seed

    def __len__(self):
        return self.length

    def source_size(self, i):
        return self.SIZES[(self.seed + i) % len(self.SIZES)]

    def __getitem__(self, i):
        H, W = self.source_size(i)
        g = torch.Generator().manual_seed(self.seed + i)
        clips = []
        for _ in range(self.num_clips):
            f = 1.0 + 3.0 * torch.rand(3, 3, generator=g)
            t = torch.arange(self.num_frames, dtype=torch.float32)[:, None, None, None] / self.num_frames
            y = torch.arange(H, dtype=torch.float32)[None, :, None, None] / H
            x = torch.arange(W, dtype=torch.float32)[None, None, :, None] / W
            wave = torch.cos(6.283185307179586 * (f[0] * t + f[1] * y + f[2] * x))
            noise = torch.randn(self.num_frames, H, W, 3, generator=g)
            clips.append((127.5 + 90.0 * wave + 20.0 * noise).clamp_(0, 255).to(torch.uint8).numpy())
        if self.transform is not None:
            clips = [self.transform(c) for c in clips]
        return clips, 0, [np.arange(self.num_frames) for _ in range(self.num_clips)]


def _label_and_generator(seed, i, num_classes):
    """The label of classification item i of split `seed`, and the item's generator right after that draw."""
    g = torch.Generator().manual_seed((seed * 1_000_003 + i) % (1 << 62))
    return int(torch.randint(0, num_classes, (1,), generator=g)), g


def _class_wave(pattern_seed, label, signal, sizes):
    """The pattern of a class: one plane wave per channel over the axes of extents `sizes` -- (T, H, W) for clips, (H, W) for
    images -- in relative coordinates, with frequency, phase and amplitude drawn from (pattern_seed, label) -> fp32 [3, *sizes]."""
    g = torch.Generator().manual_seed((1 << 62) + pattern_seed * 1_000_003 + label)   # items use seeds < 2^62
    n = len(sizes)
    f = 1.0 + 3.0 * torch.rand(3, n, generator=g)                  # cycles along each axis, per channel
    phase = 6.283185307179586 * torch.rand(3, generator=g)
    amp = signal * (0.5 + torch.rand(3, generator=g))
    per_channel = (3,) + (1,) * n
    arg = None
    for k, size in enumerate(sizes):                               # summed in axis order: the rounding of (t + h) + w
        coord = (torch.arange(size, dtype=torch.float32) / size).reshape((1,) * (k + 1) + (size,) + (1,) * (n - 1 - k))
        term = f[:, k].reshape(per_channel) * coord
        arg = term if arg is None else arg + term
    return amp.reshape(per_channel) * torch.cos(6.283185307179586 * arg + phase.reshape(per_channel))


def _segment_indices(num_segments, frames, frame_step):
    """Frame indices of consecutive segments of `frames` frames, `frame_step` apart: [S] of int64 [frames]."""
    span = frames * frame_step
    return [torch.arange(s * span, (s + 1) * span, frame_step, dtype=torch.int64) for s in range(num_segments)]


class SyntheticVideoClassification(torch.utils.data.Dataset):
    """Seeded labelled clips for the frozen video-classification eval, in the item layout of the reference's VideoDataset
    under the eval transform (video_dataset.py:156-184, evals/video_classification_frozen/utils.py:172-190):
    ([S segments] of [V views] of fp32 [3,T,H,W], label, [S] of int64 frame indices).

    Item i depends on (seed, i) alone: its label is uniform in [0, num_classes) and every view is N(0,1) noise plus the
    pattern of its class.  A class's pattern (a plane wave per channel whose frequency, phase and amplitude are drawn from
    (pattern_seed, label)) does not depend on `seed`, so splits built with different seeds (training / validation) share
    their classes and a probe trained on one split can classify the other.  Item and pattern generators are seeded from
    disjoint ranges."""

    def __init__(self, length, num_classes, frames_per_clip, crop_size, num_segments=1, num_views_per_segment=1,
                 frame_step=4, seed=0, signal=1.0, pattern_seed=0):
        self.length, self.num_classes, self.frames, self.crop = length, num_classes, frames_per_clip, crop_size
        self.S, self.V, self.frame_step, self.seed, self.signal = num_segments, num_views_per_segment, frame_step, seed, signal
        self.pattern_seed = pattern_seed

    def __len__(self):
        return self.length

    def _pattern(self, label):
        return _class_wave(self.pattern_seed, label, self.signal, (self.frames, self.crop, self.crop))

    def __getitem__(self, i):
        label, g = _label_and_generator(self.seed, i, self.num_classes)
        pat = self._pattern(label)
        clips = [[torch.randn(3, self.frames, self.crop, self.crop, generator=g) + pat for _ in range(self.V)]
                 for _ in range(self.S)]
        return clips, label, _segment_indices(self.S, self.frames, self.frame_step)


class SyntheticFramesClassification(torch.utils.data.Dataset):
    """Seeded labelled uint8 frame buffers for the frozen video-classification eval: the decoded-video counterpart of
    SyntheticVideoClassification.  Item layout: ([S segments] of transform(uint8 [T,Hs,Ws,3]), label, [S] of int64 frame indices);
    `transform` is one of the eval's transforms (evals/video_classification_frozen/utils.py make_transforms), which return one
    `RawClip` per segment that carries every spatial view.

    Item i depends on (seed, i) alone.  Its label is uniform in [0, num_classes); its frames are the class pattern of
    SyntheticVideoClassification (the same plane wave per channel, drawn from (pattern_seed, label), laid over the source frame in
    relative coordinates) plus N(0,1) noise, mapped to bytes as 127.5 + 48 * value and clamped.  Source sizes are mixed and follow
    `short_side`: None (training: the transform crops and resizes anything) cycles through sizes around `crop_size` -- landscape,
    portrait, square, wide; a number (validation: the short side the reference's Resize would leave, which the transforms require)
    cycles through landscape and portrait sources of that short side with odd and even long sides."""

    def __init__(self, length, num_classes, frames_per_clip, crop_size, transform, num_segments=1, short_side=None, frame_step=4,
                 seed=0, signal=1.0, pattern_seed=0):
        if transform is None:
            raise ValueError("SyntheticFramesClassification needs the eval's clip transform (make_transforms)")
        self.length, self.num_classes, self.frames, self.crop = length, num_classes, frames_per_clip, crop_size
        self.S, self.frame_step, self.seed, self.signal, self.pattern_seed = num_segments, frame_step, seed, signal, pattern_seed
        self.transform, self.short_side = transform, short_side
        c = crop_size
        if short_side is None:
            self.sizes = ((c * 8 // 7, c * 3 // 2), (c * 3 // 2, c * 9 // 8), (c, c), (c * 5 // 4, c * 2 + 1))
        else:
            s = short_side
            self.sizes = ((s, s * 4 // 3 + 1), (s * 16 // 9, s), (s, s * 16 // 9), (s * 3 // 2 + 1, s))

    def __len__(self):
        return self.length

    def source_size(self, i):
        return self.sizes[(self.seed + i) % len(self.sizes)]

    def _pattern(self, label, H, W):
        return _class_wave(self.pattern_seed, label, self.signal, (self.frames, H, W)).permute(1, 2, 3, 0)

    def frames_of(self, i):
        """(list over segments of uint8 [T,Hs,Ws,3] arrays, label) of item i, before the transform."""
        label, g = _label_and_generator(self.seed, i, self.num_classes)
        H, W = self.source_size(i)
        pat = self._pattern(label, H, W)
        segs = [(127.5 + 48.0 * (torch.randn(self.frames, H, W, 3, generator=g) + pat)).clamp_(0, 255).to(torch.uint8).numpy()
                for _ in range(self.S)]
        return segs, label

    def __getitem__(self, i):
        segs, label = self.frames_of(i)
        return [self.transform(f) for f in segs], label, _segment_indices(self.S, self.frames, self.frame_step)


class SyntheticImageClassification(torch.utils.data.Dataset):
    """Seeded labelled images for the frozen image-classification eval, in the item layout of the reference's image datasets
    under its eval transform (evals/image_classification_frozen/eval.py:286, 404-409): (fp32 [3,H,W], label).

    Item i depends on (seed, i) alone: its label is uniform in [0, num_classes) and the image is N(0,1) noise plus the pattern of
    its class.  A class's pattern (a plane wave per channel whose frequency, phase and amplitude are drawn from
    (pattern_seed, label)) does not depend on `seed`, so the training and validation splits share their classes, as in
    SyntheticVideoClassification.  Item and pattern generators are seeded from disjoint ranges."""

    def __init__(self, length, num_classes, crop_size, seed=0, signal=1.0, pattern_seed=0):
        self.length, self.num_classes, self.crop, self.seed, self.signal = length, num_classes, crop_size, seed, signal
        self.pattern_seed = pattern_seed

    def __len__(self):
        return self.length

    def _pattern(self, label):
        return _class_wave(self.pattern_seed, label, self.signal, (self.crop, self.crop))

    def __getitem__(self, i):
        label, g = _label_and_generator(self.seed, i, self.num_classes)
        return torch.randn(3, self.crop, self.crop, generator=g) + self._pattern(label), label


def init_data(batch_size, transform=None, shared_transform=None, data='ImageNet', collator=None, pin_mem=True,
              num_workers=8, world_size=1, rank=0, root_path=None, image_folder=None, training=True, copy_data=False,
              drop_last=True, tokenize_txt=True, subset_file=None, clip_len=8, frame_sample_rate=2, duration=None,
              num_clips=1, random_clip_sampling=True, allow_clip_overlap=False, filter_short_videos=False,
              filter_long_videos=int(1e9), decode_one_clip=True, datasets_weights=None, persistent_workers=False,
              repeat_wds=False, ipe=300, log_dir=None, crop_size=224, synthetic_length=None):
    kind = str(data).lower()
    if kind == 'frame_folder':
        # real videos as folders of frames / .npy frame arrays (frame_folder.py), with the arguments, the sampler and the loader of
        # the reference's make_videodataset (src/datasets/video_dataset.py:27-88)
        from .frame_folder import FrameFolderVideoDataset
        dataset = FrameFolderVideoDataset(
            data_paths=root_path, datasets_weights=datasets_weights, frames_per_clip=clip_len, frame_step=frame_sample_rate,
            num_clips=num_clips, random_clip_sampling=random_clip_sampling, allow_clip_overlap=allow_clip_overlap,
            filter_short_videos=filter_short_videos, filter_long_videos=filter_long_videos, duration=duration,
            shared_transform=shared_transform, transform=transform)
        sampler = torch.utils.data.distributed.DistributedSampler(dataset, num_replicas=world_size, rank=rank, shuffle=True)
        loader = torch.utils.data.DataLoader(dataset, collate_fn=collator, sampler=sampler, batch_size=batch_size,
                                             drop_last=drop_last, pin_memory=pin_mem, num_workers=num_workers,
                                             persistent_workers=num_workers > 0)
        return loader, sampler
    if kind not in ('synthetic', 'synthetic_frames'):
        raise NotImplementedError(
            f"dataset_type={data!r}: the reference's decord video decoding needs packages that are not available here. "
            "The augmentation is: `transform` (jepa_amd.app.vjepa.transforms.make_transforms) takes a uint8 [T,H,W,3] "
            "buffer per clip and the device does the pixel work, so a loader that yields such buffers through `transform` "
            "in the VideoDataset item layout is all that is needed -- the reference's src/datasets/video_dataset.py does, "
            "unchanged.  Assign its factory to jepa_amd.app.vjepa.train.init_data, or use dataset_type: synthetic / "
            "synthetic_frames")
    length = synthetic_length if synthetic_length is not None else batch_size * world_size * ipe
    if kind == 'synthetic_frames':
        if transform is None:
            raise ValueError("dataset_type: synthetic_frames needs the clip transform (app/vjepa/transforms.py make_transforms)")
        dataset = SyntheticFrames(length, clip_len, num_clips=num_clips, transform=transform)
    else:
        dataset = SyntheticClips(length, clip_len, crop_size, num_clips=num_clips)
    sampler = torch.utils.data.distributed.DistributedSampler(dataset, num_replicas=world_size, rank=rank, shuffle=True)
    loader = torch.utils.data.DataLoader(dataset, collate_fn=collator, sampler=sampler, batch_size=batch_size,
                                         drop_last=drop_last, pin_memory=pin_mem, num_workers=num_workers,
                                         persistent_workers=(num_workers > 0) and persistent_workers)
    return loader, sampler
