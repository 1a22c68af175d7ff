"""Real videos without a video decoder: folders of frame images (how SSv2 is distributed and K400 is routinely extracted) or `.npy`
arrays of frames, under the index, the clip sampling and the item layout of the reference's VideoDataset
(src/datasets/video_dataset.py:91-272).  Behaviour restated, never copied.

    index   the reference's index file (video_dataset.py:130-135): a space-delimited csv, one `path label` per row; a list of csvs
            is concatenated.  `path` is a directory of frame image files (sorted by name; the extensions of
            image_datasets.IMG_EXTENSIONS) or a `.npy` file holding uint8 [F,H,W,3]; relative paths resolve against the csv's
            directory.  An optional third column is the video's frame rate, which only `duration` reads.
    clips   loadvideo_decord's arithmetic (video_dataset.py:207-266) with the frame count F in the place of len(vr): `sample_indices`.
            The only draw is np.random.randint(clip_len, partition_len) on numpy's global generator, at the reference's point in
            the reference's order, so a seeded stream gives the reference's indices.
    read    only the sampled frames are opened (PIL.Image.open(...).convert('RGB'); np.load(mmap_mode='r')).
    item    (clips, label, clip_indices): num_clips clips of frames_per_clip frames, uint8 [T,H,W,3], each through `transform`
            (after `shared_transform` on the whole buffer), the label, and the sampled indices per clip.

Not here: the weighted multi-dataset sampler (`datasets_weights` raises), `filter_long_videos` (a file-size test: ignored) and
video container decoding.
"""
import os
import warnings

import numpy as np
import torch

from .image_datasets import IMG_EXTENSIONS


def sample_indices(num_frames, frames_per_clip, frame_step, num_clips, random_clip_sampling=True, allow_clip_overlap=False):
    """The frame indices of `num_clips` clips of a video of `num_frames` frames: a list of int64 [frames_per_clip] arrays.  The
    video is cut into num_clips partitions and clip i comes from partition i (video_dataset.py:223-266):
      partition longer than the clip   a window of clip_len = frames_per_clip * frame_step frames ending at a drawn (or the first
                                       possible) end, sampled by linspace and truncated;
      shorter, no overlap allowed      the partition sampled every frame_step frames, padded with its last frame;
      shorter, overlap allowed         min(clip_len, F) - 1 frames sampled likewise, clips (F - clip_len) // (num_clips - 1) apart."""
    fpc, fstp, F = frames_per_clip, frame_step, num_frames
    clip_len = int(fpc * fstp)
    partition_len = F // num_clips
    clips = []
    for i in range(num_clips):
        if partition_len > clip_len:
            end = np.random.randint(clip_len, partition_len) if random_clip_sampling else clip_len
            start = end - clip_len
            idx = np.clip(np.linspace(start, end, num=fpc), start, end - 1).astype(np.int64) + i * partition_len
        elif not allow_clip_overlap:
            n = partition_len // fstp
            idx = np.concatenate((np.linspace(0, partition_len, num=n), np.ones(fpc - n) * partition_len))
            idx = np.clip(idx, 0, partition_len - 1).astype(np.int64) + i * partition_len
        else:
            sample_len = min(clip_len, F) - 1
            n = sample_len // fstp
            idx = np.concatenate((np.linspace(0, sample_len, num=n), np.ones(fpc - n) * sample_len))
            idx = np.clip(idx, 0, sample_len - 1).astype(np.int64)
            clip_step = (F - clip_len) // (num_clips - 1) if F > clip_len else 0
            idx = idx + i * clip_step
        clips.append(idx)
    return clips


class FrameFolderVideoDataset(torch.utils.data.Dataset):
    """Video classification dataset over frame folders and `.npy` frame arrays, with the reference VideoDataset's constructor
    (video_dataset.py:94-108)."""

    def __init__(self, data_paths, datasets_weights=None, frames_per_clip=16, frame_step=4, num_clips=1, transform=None,
                 shared_transform=None, random_clip_sampling=True, allow_clip_overlap=False, filter_short_videos=False,
                 filter_long_videos=int(10**9), duration=None):
        if datasets_weights is not None:
            raise NotImplementedError("FrameFolderVideoDataset: datasets_weights needs the reference's DistributedWeightedSampler, "
                                      "which is out of scope; concatenate the csvs or pass one dataset")
        self.data_paths = [data_paths] if isinstance(data_paths, str) else list(data_paths)
        self.datasets_weights = None
        self.frames_per_clip, self.frame_step, self.num_clips = frames_per_clip, frame_step, num_clips
        self.transform, self.shared_transform = transform, shared_transform
        self.random_clip_sampling, self.allow_clip_overlap = random_clip_sampling, allow_clip_overlap
        self.filter_short_videos = filter_short_videos
        self.filter_long_videos = filter_long_videos      # a file-size test in the reference: not applied to folders
        self.duration = duration
        self.samples, self.labels, self.fps, self.rows = [], [], [], []
        self.num_samples_per_dataset = []
        for csv in self.data_paths:
            if not str(csv).endswith('.csv'):
                raise ValueError(f"FrameFolderVideoDataset: the index {csv!r} is not a .csv of `path label [fps]` rows")
            base, n = os.path.dirname(os.path.abspath(csv)), 0
            with open(csv) as f:
                for lineno, line in enumerate(f, 1):
                    cols = line.split()
                    if not cols:
                        continue
                    if len(cols) not in (2, 3):
                        raise ValueError(f"{csv}:{lineno}: expected `path label [fps]`, got {line.rstrip()!r}")
                    self.samples.append(cols[0] if os.path.isabs(cols[0]) else os.path.join(base, cols[0]))
                    self.labels.append(int(cols[1]))
                    self.fps.append(float(cols[2]) if len(cols) == 3 else None)
                    self.rows.append(f"{csv}:{lineno}")
                    n += 1
            self.num_samples_per_dataset.append(n)
        self._listing = {}      # folder -> sorted frame files, listed once per worker

    def __len__(self):
        return len(self.samples)

    # -- reading
    @staticmethod
    def load_image(path):
        """The uint8 [H,W,3] array of a frame file."""
        try:
            from PIL import Image
        except ImportError as e:
            raise ImportError("data.dataset_type: frame_folder reads frame image files with PIL (Pillow), which is not installed; "
                              "install Pillow or store the videos as .npy arrays of frames") from e
        with open(path, 'rb') as f:
            return np.array(Image.open(f).convert('RGB'))

    def _frame_files(self, path):
        files = self._listing.get(path)
        if files is None:
            files = self._listing[path] = sorted(f for f in os.listdir(path) if f.lower().endswith(IMG_EXTENSIONS))
        return files

    def _open(self, path):
        """(number of frames, read(indices) -> uint8 [n,H,W,3]) of a video, or (0, None) for one that cannot be read."""
        try:
            if path.endswith('.npy'):
                arr = np.load(path, mmap_mode='r')
                if arr.dtype != np.uint8 or arr.ndim != 4 or arr.shape[-1] != 3:
                    raise ValueError(f"{path}: expected uint8 [F,H,W,3], got {arr.dtype} {arr.shape}")
                return arr.shape[0], lambda idx: np.stack([np.asarray(arr[i]) for i in idx])
            files = self._frame_files(path)
        except OSError:
            return 0, None

        def read(idx):
            cache, shape = {}, None
            for i in idx:             # a padded clip names its last frame many times: every file is opened once
                if i not in cache:
                    cache[i] = self.load_image(os.path.join(path, files[i]))
                    shape = cache[i].shape if shape is None else shape
                    if cache[i].shape != shape:
                        raise ValueError(f"{path}: frame {files[i]} is {cache[i].shape[0]}x{cache[i].shape[1]}, the first sampled "
                                         f"frame {shape[0]}x{shape[1]}: the frames of one video must have one size")
            return np.stack([cache[i] for i in idx])
        return len(files), read

    def load_video(self, index):
        """(uint8 [num_clips * frames_per_clip, H, W, 3], clip indices) of video `index`, or ([], None) when it cannot be used."""
        path = self.samples[index]
        F, read = self._open(path)
        if F == 0:
            warnings.warn(f'video not found, unreadable or without frames: {path}')
            return [], None
        fstp = self.frame_step
        if self.duration is not None:
            if self.fps[index] is None:
                raise ValueError(f"{self.rows[index]}: duration={self.duration} needs the video's frame rate in a third column")
            fstp = int(self.duration * self.fps[index] / self.frames_per_clip)
        if self.filter_short_videos and F < int(self.frames_per_clip * fstp):
            warnings.warn(f'skipping video of length {F}')
            return [], None
        clip_indices = sample_indices(F, self.frames_per_clip, fstp, self.num_clips, self.random_clip_sampling,
                                      self.allow_clip_overlap)
        return read([int(i) for idx in clip_indices for i in idx]), clip_indices

    def __getitem__(self, index):
        # keep drawing until a video loads, as the reference does (video_dataset.py:156-166)
        while True:
            buffer, clip_indices = self.load_video(index)
            if len(buffer) > 0:
                break
            index = np.random.randint(self.__len__())
        label = self.labels[index]
        if self.shared_transform is not None:
            buffer = self.shared_transform(buffer)
        fpc = self.frames_per_clip
        buffer = [buffer[i * fpc:(i + 1) * fpc] for i in range(self.num_clips)]
        if self.transform is not None:
            buffer = [self.transform(clip) for clip in buffer]
        return buffer, label, clip_indices
