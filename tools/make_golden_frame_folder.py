#!/usr/bin/env python
"""Generate tests/golden/frame_folder_micro.npz from the reference's video dataset and validation transforms, on the CPU.

    JEPA_REFERENCE=/path/to/jepa python tools/make_golden_frame_folder.py

Needs Pillow.  Two kinds of records.

Sampling (`sampling/*`).  src/datasets/video_dataset.py is imported as it is, after stand-ins for what it imports and this machine
may lack have been registered: `decord` (a VideoReader with a set length and frame rate whose get_batch(idx).asnumpy() returns the
indices it was asked for, and `cpu`) and, when it is missing, `pandas` (only the constructor reads an index with it, and the
dataset is built over no index).  The real VideoDataset.loadvideo_decord then runs on a dummy file of 1 KiB (it checks
os.path.getsize) under a seeded np.random over a grid of video length, frames per clip, frame step, number of clips, random
sampling, clip overlap, and duration with a frame rate.  Per case: the arguments, the indices [num_clips, fpc] and numpy's global
generator state afterwards (key and position).  The script asserts that the grid reaches the three branches of the sampling,
partition_len == clip_len and a video shorter than one clip.

Pixels (`pixels/*`).  evals/video_classification_frozen/utils.py imports torchvision and the models, so EvalVideoTransform and
VideoTransform are taken out of it with `ast`, as tools/make_golden_eval_transform.py does, with Compose, Resize, CenterCrop and
Normalize of src/datasets/utils/video/transforms.py, the helpers of functional.py and ClipToTensor of volume_transforms.py.  PIL is
the real one here: the frames are handed over as lists of PIL images, so the reference's Resize goes through
Image.resize(BILINEAR) (functional.py:52-67); cv2 is never reached.  Per case: the uint8 source frames, (OH, OW), Pillow's resized
bytes for BILINEAR and for BICUBIC (the second only for the kernel test), the view starts or centre-crop offsets, and the finished
fp32 views [V,3,T,S,S].  One CPU thread, so that a second run reproduces the file bit for bit.
"""
import ast
import itertools
import math
import numbers
import os
import random
import sys
import tempfile
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get("JEPA_REFERENCE", "")
OUT = os.path.join(ROOT, "tests", "golden", "frame_folder_micro.npz")

S = 16
FRAME_SEED = 2718
# name, T, (H, W), expected (OH, OW) after EvalVideoTransform(3, S)'s Resize
VIEW_CASES = (
    ("views_landscape", 3, (23, 41), (16, 28)),
    ("views_portrait", 1, (37, 22), (26, 16)),
    ("views_upscale", 2, (11, 15), (16, 21)),        # a row of 63 bytes
    ("views_ratio4", 2, (97, 64), (24, 16)),         # ratio 4.04: 11 taps
    ("views_square", 2, (20, 20), (16, 16)),         # the views coincide
    ("views_native", 2, (16, 30), (16, 30)),         # no resize
)
# name, T, (H, W), expected (OH, OW) after VideoTransform(training=False, crop_size=S)'s Resize to int(S * 256 / 224) = 18
CENTRE_CASES = (
    ("centre_landscape", 2, (40, 56), (18, 25)),
)
# the sampling grid: video length x (frames per clip, frame step) x clips x random sampling x overlap
LENGTHS = (7, 16, 33, 100)
CLIPS = ((4, 2), (4, 4))
NUM_CLIPS = (1, 2, 3)
# (length, fps, duration, fpc, num_clips): the frame step becomes int(duration * fps / fpc)
DURATION_CASES = ((50, 7.5, 2.0, 4, 2), (90, 30.0, 1.0, 4, 3), (20, 12.0, 3.0, 4, 2))


def _reference_defs(rel_path, names, ns):
    src = open(os.path.join(REF, rel_path)).read()
    body = [n for n in ast.parse(src).body if isinstance(n, (ast.FunctionDef, ast.ClassDef)) and n.name in names]
    assert sorted(n.name for n in body) == sorted(names), (rel_path, names)
    exec(compile(ast.Module(body=body, type_ignores=[]), rel_path, "exec"), ns)
    return [ns[n] for n in names]


class _Reader:
    """decord.VideoReader as loadvideo_decord uses it: a length, a frame rate, seek, and get_batch that hands the indices back."""
    length, fps = 0, None

    def __init__(self, fname, num_threads=-1, ctx=None):
        pass

    def __len__(self):
        return _Reader.length

    def get_avg_fps(self):
        return _Reader.fps

    def seek(self, pos):
        pass

    def get_batch(self, idx):
        return types.SimpleNamespace(asnumpy=lambda: np.array(idx, dtype=np.int64))


def reference_video_dataset():
    sys.modules["decord"] = types.SimpleNamespace(VideoReader=_Reader, cpu=lambda i=0: None)
    try:
        import pandas  # noqa: F401
    except ImportError:
        sys.modules["pandas"] = types.SimpleNamespace()
    sys.path.insert(0, REF)
    try:
        from src.datasets.video_dataset import VideoDataset
    finally:
        sys.path.remove(REF)
    return VideoDataset


def sampling_records(out):
    VideoDataset = reference_video_dataset()
    grid = [(F, fpc, fstp, nc, rnd, ov, None, None) for F, (fpc, fstp), nc, rnd, ov
            in itertools.product(LENGTHS, CLIPS, NUM_CLIPS, (True, False), (False, True))]
    grid += [(F, fpc, 0, nc, True, ov, dur, fps) for (F, fps, dur, fpc, nc), ov in itertools.product(DURATION_CASES, (False, True))]
    args, indices, keys, poss, branches = [], [], [], [], set()
    with tempfile.TemporaryDirectory() as tmp:
        dummy = os.path.join(tmp, "video.mp4")
        with open(dummy, "wb") as f:
            f.write(b"\0" * 1024)
        for n, (F, fpc, fstp, nc, rnd, ov, dur, fps) in enumerate(grid):
            ds = VideoDataset(data_paths=[], frames_per_clip=fpc, frame_step=fstp, num_clips=nc, random_clip_sampling=rnd,
                              allow_clip_overlap=ov, duration=dur)
            _Reader.length, _Reader.fps = F, fps
            seed = 1000 + n
            np.random.seed(seed)
            buffer, clip_indices = ds.loadvideo_decord(dummy)
            state = np.random.get_state()
            idx = np.stack(clip_indices).astype(np.int64)
            assert idx.shape == (nc, fpc) and np.array_equal(buffer, idx.reshape(-1))
            step = fstp if dur is None else int(dur * fps / fpc)
            clip_len, part = int(fpc * step), F // nc
            branches.add("window" if part > clip_len else "overlap" if ov else "pad")
            if part == clip_len:
                branches.add("equal")
            if F < clip_len:
                branches.add("short")
            args.append([F, fpc, fstp, nc, int(rnd), int(ov), seed, -1.0 if dur is None else dur, -1.0 if fps is None else fps])
            indices.append(idx.reshape(-1))
            keys.append(state[1].astype(np.uint32))
            poss.append(state[2])
    assert branches == {"window", "pad", "overlap", "equal", "short"}, branches
    out["sampling/args"] = np.array(args, dtype=np.float64)      # F, fpc, fstp, num_clips, random, overlap, seed, duration, fps
    out["sampling/indices"] = np.concatenate(indices)            # case after case, num_clips * fpc each
    out["sampling/state_key"] = np.stack(keys)
    out["sampling/state_pos"] = np.array(poss, dtype=np.int64)
    print(f"sampling: {len(grid)} cases, branches {sorted(branches)}")


def frames_for(name, T, hw):
    g = torch.Generator().manual_seed(FRAME_SEED + sum(ord(c) for c in name))
    return torch.randint(0, 256, (T, hw[0], hw[1], 3), generator=g, dtype=torch.uint8).numpy()


def pixel_records(out):
    import PIL.Image
    from PIL import Image

    fns = dict(np=np, torch=torch, numbers=numbers, PIL=PIL, cv2=None)
    fnames = ["_is_tensor_clip", "crop_clip", "resize_clip", "get_resize_sizes", "normalize"]
    _reference_defs("src/datasets/utils/video/functional.py", fnames, fns)
    FF = types.SimpleNamespace(**{n: fns[n] for n in fnames})
    vns = dict(torch=torch, np=np, math=math, random=random, numbers=numbers, PIL=PIL, FF=FF)
    vnames = ["Compose", "Resize", "CenterCrop", "Normalize"]
    _reference_defs("src/datasets/utils/video/transforms.py", vnames, vns)
    video_transforms = types.SimpleNamespace(create_random_augment=lambda **k: None, random_resized_crop=None,
                                             random_resized_crop_with_shift=None, **{n: vns[n] for n in vnames})
    cns = dict(np=np, torch=torch, Image=Image)
    _reference_defs("src/datasets/utils/video/volume_transforms.py", ["convert_img", "ClipToTensor"], cns)
    volume_transforms = types.SimpleNamespace(ClipToTensor=cns["ClipToTensor"])
    ens = dict(np=np, torch=torch, transforms=None, video_transforms=video_transforms, volume_transforms=volume_transforms,
               RandomErasing=lambda *a, **k: None, print=lambda *a, **k: None)
    VideoTransform, EvalVideoTransform = _reference_defs("evals/video_classification_frozen/utils.py",
                                                         ["VideoTransform", "EvalVideoTransform"], ens)
    mean = torch.tensor((0.485, 0.456, 0.406))[:, None, None, None]
    std = torch.tensor((0.229, 0.224, 0.225))[:, None, None, None]

    def resized(frames, ohw, resample):
        return np.stack([np.array(Image.fromarray(f).resize((ohw[1], ohw[0]), resample)) for f in frames])

    def finished(u8, y, x):
        """The reference's ClipToTensor + Normalize on the S x S crop at (y, x) of uint8 [T,H,W,3]."""
        v = torch.from_numpy(u8[:, y:y + S, x:x + S].astype(np.float64)).permute(3, 0, 1, 2).float().div(255)
        return v.sub(mean).div(std)

    def record(name, frames, ohw, boxes, views):
        out[f"{name}/frames"] = frames
        out[f"{name}/resize"] = np.array(ohw, dtype=np.int32)
        out[f"{name}/bilinear"] = resized(frames, ohw, Image.BILINEAR)
        out[f"{name}/bicubic"] = resized(frames, ohw, Image.BICUBIC)
        out[f"{name}/boxes"] = np.array(boxes, dtype=np.int32)           # [V,4] = (i, j, S, S) in the resized frames
        out[f"{name}/views"] = torch.stack(views).numpy().copy()
        for (y, x, _, _), v in zip(boxes, views):                        # the recorded bytes are what the reference cropped
            assert torch.equal(v, finished(out[f"{name}/bilinear"], y, x)), name
        print(f"{name}: source {frames.shape[1:3]} -> {tuple(ohw)} boxes {[b[:2] for b in boxes]}")

    for name, T, hw, want in VIEW_CASES:
        frames = frames_for(name, T, hw)
        views = EvalVideoTransform(num_views_per_clip=3, short_side_size=S)([Image.fromarray(f) for f in frames])
        assert len(views) == 3 and all(v.shape == (3, T, S, S) and v.dtype == torch.float32 for v in views)
        ohw = hw if min(hw) == S else FF.get_resize_sizes(hw[0], hw[1], S)
        assert tuple(ohw) == want, (name, ohw)
        step = (max(ohw) - S) // 2
        record(name, frames, ohw, [(i * step, 0, S, S) if ohw[0] > ohw[1] else (0, i * step, S, S) for i in range(3)], views)
    for name, T, hw, want in CENTRE_CASES:
        frames = frames_for(name, T, hw)
        views = VideoTransform(training=False, crop_size=S)([Image.fromarray(f) for f in frames])
        assert len(views) == 1 and views[0].shape == (3, T, S, S) and views[0].dtype == torch.float32
        ohw = FF.get_resize_sizes(hw[0], hw[1], int(S * 256 / 224))
        assert tuple(ohw) == want, (name, ohw)
        record(name, frames, ohw, [(int(round((ohw[0] - S) / 2.)), int(round((ohw[1] - S) / 2.)), S, S)], views)
    out["pixels/view_names"] = np.array([c[0] for c in VIEW_CASES])
    out["pixels/centre_names"] = np.array([c[0] for c in CENTRE_CASES])
    out["pixels/side"] = np.array(S)
    assert any((c[3][1] * 3) % 4 != 0 for c in VIEW_CASES) and any(c[2] == c[3] for c in VIEW_CASES)
    assert any(c[2][0] > c[2][1] for c in VIEW_CASES) and any(c[2][0] < c[3][0] for c in VIEW_CASES)


def main():
    if not REF or not os.path.isfile(os.path.join(REF, "src", "datasets", "video_dataset.py")):
        raise SystemExit("set JEPA_REFERENCE to the root of a facebookresearch/jepa checkout")
    torch.set_num_threads(1)
    out = {}
    sampling_records(out)
    pixel_records(out)
    np.savez_compressed(OUT, **out)
    size = os.path.getsize(OUT)
    assert size < 1_000_000, size
    print(f"wrote {OUT}: {size} bytes")


if __name__ == "__main__":
    main()
