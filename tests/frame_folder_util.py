"""What the frame-folder tests share (test_frame_folder_host, test_clip_resample_gpu, test_frame_folder_gpu): the fixture
tests/golden/frame_folder_micro.npz (tools/make_golden_frame_folder.py: the reference's clip sampling and its validation transforms
on PIL frames) and writers of small datasets of PNG frame folders and .npy videos."""
import functools
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "frame_folder_micro.npz")


@functools.lru_cache(maxsize=1)
def fixture():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def view_names():
    return [str(n) for n in fixture()["pixels/view_names"]]


def centre_names():
    return [str(n) for n in fixture()["pixels/centre_names"]]


def case(name):
    """frames uint8 [T,H,W,3], resize (OH, OW), bilinear / bicubic uint8 [T,OH,OW,3], boxes int32 [V,4], views fp32 [V,3,T,S,S]."""
    z = fixture()
    return {k: z[f"{name}/{k}"] for k in ("frames", "resize", "bilinear", "bicubic", "boxes", "views")}


def write_frames(folder, frames, ext=".png"):
    """uint8 [F,H,W,3] -> folder/000000.png ... (lossless), written with Pillow."""
    from PIL import Image
    os.makedirs(folder, exist_ok=True)
    for i, f in enumerate(frames):
        Image.fromarray(np.ascontiguousarray(f)).save(os.path.join(folder, f"{i:06d}{ext}"))
    return folder


def write_index(path, rows):
    """rows of (video path, label[, fps]) -> the space-delimited index file."""
    with open(path, "w") as f:
        for r in rows:
            f.write(" ".join(str(c) for c in r) + "\n")
    return str(path)


def smooth_video(F, H, W, seed):
    """A seeded uint8 [F,H,W,3] video: a drifting wave plus noise."""
    g = np.random.RandomState(seed)
    t, y, x = np.meshgrid(np.arange(F) / F, np.arange(H) / H, np.arange(W) / W, indexing="ij")
    f = 1.0 + 3.0 * g.rand(3, 3)
    wave = np.stack([np.cos(6.283185307179586 * (f[c, 0] * t + f[c, 1] * y + f[c, 2] * x)) for c in range(3)], axis=-1)
    return np.clip(127.5 + 90.0 * wave + 20.0 * g.randn(F, H, W, 3), 0, 255).astype(np.uint8)
