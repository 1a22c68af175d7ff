"""CPU: the frame-folder video dataset (jepa_amd/src/datasets/frame_folder.py), the opt-in device resize of the validation
transforms and the resize table of RawClip / RawClipBatch, against tests/golden/frame_folder_micro.npz: the reference's
VideoDataset.loadvideo_decord over a grid of lengths and clip settings, and its validation transforms on PIL frames."""
import warnings

import numpy as np
import pytest
import torch
from torch.utils.data import default_collate

from jepa_amd.app.vjepa.transforms import RawClipBatch, resample_taps
from jepa_amd.evals.video_classification_frozen.utils import EvalVideoTransform, VideoTransform
from jepa_amd.src.datasets.frame_folder import FrameFolderVideoDataset, sample_indices
from tests.frame_folder_util import case, centre_names, fixture, smooth_video, view_names, write_frames, write_index


# ------------------------------------------------------------------------------------------------ clip sampling
def test_sampling_equals_the_reference_over_the_grid_and_leaves_its_generator_state():
    z = fixture()
    args, flat = z["sampling/args"], z["sampling/indices"]
    at, branches = 0, set()
    for n, (F, fpc, fstp, nc, rnd, ov, seed, dur, fps) in enumerate(args):
        F, fpc, fstp, nc, seed = int(F), int(fpc), int(fstp), int(nc), int(seed)
        if dur >= 0:
            fstp = int(dur * fps / fpc)
        want = flat[at:at + nc * fpc].reshape(nc, fpc)
        at += nc * fpc
        np.random.seed(seed)
        got = sample_indices(F, fpc, fstp, nc, random_clip_sampling=bool(rnd), allow_clip_overlap=bool(ov))
        state = np.random.get_state()
        assert all(g.dtype == np.int64 for g in got)
        assert np.array_equal(np.stack(got), want), (n, args[n].tolist(), np.stack(got).tolist(), want.tolist())
        assert np.array_equal(state[1], z["sampling/state_key"][n]) and state[2] == int(z["sampling/state_pos"][n]), n
        branches.add("window" if F // nc > fpc * fstp else "overlap" if ov else "pad")
    assert at == flat.size and branches == {"window", "pad", "overlap"}


def test_duration_takes_the_frame_step_from_the_rows_frame_rate(tmp_path):
    z = fixture()
    rows = [(n, a) for n, a in enumerate(z["sampling/args"]) if a[7] >= 0 and not a[5]]
    n, (F, fpc, _, nc, _, _, seed, dur, fps) = rows[0]
    video = np.zeros((int(F), 4, 4, 3), dtype=np.uint8)
    video[:, 0, 0, 0] = np.arange(int(F))
    np.save(tmp_path / "v.npy", video)
    index = write_index(tmp_path / "index.csv", [("v.npy", 3, fps)])
    ds = FrameFolderVideoDataset([index], frames_per_clip=int(fpc), frame_step=1, num_clips=int(nc), duration=float(dur))
    np.random.seed(int(seed))
    clips, label, idx = ds[0]
    at = sum(int(a[3] * a[1]) for a in z["sampling/args"][:n])
    want = z["sampling/indices"][at:at + int(nc * fpc)].reshape(int(nc), int(fpc))
    assert label == 3 and np.array_equal(np.stack(idx), want)
    assert [c[:, 0, 0, 0].tolist() for c in clips] == want.tolist()

    no_fps = write_index(tmp_path / "nofps.csv", [("v.npy", 3)])
    with pytest.raises(ValueError, match=r"nofps\.csv:1.*frame rate"):
        FrameFolderVideoDataset([no_fps], frames_per_clip=4, duration=1.0)[0]


# ------------------------------------------------------------------------------------------------ reading
@pytest.fixture()
def dataset_dir(tmp_path):
    """Two PNG folders and one .npy video of different sizes, indexed by two csvs (relative paths)."""
    videos = [smooth_video(20, 12, 18, 1), smooth_video(9, 17, 10, 2), smooth_video(30, 8, 8, 3)]
    write_frames(str(tmp_path / "a" / "vid0"), videos[0])
    write_frames(str(tmp_path / "a" / "vid1"), videos[1])
    np.save(tmp_path / "vid2.npy", videos[2])
    (tmp_path / "a" / "vid0" / "notes.txt").write_text("not a frame")
    one = write_index(tmp_path / "a" / "one.csv", [("vid0", 5), ("vid1", 7)])
    two = write_index(tmp_path / "two.csv", [("vid2.npy", 2)])
    return videos, [one, two]


def test_folders_and_npy_videos_are_read_back_exactly(dataset_dir):
    videos, index = dataset_dir
    ds = FrameFolderVideoDataset(index, frames_per_clip=4, frame_step=2, num_clips=2, allow_clip_overlap=True)
    assert len(ds) == 3 and ds.labels == [5, 7, 2] and ds.num_samples_per_dataset == [2, 1]
    for i, video in enumerate(videos):
        np.random.seed(10 + i)
        want = sample_indices(len(video), 4, 2, 2, allow_clip_overlap=True)
        np.random.seed(10 + i)
        clips, label, idx = ds[i]
        assert label == ds.labels[i] and len(clips) == 2 and len(idx) == 2
        for c, ix, w in zip(clips, idx, want):
            assert np.array_equal(ix, w) and c.dtype == np.uint8 and np.array_equal(c, video[w])


def test_transforms_are_applied_as_in_the_reference(dataset_dir):
    videos, index = dataset_dir
    ds = FrameFolderVideoDataset(index, frames_per_clip=4, frame_step=1, num_clips=2, random_clip_sampling=False,
                                 shared_transform=lambda b: b[:, ::-1], transform=lambda c: ("clip", c))
    clips, _, idx = ds[0]
    assert [c[0] for c in clips] == ["clip", "clip"]
    assert all(np.array_equal(c[1], videos[0][ix][:, ::-1]) for c, ix in zip(clips, idx))


def test_only_the_sampled_files_are_opened(dataset_dir, monkeypatch):
    videos, index = dataset_dir
    opened = []
    real = FrameFolderVideoDataset.load_image
    monkeypatch.setattr(FrameFolderVideoDataset, "load_image", staticmethod(lambda p: (opened.append(p), real(p))[1]))
    ds = FrameFolderVideoDataset(index, frames_per_clip=4, frame_step=2, num_clips=1)
    np.random.seed(0)
    _, _, idx = ds[0]
    assert sorted(opened) == sorted({str(p) for p in opened}) and len(opened) == len(set(idx[0].tolist())) <= 4
    assert sorted(int(p[-10:-4]) for p in opened) == sorted(set(idx[0].tolist()))
    # a short video is padded with its last frame: that file is opened once
    del opened[:]
    ds = FrameFolderVideoDataset(index, frames_per_clip=8, frame_step=2, num_clips=1)
    _, _, idx = ds[1]
    assert len(idx[0]) == 8 and len(opened) == len(set(idx[0].tolist())) < 8


def test_what_is_refused(dataset_dir, tmp_path):
    videos, index = dataset_dir
    with pytest.raises(NotImplementedError, match="datasets_weights"):
        FrameFolderVideoDataset(index, datasets_weights=[0.5, 0.5])
    mixed = write_frames(str(tmp_path / "mixed"), videos[0][:3])
    from PIL import Image
    Image.fromarray(videos[1][0]).save(tmp_path / "mixed" / "000003.png")
    idx = write_index(tmp_path / "mixed.csv", [(mixed, 0)])
    with pytest.raises(ValueError, match="one size"):
        FrameFolderVideoDataset([idx], frames_per_clip=4, frame_step=1, random_clip_sampling=False)[0]
    with pytest.raises(ValueError, match="path label"):
        FrameFolderVideoDataset([write_index(tmp_path / "bad.csv", [("a", 1, 2, 3)])])
    bad = tmp_path / "floats.npy"
    np.save(bad, np.zeros((4, 2, 2, 3), dtype=np.float32))
    with pytest.raises(ValueError, match="uint8"):
        FrameFolderVideoDataset([write_index(tmp_path / "f.csv", [(bad, 0)])], frames_per_clip=2, frame_step=1)[0]


def test_an_empty_or_missing_video_warns_and_another_is_drawn(dataset_dir, tmp_path):
    videos, _ = dataset_dir
    (tmp_path / "empty").mkdir()
    good = write_frames(str(tmp_path / "good"), videos[0])
    index = write_index(tmp_path / "holes.csv", [("empty", 1), ("missing", 2), ("good", 3)])
    ds = FrameFolderVideoDataset([index], frames_per_clip=4, frame_step=2, filter_short_videos=True)
    np.random.seed(0)
    draws = []
    while not draws or draws[-1] != 2:          # what __getitem__ will draw until it hits the readable video
        draws.append(np.random.randint(3))
    np.random.seed(0)
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        clips, label, _ = ds[0]
    assert label == 3 and clips[0].shape == (4, 12, 18, 3) and len(caught) == len(draws)
    assert good and all("empty" in str(w.message) or "missing" in str(w.message) for w in caught)
    # a video shorter than one clip is skipped the same way when filter_short_videos is set
    short = write_index(tmp_path / "short.csv", [("good", 3)])
    with pytest.warns(UserWarning, match="length 20"):
        buffer, idx = FrameFolderVideoDataset([short], frames_per_clip=16, frame_step=2, filter_short_videos=True).load_video(0)
    assert len(buffer) == 0 and idx is None


# ------------------------------------------------------------------------------------------------ transforms and tables
def test_device_resize_gives_the_reference_sizes_boxes_and_view_starts():
    for name in view_names():
        c = case(name)
        t = EvalVideoTransform(num_views_per_clip=3, short_side_size=16)
        assert t.device_resize is False
        t.device_resize = True
        clip = t(c["frames"])
        T, H, W, _ = c["frames"].shape
        native = (H, W) == tuple(c["resize"])
        assert clip.resize == (None if native else tuple(int(v) for v in c["resize"])), name
        assert torch.equal(clip.frames, torch.from_numpy(c["frames"])) and clip.pre and not clip.flip
        assert tuple(clip.boxes.shape) == (3, T, 4)
        assert clip.boxes[:, 0].tolist() == c["boxes"].tolist() and bool((clip.boxes == clip.boxes[:, :1]).all()), name
    for name in centre_names():
        c = case(name)
        t = VideoTransform(training=False, crop_size=16)
        assert t.device_resize is False
        t.device_resize = True
        clip = t(c["frames"])
        assert clip.resize == tuple(int(v) for v in c["resize"]) and clip.boxes[0, 0].tolist() == c["boxes"][0].tolist()


def test_without_device_resize_a_wrong_short_side_is_still_refused():
    frames = case("views_landscape")["frames"]
    with pytest.raises(ValueError, match="short side 16"):
        EvalVideoTransform(num_views_per_clip=3, short_side_size=16)(frames)
    with pytest.raises(ValueError, match="short side 18"):
        VideoTransform(training=False, crop_size=16)(frames)
    t = VideoTransform(training=True, crop_size=16)
    t.device_resize = True                       # the training transform takes any size as it is
    assert t(frames).resize is None


def _batch(names):
    t = EvalVideoTransform(num_views_per_clip=3, short_side_size=16)
    t.device_resize = True
    return default_collate([t(case(n)["frames"][:1]) for n in names])


def test_collate_carries_the_resize_table_and_validate_checks_it():
    names = ["views_landscape", "views_native", "views_portrait"]
    b = _batch(names)
    assert isinstance(b, RawClipBatch) and b.resized and b.rgeom.dtype == torch.int32 and tuple(b.rgeom.shape) == (9, 2)
    assert b.rgeom[:3].tolist() == [[16, 28], [16, 30], [26, 16]] and torch.equal(b.rgeom, b.rgeom[:3].repeat(3, 1))
    rgeom, desc_out, nbytes, caps = b.resample_plan()
    assert rgeom.tolist() == [[16, 28], [16, 30], [26, 16]]
    assert desc_out[:, 0].tolist() == [0, 1344, 2784] * 3 and nbytes == 2784 + 1248 and bool((desc_out[:, 0] % 16 == 0).all())
    assert desc_out[:, 1:3].tolist() == b.rgeom.tolist()
    assert caps == (26, 30, resample_taps(41, 28), resample_taps(37, 26), 37) and resample_taps(97, 24) == 11
    # all clips native: no table, nothing about the batch changes
    native = _batch(["views_native", "views_native"])
    assert native.rgeom is None and not native.resized
    # a box outside the RESIZED extent is refused, as are sizes out of range and views that disagree
    for edit, msg in ((lambda x: x.boxes.__setitem__((0, 0, 1), 13), "leaves its 16x28"),
                      (lambda x: x.rgeom.__setitem__((0, 0), 0), "not positive"),
                      (lambda x: x.rgeom.__setitem__((1, 1), 1 << 15), "not positive"),
                      (lambda x: x.rgeom.__setitem__((3, 1), 29), "share")):
        bad = _batch(names)
        edit(bad)
        with pytest.raises(ValueError, match=msg):
            bad.validate()


# ------------------------------------------------------------------------------------------------ wiring
def test_init_data_and_make_dataloader_accept_frame_folder_and_still_refuse_videodataset(dataset_dir):
    from jepa_amd.app.vjepa.transforms import make_transforms
    from jepa_amd.evals.video_classification_frozen.eval import make_dataloader
    from jepa_amd.src.datasets.data_manager import init_data
    videos, index = dataset_dir
    loader, sampler = init_data(batch_size=2, transform=make_transforms(crop_size=16), data="Frame_Folder", root_path=index,
                                num_workers=0, clip_len=4, frame_sample_rate=1, num_clips=1, pin_mem=False, drop_last=False)
    assert isinstance(loader.dataset, FrameFolderVideoDataset) and isinstance(sampler, torch.utils.data.DistributedSampler)
    clips, labels, idx = next(iter(loader))
    assert isinstance(clips[0], RawClipBatch) and len(clips[0]) == 2 and clips[0].rgeom is None and labels.shape == (2,)
    with pytest.raises(NotImplementedError):
        init_data(batch_size=2, data="VideoDataset", root_path=index)

    kw = dict(root_path=index, batch_size=3, world_size=1, rank=0, resolution=16, frames_per_clip=4, frame_step=1,
              num_segments=2, num_workers=0)
    val = make_dataloader(dataset_type="frame_folder", num_views_per_segment=3, training=False, **kw)
    assert isinstance(val.dataset, FrameFolderVideoDataset) and val.dataset.transform.device_resize and not val.drop_last
    assert val.dataset.allow_clip_overlap and val.dataset.num_clips == 2 and val.dataset.frames_per_clip == 4
    segs, labels, idx = next(iter(val))
    assert len(segs) == 2 and all(isinstance(s, RawClipBatch) and len(s) == 9 and s.num_views == 3 and s.resized for s in segs)
    assert sorted(labels.tolist()) == [2, 5, 7] and len(idx) == 2 and tuple(idx[0].shape) == (3, 4)
    train = make_dataloader(dataset_type="frame_folder", num_views_per_segment=1, training=True, **kw)
    assert not train.dataset.transform.device_resize and next(iter(train))[0][0].rgeom is None
    centre = make_dataloader(dataset_type="frame_folder", num_views_per_segment=1, training=False, **kw)
    assert centre.dataset.transform.device_resize and centre.dataset.transform.short_side_size == 18
    with pytest.raises(NotImplementedError):
        make_dataloader(dataset_type="VideoDataset", num_views_per_segment=1, training=False, num_classes=3, **kw)
    with pytest.raises(NotImplementedError, match="subset_file"):
        make_dataloader(dataset_type="frame_folder", subset_file="x.csv", **kw)
