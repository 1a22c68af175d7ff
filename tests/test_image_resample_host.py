"""CPU: the host half of the image evals' input edge.  The numpy oracle of vj_image_resample (tests/image_resample_util.py) against
the Pillow fixture and, where Pillow imports, against Pillow itself; the validation geometry and the training draws; collation and
validation of RawImageBatch; the image_folder dataset; the evals' loader factory; the entry point's host-side argument checks.
Nothing here uses a tolerance: bytes are compared with ==, fp32 bit for bit."""
import random

import numpy as np
import pytest
import torch

from tests.image_resample_util import BICUBIC, BILINEAR, GOLDEN, load_cases, reference_chain, resample, resample_window


def _seed(s):
    random.seed(s), np.random.seed(s), torch.manual_seed(s)


# ------------------------------------------------------------------------------------------------------------------------- oracle

def test_oracle_equals_every_fixture_case():
    z = np.load(GOLDEN)
    cases = load_cases(z)
    assert len(cases) == 64
    for name, src, geom, S, filt, want in cases:
        assert np.array_equal(resample_window(src, geom, S, filt), want), name


def test_oracle_chain_equals_the_fixture_chain_bit_for_bit():
    z = np.load(GOLDEN)
    assert len(z["chain_case"]) == 6 and z["chain_flip"].any() and (z["chain_ebox"][:, 2] > 0).any()
    for k, n in enumerate(z["chain_case"]):
        got = reference_chain(z[f"want_{int(n)}"], bool(z["chain_flip"][k]), z["chain_ebox"][k], z[f"chain_noise_{k}"])
        assert np.array_equal(got.numpy().view(np.uint32), z[f"chain_{k}"].view(np.uint32)), k


def test_oracle_equals_pillow_on_a_seeded_sweep():
    Image = pytest.importorskip("PIL.Image")
    rng = np.random.RandomState(11)
    pairs = 0
    for k in range(60):
        H, W = (int(v) for v in rng.randint(1, 260, 2))
        OH, OW = (int(v) for v in rng.randint(1, 200, 2))
        if k % 4 == 0:
            img = (rng.randint(0, 2, (H, W, 3)) * 255).astype(np.uint8)
        else:
            img = rng.randint(0, 256, (H, W, 3)).astype(np.uint8)
        i, j = int(rng.randint(0, H)), int(rng.randint(0, W))
        h, w = int(rng.randint(1, H - i + 1)), int(rng.randint(1, W - j + 1))
        for filt, pf in ((BILINEAR, Image.BILINEAR), (BICUBIC, Image.BICUBIC)):
            want = np.asarray(Image.fromarray(img).crop((j, i, j + w, i + h)).resize((OW, OH), pf))
            got = resample(np.ascontiguousarray(img[i:i + h, j:j + w]), OH, OW, filt)
            assert np.array_equal(got, want), (H, W, (i, j, h, w), OH, OW, filt)
            pairs += 1
    assert pairs >= 100
    # the window form computes only what it needs and gives the same bytes: the validation form of a 375x500 photograph
    img = rng.randint(0, 256, (375, 500, 3)).astype(np.uint8)
    want = np.asarray(Image.fromarray(img).resize((341, 256), Image.BILINEAR))[16:240, 58:282]
    assert np.array_equal(resample_window(img, (0, 0, 375, 500, 256, 341, 16, 58), 224, BILINEAR), want)


# ----------------------------------------------------------------------------------------------------------------------- geometry

@pytest.mark.parametrize("hw,resize,window", [((375, 500), (256, 341), (16, 58)),      # round(58.5) == 58
                                              ((500, 375), (341, 256), (58, 16)),
                                              ((256, 300), (256, 300), (16, 38)),      # the short side already is R
                                              ((256, 256), (256, 256), (16, 16)),
                                              ((100, 333), (256, 852), (16, 314))])
def test_validation_geometry(hw, resize, window):
    from jepa_amd.evals.image_classification_frozen.transforms import BILINEAR as F, make_transforms
    t = make_transforms(training=False, resolution=224)
    raw = t(np.zeros(hw + (3,), dtype=np.uint8))
    assert raw.geom == (0, 0) + hw + resize + window
    assert raw.filter == F and not raw.flip and raw.noise is None and raw.crop_size == 224


def test_training_draws_stay_inside_and_repeat_with_the_seed():
    from jepa_amd.evals.image_classification_frozen.transforms import BICUBIC as F, make_transforms
    t = make_transforms(training=True, resolution=32)

    def sequence():
        _seed(5)
        out = []
        for k in range(200):
            H, W = 20 + 7 * (k % 9), 33 + 5 * (k % 11)
            raw = t(np.zeros((H, W, 3), dtype=np.uint8))
            out.append((raw.geom, raw.flip, raw.ebox, None if raw.noise is None else raw.noise.clone()))
            i, j, h, w, OH, OW, wy, wx = raw.geom
            assert 0 <= i and 0 <= j and 0 < h and 0 < w and i + h <= H and j + w <= W and (OH, OW, wy, wx) == (32, 32, 0, 0)
            assert raw.filter == F
            top, left, eh, ew = raw.ebox
            if raw.noise is not None:
                assert tuple(raw.noise.shape) == (1, 3, eh, ew) and 0 <= top and top + eh <= 32 and 0 <= left and left + ew <= 32
        return out
    a, b = sequence(), sequence()
    assert [x[:3] for x in a] == [x[:3] for x in b]
    assert all((x[3] is None and y[3] is None) or torch.equal(x[3], y[3]) for x, y in zip(a, b))
    assert any(x[1] for x in a) and not all(x[1] for x in a)                       # flips are drawn
    erased = sum(x[3] is not None for x in a)
    assert 20 <= erased <= 85                                                      # 0.25 of 200: 50 +- 5 sigma (sigma = 6.1)
    assert len({x[0] for x in a}) > 150                                            # boxes vary


# ------------------------------------------------------------------------------------------------------------- collate and validate

def _raw(H=30, W=47, S=8, geom=None, **kw):
    from jepa_amd.evals.image_classification_frozen.transforms import BICUBIC as F, RawImage
    img = torch.arange(H * W * 3, dtype=torch.int64).remainder(251).to(torch.uint8).reshape(H, W, 3)
    return RawImage(img, geom or (0, 0, H, W, S, S, 0, 0), kw.pop("flip", False), S, F, (0.5, 0.5, 0.5), (0.25, 0.25, 0.25), **kw)


def test_collate_packs_images_on_16_byte_boundaries():
    from torch.utils.data import default_collate
    from jepa_amd.evals.image_classification_frozen.transforms import RawImageBatch
    items = [(_raw(5, 7, flip=True), 1), (_raw(30, 47, ebox=(1, 2, 3, 4), noise=torch.ones(1, 3, 3, 4)), 0), (_raw(9, 9), 2)]
    batch, labels = default_collate(items)
    assert isinstance(batch, RawImageBatch) and labels.tolist() == [1, 0, 2] and len(batch) == 3
    assert batch.desc.tolist() == [[0, 5, 7, 1], [112, 30, 47, 0], [112 + 4240, 9, 9, 0]]
    for b, (raw, _) in enumerate(items):
        assert torch.equal(batch.image(b), raw.image)
    assert batch.geom.dtype == torch.int32 and batch.geom[1].tolist() == [0, 0, 30, 47, 8, 8, 0, 0]
    assert batch.erased and batch.ebox.tolist() == [[0, 0, 0, 0], [1, 2, 3, 4], [0, 0, 0, 0]] and batch.noise.numel() == 36
    assert batch.capacities() == (2 * 12 + 1, 2 * 8 + 1, 30)                       # ceil(2 * 47 / 8) = 12, ceil(2 * 30 / 8) = 8
    desc1, boxes1 = batch.resampled_tables()
    assert desc1.tolist() == [[0, 8, 8, 1], [192, 8, 8, 0], [384, 8, 8, 0]] and boxes1.tolist() == [[[0, 0, 8, 8]]] * 3


@pytest.mark.parametrize("what,geom,S", [("box", (0, 0, 31, 47, 8, 8, 0, 0), 8),          # one row too many
                                         ("box", (0, 40, 30, 8, 8, 8, 0, 0), 8),          # leaves on the right
                                         ("box", (-1, 0, 10, 10, 8, 8, 0, 0), 8),
                                         ("window", (0, 0, 30, 47, 12, 18, 5, 0), 8),     # 5 + 8 > 12
                                         ("window", (0, 0, 30, 47, 12, 18, 0, 11), 8),    # 11 + 8 > 18
                                         ("window", (0, 0, 30, 47, 6, 18, 0, 0), 8),      # the resize is smaller than the window
                                         ("multiple of 4", (0, 0, 30, 47, 10, 10, 0, 0), 10)])
def test_collate_refuses_bad_geometry_before_anything_is_copied(monkeypatch, what, geom, S):
    from jepa_amd.evals.image_classification_frozen import transforms as T
    copied = []
    monkeypatch.setattr(T, "pack_buffers", lambda tensors: copied.append(len(tensors)) or (torch.zeros(0, dtype=torch.uint8), []))
    with pytest.raises(ValueError, match=what):
        T.collate_raw_images([_raw(geom=geom, S=S)])
    assert not copied


def test_validate_refuses_offsets_beyond_the_buffer_and_bad_tables():
    from jepa_amd.evals.image_classification_frozen.transforms import collate_raw_images
    good = collate_raw_images([_raw(5, 7), _raw(30, 47)])
    good.validate()
    bad = collate_raw_images([_raw(5, 7), _raw(30, 47)])
    bad.desc[1, 0] = 4096                                                          # 4096 + 4230 bytes leave the 4352-byte buffer
    with pytest.raises(ValueError, match="inside the frame buffer"):
        bad.validate()
    bad = collate_raw_images([_raw(5, 7), _raw(30, 47)])
    bad.desc[1, 0] += 8                                                            # not on a 16-byte boundary
    with pytest.raises(ValueError, match="16-byte"):
        bad.validate()
    bad = collate_raw_images([_raw(5, 7)])
    bad.frames = bad.frames[:-16]
    with pytest.raises(ValueError, match="inside the frame buffer"):
        bad.validate()
    bad = collate_raw_images([_raw(5, 7)])
    bad.ebox[0] = torch.tensor([4, 4, 5, 2], dtype=torch.int32)                    # 4 + 5 > 8
    bad.noise = torch.zeros(30)
    with pytest.raises(ValueError, match="erase box"):
        bad.validate()
    bad = collate_raw_images([_raw(5, 7)])
    bad.filter = 2
    with pytest.raises(ValueError, match="filter"):
        bad.validate()


def test_prefetcher_validates_before_it_copies():
    """The staging function refuses a batch whose tables were changed after collation, before it touches a device."""
    from jepa_amd.engine.input import ImagePrefetcher
    from jepa_amd.evals.image_classification_frozen.transforms import collate_raw_images
    bad = collate_raw_images([_raw(5, 7)])
    bad.geom[0, 2] = 6
    pf = ImagePrefetcher.__new__(ImagePrefetcher)            # no stream, no device: validate comes first
    with pytest.raises(ValueError, match="box"):
        pf._stage_images(0, bad)


# ----------------------------------------------------------------------------------------------------------------------- datasets

def test_synthetic_images_are_mixed_sizes_and_seeded():
    from jepa_amd.src.datasets.image_datasets import SyntheticImages
    ds = SyntheticImages(20, 3, 32, transform=lambda im: im, seed=0)
    sizes = {ds[i][0].shape[:2] for i in range(10)}
    assert len(sizes) == 5 and all(h != w and h % 4 and w % 4 for h, w in sizes)
    a, b = ds[3], SyntheticImages(20, 3, 32, transform=lambda im: im, seed=0)[3]
    assert a[0].dtype == np.uint8 and a[0].shape[2] == 3 and np.array_equal(a[0], b[0]) and a[1] == b[1]
    other = SyntheticImages(20, 3, 32, transform=lambda im: im, seed=1)
    # another split draws other items: item i + 1 of seed 0 and item i of seed 1 have the same size and other pixels
    assert all(ds[i + 1][0].shape == other[i][0].shape and not np.array_equal(ds[i + 1][0], other[i][0]) for i in range(5))
    assert 0 < np.mean([ds[i][0].mean() for i in range(5)]) < 255


def _write_folder(root):
    Image = pytest.importorskip("PIL.Image")
    rng = np.random.RandomState(3)
    written = {}
    for split in ("train", "val"):
        for cls in ("zebra", "ant", "moth"):
            d = root / "imgs" / split / cls
            d.mkdir(parents=True)
            for k in range(2):
                arr = rng.randint(0, 256, (5 + k, 9 - k, 3)).astype(np.uint8)
                Image.fromarray(arr).save(d / f"{k}.png")
                written[(split, cls, k)] = arr
    Image.fromarray(rng.randint(0, 256, (4, 6)).astype(np.uint8)).save(root / "imgs" / "train" / "ant" / "grey.png")
    (root / "imgs" / "train" / "ant" / "notes.txt").write_text("not an image")
    return written


def test_image_folder_reads_sorted_classes_and_rgb_arrays(tmp_path):
    from jepa_amd.src.datasets.image_datasets import ImageFolder
    written = _write_folder(tmp_path)
    ds = ImageFolder(str(tmp_path / "imgs" / "train"))
    assert ds.classes == ["ant", "moth", "zebra"] and len(ds) == 7
    assert [lab for _, lab in ds.samples] == [0, 0, 0, 1, 1, 2, 2]
    img, label = ds[0]
    assert label == 0 and img.dtype == np.uint8 and np.array_equal(img, written[("train", "ant", 0)])
    grey, _ = ds[2]                                                                # convert('RGB') of a greyscale file
    assert grey.shape == (4, 6, 3) and np.array_equal(grey[..., 0], grey[..., 1])
    img, label = ds[5]
    assert label == 2 and np.array_equal(img, written[("train", "zebra", 0)])
    with pytest.raises(FileNotFoundError):
        ImageFolder(str(tmp_path / "nowhere"))


def _check_loaders(name, **extra):
    from jepa_amd.evals.image_classification_frozen import eval as E
    from jepa_amd.evals.image_classification_frozen.transforms import BICUBIC as CUBIC, BILINEAR as LINEAR, RawImageBatch
    kw = dict(batch_size=4, world_size=1, rank=0, resolution=32, num_classes=3, synthetic_length=8)
    for training in (True, False):
        _seed(0)
        loader = E.make_dataloader(dataset_name=name, training=training, **extra, **kw)
        batch, labels = next(iter(loader))
        assert isinstance(batch, RawImageBatch) and len(batch) == 4 and labels.shape == (4,) and batch.crop_size == 32
        assert batch.filter == (CUBIC if training else LINEAR)
        if not training:
            assert (batch.geom[:, 4:6].min(dim=1).values == 36).all() and not batch.erased     # int(32 * 256 / 224) = 36
    return kw


def test_both_evals_loader_factory_takes_synthetic_images():
    """The two image evals share main and make_dataloader: the fine-tuning eval's entry point is the frozen one's with the encoder left
    trainable.  The new name gives loaders of (RawImageBatch, labels) in the training and the validation form."""
    from jepa_amd.evals.image_classification_finetune import eval as FT
    from jepa_amd.evals.image_classification_frozen import eval as E
    assert FT.frozen_eval is E and set(E.UINT8_DATASETS) == {"synthetic_images", "image_folder"}
    _check_loaders("synthetic_images", root_path=None, image_folder=None)
    with pytest.raises(ValueError, match="num_classes"):
        E.make_dataloader(dataset_name="synthetic_images", root_path=None, image_folder=None, batch_size=4, world_size=1, rank=0)


def test_both_evals_loader_factory_takes_image_folder(tmp_path):
    from jepa_amd.evals.image_classification_frozen import eval as E
    _write_folder(tmp_path)
    kw = _check_loaders("image_folder", root_path=str(tmp_path), image_folder="imgs")
    with pytest.raises(ValueError, match="root_path"):
        E.make_dataloader(dataset_name="image_folder", root_path=None, image_folder=None, **kw)
    with pytest.raises(NotImplementedError, match="subset_file"):
        E.make_dataloader(dataset_name="image_folder", root_path=str(tmp_path), image_folder="imgs", subset_file="x.txt", **kw)


# ---------------------------------------------------------------------------------------------------------------------------- ABI

def test_entry_point_rejects_bad_arguments_before_any_launch():
    import ctypes
    from jepa_amd.hip.lib import load_library
    lib = load_library()
    assert lib.vj_image_resample_ws_bytes(2, 8, 25, 17, 30) >= 2 * (2 * 8 * 2 * 4 + 8 * 25 * 4 + 8 * 17 * 4 + 30 * 8 * 3)
    assert lib.vj_image_resample_ws_bytes(2, 8, 25, 17, 30) % 256 == 0
    assert lib.vj_image_resample_ws_bytes(-1, 8, 3, 3, 8) < 0 and lib.vj_image_resample_ws_bytes(1, 8, 0, 3, 8) < 0
    buf = (ctypes.c_uint8 * 4096)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    ok = dict(frames=p, nbytes=1024, desc=p, geom=p, out=p, B=1, S=8, filt=1, tx=5, ty=5, rows=8, ws=p, ws_bytes=4096)

    def call(**over):
        a = dict(ok, **over)
        return lib.vj_image_resample(a["frames"], a["nbytes"], a["desc"], a["geom"], a["out"], a["B"], a["S"], a["filt"], a["tx"], a["ty"],
                                     a["rows"], a["ws"], a["ws_bytes"], None)
    for over, msg in ((dict(S=10), b"multiple of 4"), (dict(S=0), b"bad dims"), (dict(B=-1), b"bad dims"), (dict(B=65536), b"bad dims"),
                      (dict(filt=2), b"filter"), (dict(tx=0), b"capacities"), (dict(rows=0), b"capacities"),
                      (dict(frames=None), b"null pointer"), (dict(geom=None), b"null pointer"), (dict(out=None), b"null pointer"),
                      (dict(ws=None), b"null pointer"), (dict(ws_bytes=64), b"workspace of 64 bytes"), (dict(nbytes=-1), b"bad dims")):
        assert call(**over) < 0 and msg in lib.vj_last_error(), (over, lib.vj_last_error())
    assert call(B=0, frames=None, desc=None, geom=None, out=None, ws=None, ws_bytes=0) == 0      # nothing to do, nothing launched


def test_wrapper_refuses_host_tensors_and_bad_shapes():
    from jepa_amd.hip import ops
    f, d, g = torch.zeros(64, dtype=torch.uint8), torch.zeros((1, 4), dtype=torch.int64), torch.zeros((1, 8), dtype=torch.int32)
    with pytest.raises(ValueError, match="GPU"):
        ops.ImageResample.run(f, d, g, 8, ops.BICUBIC, 5, 5, 8)
    with pytest.raises(TypeError):
        ops.ImageResample.run(f.to(torch.int32), d, g, 8, ops.BICUBIC, 5, 5, 8)
