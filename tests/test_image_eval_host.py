"""CPU checks of the frozen image-classification eval (jepa_amd/evals/image_classification_frozen) and of the host side of the
still-image / position-interpolation entry points (no launch: there is no GPU here)."""
import inspect
import os

import numpy as np
import pytest
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
EVAL_FUNCS = ["main", "run_one_epoch", "load_checkpoint", "load_pretrained", "make_dataloader", "init_model", "init_opt"]


def _fixture():
    return np.load(os.path.join(GOLDEN, "image_eval_micro.npz"))


@pytest.mark.parametrize("name", EVAL_FUNCS)
def test_eval_functions_have_the_reference_parameters(name):
    """Each of the reference file's seven functions exists and its parameters begin with the reference's, in the reference's
    order (recorded by tools/make_golden_image_eval.py); whatever this package adds is optional."""
    from jepa_amd.evals.image_classification_frozen import eval as ev
    ref = [str(p) for p in _fixture()["params/" + name]]
    sig = inspect.signature(getattr(ev, name))
    mine = list(sig.parameters)
    assert mine[:len(ref)] == ref, (name, mine, ref)
    for extra in mine[len(ref):]:
        p = sig.parameters[extra]
        assert p.default is not inspect.Parameter.empty or p.kind is inspect.Parameter.KEYWORD_ONLY, (name, extra)


def test_synthetic_images_have_the_reference_layout():
    from jepa_amd.src.datasets.data_manager import SyntheticImageClassification
    R, C = 32, 7
    ds = SyntheticImageClassification(16, C, R, seed=5)
    img, label = ds[3]
    assert img.shape == (3, R, R) and img.dtype == torch.float32 and isinstance(label, int) and 0 <= label < C
    img2, label2 = ds[3]
    assert label2 == label and torch.equal(img, img2)                      # deterministic per (seed, index)
    assert not torch.equal(ds[4][0], img)
    assert not torch.equal(SyntheticImageClassification(16, C, R, seed=6)[3][0], img)
    labels = [ds[i][1] for i in range(len(ds))]
    assert all(0 <= lb < C for lb in labels) and len(set(labels)) > 1
    batch = torch.utils.data.default_collate([ds[i] for i in range(4)])    # what run_one_epoch reads: data[0], data[1]
    assert batch[0].shape == (4, 3, R, R) and batch[1].shape == (4,) and batch[1].dtype == torch.int64


def test_train_and_validation_images_share_their_classes():
    """The training (seed 0) and validation (seed 1) splits of make_dataloader draw other items but the same class patterns."""
    from jepa_amd.evals.image_classification_frozen.eval import make_dataloader
    kw = dict(dataset_name="synthetic", root_path=None, image_folder=None, batch_size=8, world_size=1, rank=0, resolution=16,
              num_classes=3, synthetic_length=96)
    tr_loader, va_loader = make_dataloader(training=True, **kw), make_dataloader(training=False, **kw)
    tr, va = tr_loader.dataset, va_loader.dataset
    assert len(tr_loader) == 12 and tr.seed != va.seed and not torch.equal(tr[0][0], va[0][0])
    imgs, labels = next(iter(va_loader))
    assert imgs.shape == (8, 3, 16, 16) and labels.shape == (8,)

    def class_means(ds):
        by = {}
        for i in range(len(ds)):
            img, label = ds[i]
            by.setdefault(label, []).append(img.reshape(-1))
        return {k: torch.stack(v).mean(0) for k, v in by.items()}

    mt, mv = class_means(tr), class_means(va)
    assert sorted(mt) == sorted(mv) == [0, 1, 2]
    for k in mt:
        assert float(torch.nn.functional.cosine_similarity(mt[k], mv[k], dim=0)) > 0.8, k
    correct = sum(int(min(mt, key=lambda k: float((va[i][0].reshape(-1) - mt[k]).pow(2).sum())) == va[i][1]) for i in range(len(va)))
    assert correct / len(va) > 0.9, correct


@pytest.mark.parametrize("name", ["ImageNet", "iNat21", "Places205"])
def test_real_image_datasets_raise(name):
    from jepa_amd.evals.image_classification_frozen.eval import make_dataloader
    with pytest.raises(NotImplementedError):
        make_dataloader(dataset_name=name, root_path="/nonexistent", image_folder="x", batch_size=2, world_size=1, rank=0)


def test_new_entry_points_reject_bad_arguments_before_any_launch():
    from jepa_amd.hip.lib import load_library
    lib = load_library()
    # vj_image_pack: sizes not divisible into tubelets, a patch that is no multiple of 8, a K that is not gh*gw without idx
    rc = lib.vj_image_pack(None, None, None, 2, 3, 60, 64, 2, 16, 12, None)
    assert rc < 0 and b"not divisible" in lib.vj_last_error()
    rc = lib.vj_image_pack(None, None, None, 2, 3, 60, 60, 2, 12, 25, None)
    assert rc < 0 and b"multiple of 8" in lib.vj_last_error()
    rc = lib.vj_image_pack(None, None, None, 2, 3, 64, 64, 2, 16, 15, None)
    assert rc < 0 and b"gh*gw" in lib.vj_last_error()
    assert lib.vj_image_pack(None, None, None, 0, 3, 64, 64, 2, 16, 16, None) == 0        # an empty batch launches nothing
    # vj_add_pos_bcast: D % 8
    rc = lib.vj_add_pos_bcast(None, None, None, 2, 16, 4, 60, None)
    assert rc < 0 and b"multiple of 8" in lib.vj_last_error()
    rc = lib.vj_add_pos_bcast(None, None, None, 2, -1, 4, 64, None)
    assert rc < 0 and b"bad dims" in lib.vj_last_error()
    assert lib.vj_add_pos_bcast(None, None, None, 0, 16, 4, 64, None) == 0
    # vj_pos_interp3d: a non-positive output grid, D % 4, an output grid that is not floor(in * scale)
    rc = lib.vj_pos_interp3d(None, None, 4, 4, 4, 64, 0.125, 1.0, 1.0, 0, 4, 4, None)
    assert rc < 0 and b"non-positive output grid" in lib.vj_last_error()
    rc = lib.vj_pos_interp3d(None, None, 4, 4, 4, 64, 1.0, 1.0, -1.0, 4, 4, 4, None)
    assert rc < 0 and b"positive" in lib.vj_last_error()
    rc = lib.vj_pos_interp3d(None, None, 4, 4, 4, 62, 1.0, 1.5, 1.5, 4, 6, 6, None)
    assert rc < 0 and b"multiple of 4" in lib.vj_last_error()
    rc = lib.vj_pos_interp3d(None, None, 4, 4, 4, 64, 1.0, 1.5, 1.5, 4, 6, 7, None)
    assert rc < 0 and b"floor" in lib.vj_last_error()


def test_model_rejects_indivisible_sizes_and_cpu_inputs_on_the_host():
    """Sizes that do not divide into tubelets are a ValueError before any kernel; so is a CPU input (there is no CPU path)."""
    from functools import partial
    from jepa_amd.src.models.vision_transformer import VisionTransformer
    enc = VisionTransformer(img_size=64, patch_size=16, num_frames=8, tubelet_size=2, embed_dim=64, depth=1, num_heads=2,
                            norm_layer=partial(torch.nn.LayerNorm, eps=1e-6))
    for p in enc.parameters():
        p.requires_grad = False
    x = torch.zeros(1, 3, 8, 64, 64)
    assert enc.interpolate_pos_encoding(x, enc.pos_embed) is enc.pos_embed
    assert enc.interpolate_pos_encoding(torch.zeros(1, 3, 64, 64), enc.pos_embed) is enc.pos_embed   # a still image at the native size
    for bad in (torch.zeros(1, 3, 7, 64, 64), torch.zeros(1, 3, 8, 72, 64), torch.zeros(1, 3, 64, 40)):
        with pytest.raises(ValueError):
            enc.interpolate_pos_encoding(bad, enc.pos_embed)
    with pytest.raises(ValueError):
        enc(torch.zeros(1, 3, 64, 64))                                       # CPU tensor
    with pytest.raises(ValueError):
        enc.interpolate_pos_encoding(torch.zeros(1, 3, 8, 96, 96), enc.pos_embed)   # the table is computed on the GPU only


def test_image_eval_fixture_regenerates_its_inputs():
    """tests/golden/image_eval_micro.npz keeps only the seeds and sha256 of its inputs; the CPU generator reproduces them.  The
    recorded classifications all clear the logit tolerance (the condition tools/make_golden_image_eval.py selects the seed by)."""
    from tests.image_eval_golden_util import micro_images, off_native_clips
    z = _fixture()
    B, C, iters, T, crop = (int(x) for x in z["dims"])
    train, train_labels, val, val_labels = micro_images(z)
    assert train.shape == (iters, B, 3, crop, crop) and val.shape == (B, 3, crop, crop)
    assert z["feat"].shape == (B, 64, 64) and z["iter_loss"].shape == (iters + 1,) and z["iter_logits"].shape == (iters + 1, B, C)
    for size in z["sizes"]:
        clips, mask = off_native_clips(z, tuple(int(s) for s in size))
        assert clips.shape[2:] == tuple(int(s) for s in size)
    tol = float(z["logit_tol"])
    labels = [train_labels[k] for k in range(iters)] + [val_labels]
    for lgs, lbs in zip([z["logits0"]] + list(z["iter_logits"]), [val_labels] + labels):
        for lg, lb in zip(torch.from_numpy(lgs).double(), lbs):
            top = int(lg.argmax())
            rival = float(lg[lb]) if top != int(lb) else float(torch.cat([lg[:top], lg[top + 1:]]).max())
            assert float(lg[top]) - rival > 2 * tol * float(lg.norm())
    assert {tuple(int(s) for s in sz) for sz in z["sizes"]} >= {(8, 96, 96), (16, 64, 64), (4, 32, 32), (12, 80, 48)}
