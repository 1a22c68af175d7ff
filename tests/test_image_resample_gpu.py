"""GPU: vj_image_resample against tests/golden/image_resample_micro.npz (Pillow's bytes, tools/make_golden_image_resample.py), the
staged batch of engine.input.ImagePrefetcher against the fixture's reference chain, and both image evals on uint8 images of mixed
sizes.  No tolerance anywhere: uint8 is compared with ==, fp32 bit for bit.  The fixture is all these tests read; Pillow is not needed."""
import random

import numpy as np
import pytest
import torch

from tests.image_resample_util import GOLDEN, load_cases, pack

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _seed(s):
    random.seed(s), np.random.seed(s), torch.manual_seed(s)


@pytest.fixture(scope="module")
def golden():
    z = np.load(GOLDEN)
    return z, load_cases(z)


def _capacities(geoms, S, filt):
    from jepa_amd.evals.image_classification_frozen.transforms import axis_span, axis_taps
    tx = max(axis_taps(int(g[3]), int(g[5]), filt) for g in geoms)
    ty = max(axis_taps(int(g[2]), int(g[4]), filt) for g in geoms)
    rows = max(axis_span(int(g[2]), int(g[4]), filt, int(g[6]), S)[1] for g in geoms)
    return tx, ty, rows


def _run(images, geoms, S, filt):
    """vj_image_resample of one batch -> (uint8 [B,S,S,3] on the host, the frame buffer read back, the buffer as uploaded)."""
    from jepa_amd.hip import ops
    flat, offs = pack(images)
    desc = torch.tensor([[off, im.shape[0], im.shape[1], 0] for im, off in zip(images, offs)], dtype=torch.int64).reshape(-1, 4)
    geom = torch.tensor(np.asarray(geoms, dtype=np.int32).reshape(-1, 8))
    frames = torch.from_numpy(flat).to(DEV)
    out = ops.ImageResample.run(frames, desc.to(DEV), geom.to(DEV), S, filt, *_capacities(geoms, S, filt))
    torch.cuda.synchronize()
    return out.cpu().numpy(), frames.cpu().numpy(), flat


@pytest.mark.parametrize("S", [8, 12])
@pytest.mark.parametrize("filt", [0, 1], ids=["bilinear", "bicubic"])
def test_every_fixture_case_byte_for_byte(golden, S, filt):
    """Cases 1a-1g, one launch each: upscale, reduction, a 25x reduction beside an upscale, an identity axis, crops at the corners
    and of one pixel, 0/255 checkerboards, the validation form."""
    _, cases = golden
    mine = [c for c in cases if c[3] == S and c[4] == filt]
    assert len(mine) == 16
    wrong = []
    for name, src, geom, _, _, want in mine:
        got, after, before = _run([src], [geom], S, filt)
        if not np.array_equal(got[0], want):
            wrong.append((name, int(np.abs(got[0].astype(int) - want).max()), int((got[0] != want).sum())))
        assert np.array_equal(after, before), name
    assert not wrong, wrong


@pytest.mark.parametrize("S", [8, 12])
@pytest.mark.parametrize("filt", [0, 1], ids=["bilinear", "bicubic"])
def test_ragged_batch_in_one_launch(golden, S, filt):
    """Case 1h: all cases of one (S, filter) in ONE batch of mixed shapes; the frame buffer, padding between the images included,
    is unchanged afterwards."""
    _, cases = golden
    mine = [c for c in cases if c[3] == S and c[4] == filt]
    got, after, before = _run([c[1] for c in mine], [c[2] for c in mine], S, filt)
    assert (before == 0xA5).sum() >= 15                               # there is padding to change
    assert np.array_equal(after, before)
    wrong = [c[0] for b, c in enumerate(mine) if not np.array_equal(got[b], c[5])]
    assert not wrong, wrong


def _chain_batch(z, cases):
    from jepa_amd.evals.image_classification_frozen.transforms import RawImage, collate_raw_images
    mean, std = tuple(torch.tensor(z["mean"], dtype=torch.float32).tolist()), tuple(torch.tensor(z["std"], dtype=torch.float32).tolist())
    items = []
    for k, n in enumerate(z["chain_case"]):
        _, src, geom, S, filt, _ = cases[int(n)]
        ebox = tuple(int(v) for v in z["chain_ebox"][k])
        noise = torch.from_numpy(z[f"chain_noise_{k}"]).reshape(1, 3, ebox[2], ebox[3]) if ebox[2] > 0 else None
        items.append(RawImage(torch.from_numpy(src), geom, bool(z["chain_flip"][k]), S, filt, mean, std, ebox=ebox, noise=noise))
    return collate_raw_images(items)


def test_staged_batch_equals_the_reference_chain_bit_for_bit(golden):
    """Case 2: upload, vj_image_resample, vj_clip_transform_pre with identity boxes and the flip flags, vj_clip_erase -- through
    ImagePrefetcher, twice round its two slots -- against ToTensor + Normalize of Pillow's flipped bytes with the noise written in."""
    from jepa_amd.engine.input import ImagePrefetcher
    z, cases = golden
    labels = torch.arange(len(z["chain_case"]))
    pf = ImagePrefetcher([(_chain_batch(z, cases), labels) for _ in range(3)], DEV)
    seen = 0
    for imgs, lab in pf:
        assert imgs.is_cuda and imgs.dtype == torch.float32 and tuple(imgs.shape) == (6, 3, 8, 8) and imgs.is_contiguous()
        got = imgs.cpu().numpy()
        for k in range(6):
            assert np.array_equal(got[k].view(np.uint32), z[f"chain_{k}"].view(np.uint32)), (seen, k)
        assert torch.equal(lab.cpu(), labels)
        seen += 1
    assert seen == 3 and pf.bytes_copied > 0


def test_empty_batch_launches_nothing():
    """Case 3."""
    from jepa_amd.hip import ops
    frames = torch.zeros(16, dtype=torch.uint8, device=DEV)
    out = ops.ImageResample.run(frames, torch.zeros((0, 4), dtype=torch.int64, device=DEV), torch.zeros((0, 8), dtype=torch.int32, device=DEV),
                             8, ops.BICUBIC, 5, 5, 8)
    assert tuple(out.shape) == (0, 8, 8, 3)
    from jepa_amd.hip.lib import load_library
    assert load_library().vj_image_resample(None, 0, None, None, None, 0, 8, 1, 5, 5, 8, None, 0, None) == 0


def test_bad_arguments_are_refused_before_any_launch(golden):
    """Case 4: through the wrapper, on device tensors; and an image whose table is wrong on the device is written as zeros."""
    from jepa_amd.hip import ops
    from jepa_amd.hip.lib import HipKernelError
    _, cases = golden
    f = torch.zeros(1024, dtype=torch.uint8, device=DEV)
    d = torch.tensor([[0, 5, 7, 0]], dtype=torch.int64, device=DEV)
    g = torch.tensor([[0, 0, 5, 7, 8, 8, 0, 0]], dtype=torch.int32, device=DEV)
    with pytest.raises(ValueError, match="multiple of 4"):
        ops.ImageResample.run(f, d, g, 10, ops.BICUBIC, 5, 5, 8)
    with pytest.raises(ValueError, match="expected"):
        ops.ImageResample.run(f, d, g[:, :4].contiguous(), 8, ops.BICUBIC, 5, 5, 8)
    with pytest.raises(HipKernelError, match="filter"):
        ops.ImageResample.run(f, d, g, 8, 7, 5, 5, 8)
    with pytest.raises(ValueError, match="bad dims"):
        ops.ImageResample.run(f, d, g, 8, ops.BICUBIC, 0, 5, 8)
    with pytest.raises(ValueError, match="needed"):
        ops.ImageResample.run(f, d, g, 8, ops.BICUBIC, 5, 5, 8, ws=torch.zeros(64, dtype=torch.uint8, device=DEV))
    with pytest.raises(ValueError, match="is not"):
        ops.ImageResample.run(f, d, g, 8, ops.BICUBIC, 5, 5, 8, out=torch.zeros((1, 8, 8, 4), dtype=torch.uint8, device=DEV))
    # tables that skipped the host's validation: the box leaves the image, the window leaves the resize, the image leaves the buffer,
    # the capacities are too small -- zeros, and the good neighbour is still right
    name, src, geom, S, filt, want = next(c for c in cases if c[0] == "down-S8-bicubic")
    H, W = src.shape[:2]
    flat, offs = pack([src, src, src, src, src])
    desc = torch.tensor([[offs[0], H, W, 0], [offs[1], H, W + 1, 0], [offs[2], H, W, 0], [offs[4], H + 1, W, 0], [offs[3], H, W, 0]],
                        dtype=torch.int64)
    gm = torch.tensor([list(geom), [0, 0, H, W + 2, 8, 8, 0, 0], [0, 0, H, W, 8, 8, 1, 0], list(geom), list(geom)], dtype=torch.int32)
    from jepa_amd.evals.image_classification_frozen.transforms import axis_taps
    tx, ty = axis_taps(W, 8, filt), axis_taps(H, 8, filt)
    out = ops.ImageResample.run(torch.from_numpy(flat).to(DEV), desc.to(DEV), gm.to(DEV), 8, filt, tx, ty, H).cpu().numpy()
    assert np.array_equal(out[0], want) and np.array_equal(out[4], want)
    assert not out[1].any() and not out[2].any() and not out[3].any()
    out = ops.ImageResample.run(torch.from_numpy(flat).to(DEV), desc[:1].to(DEV), gm[:1].to(DEV), 8, filt, tx - 1, ty, H).cpu().numpy()
    assert not out.any()


# ---------------------------------------------------------------------------------------------------------------------- the evals

def _cfg(folder, **over):
    """vit_tiny at resolution 32 on 1024 synthetic_images of two classes, one epoch of 128 iterations of 8 (about a second).  The
    epoch's training top-1 is an average that starts at chance and is taken under the random-resized crop (scale 0.08 .. 1) and
    RandomErasing, so it rises slowly; 1024 items put the standard deviation of a chance-level average at 1.6 points.  Measured on
    MI355X: lone probe 53.9, fine-tuning 53.0, bank (54.8, 53.9); shorter epochs (48 .. 256 items) stayed within a chance-level
    deviation of 50 and are no test of learning."""
    cfg = {
        'pretrain': {'model_name': 'vit_tiny', 'checkpoint_key': 'target_encoder', 'patch_size': 16, 'folder': folder,
                     'checkpoint': 'tiny-latest.pth.tar', 'write_tag': 'tiny', 'tubelet_size': 2, 'frames_per_clip': 8,
                     'uniform_power': True, 'use_sdpa': True, 'use_silu': False, 'tight_silu': False},
        'data': {'dataset_name': 'synthetic_images', 'num_classes': 2, 'root_path': None, 'image_folder': None, 'resolution': 32,
                 'synthetic_length': 1024},
        'optimization': {'batch_size': 8, 'num_epochs': 1, 'weight_decay': 0.01, 'start_lr': 0.001, 'lr': 0.001, 'final_lr': 0.0,
                         'warmup': 0.0, 'use_bfloat16': False},
        'tag': 'uint8_eval',
    }
    for k, v in over.items():
        cfg[k].update(v) if isinstance(v, dict) else cfg.__setitem__(k, v)
    return cfg


def _checkpoint(tmp_path):
    from jepa_amd.src.models import vision_transformer as vit
    torch.manual_seed(1)
    enc = vit.vit_tiny(img_size=32, patch_size=16, num_frames=8, tubelet_size=2, uniform_power=True)
    torch.save({'target_encoder': {'module.backbone.' + k: v for k, v in enc.state_dict().items()}, 'epoch': 10},
               tmp_path / 'tiny-latest.pth.tar')


def _twice(main, cfg):
    recs = []
    for _ in range(2):
        _seed(0)
        recs.append(main(cfg()))
    return recs


def _flat(v):
    return [float(x) for x in np.asarray(v, dtype=np.float64).reshape(-1)]


def test_frozen_eval_on_uint8_images_lone_probe(tmp_path):
    """Case 5: one training and one validation epoch of main on synthetic_images (five source sizes, none square, resolution 32), two
    classes: finite losses, training top-1 above the 50 % of chance, and the same record from a second run with the same seed."""
    from jepa_amd.evals.image_classification_frozen import eval as E
    _checkpoint(tmp_path)
    a, b = _twice(E.main, lambda: _cfg(str(tmp_path)))
    assert len(a['train_history']) == 128 and all(np.isfinite(ls) for _, ls in a['train_history'])
    print("train_acc", a['train_acc'], "val_acc", a['val_acc'])
    assert len(a['train_acc']) == 1 and len(a['val_acc']) == 1 and np.isfinite(a['val_acc'][0])
    assert a['train_acc'][0] > 50.0
    assert a['train_history'] == b['train_history'] and a['train_acc'] == b['train_acc'] and a['val_acc'] == b['val_acc']


def test_frozen_eval_on_uint8_images_probe_bank(tmp_path):
    """Case 5 for a bank of two probes on the one frozen forward."""
    from jepa_amd.evals.image_classification_frozen import eval as E
    _checkpoint(tmp_path)
    heads = {'optimization': {'multihead_kwargs': [
        {'weight_decay': 0.01, 'lr': 0.001, 'start_lr': 0.001, 'final_lr': 0.0, 'warmup': 0.0},
        {'weight_decay': 0.1, 'lr': 0.0005, 'start_lr': 0.0005, 'final_lr': 0.0, 'warmup': 0.0}]}}
    a, b = _twice(E.main, lambda: _cfg(str(tmp_path), **heads))
    print("train_acc", a['train_acc'], "val_acc", a['val_acc'])
    assert len(a['train_acc']) == 1 and len(_flat(a['train_acc'])) == 2 and len(_flat(a['val_acc'])) == 2
    assert np.isfinite(_flat(a['train_acc']) + _flat(a['val_acc'])).all()
    assert np.isfinite(np.asarray([_flat(ls) for _, ls in a['train_history']])).all()
    assert min(_flat(a['train_acc'])) > 50.0
    assert _flat(a['train_acc']) == _flat(b['train_acc']) and _flat(a['val_acc']) == _flat(b['val_acc'])


@pytest.mark.parametrize("mix", [False, True], ids=["plain", "mix"])
def test_finetune_eval_on_uint8_images(tmp_path, mix):
    """Cases 5 and 6: the fine-tuning eval on the same loader, with drop_path, and with `mix` mixing in place in the prefetcher's
    buffers."""
    from jepa_amd.evals.image_classification_finetune import eval as FT
    _checkpoint(tmp_path)
    ft = {'encoder_lr': 0.0001, 'drop_path': 0.1}
    if mix:
        ft['mix'] = {'mixup_alpha': 0.8, 'cutmix_alpha': 1.0, 'prob': 1.0, 'switch_prob': 0.5, 'label_smoothing': 0.1}
    a, b = _twice(FT.main, lambda: _cfg(str(tmp_path), optimization={'finetune': ft}))
    print("train_acc", a['train_acc'], "val_acc", a['val_acc'])
    assert len(a['train_history']) == 128 and all(np.isfinite(ls) for _, ls in a['train_history'])
    assert np.isfinite(a['train_acc'] + a['val_acc']).all()
    if not mix:
        assert a['train_acc'][0] > 50.0
    assert a['train_history'] == b['train_history'] and a['train_acc'] == b['train_acc'] and a['val_acc'] == b['val_acc']
