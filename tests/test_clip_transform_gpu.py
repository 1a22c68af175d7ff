"""vj_clip_transform on the GPU (uint8 frames -> crop, bilinear resize, flip, normalise -> fp32 [B,3,T,S,S]) against the reference's
CPU transform (tests/golden/transform_micro.npz, tools/make_golden_transform.py) and CPU torch, the RawClipBatch path of
engine/input.py DevicePrefetcher, and `train.main` on uint8 frames (dataset_type: synthetic_frames).

Bound of the parity checks, max abs <= 1e-5: values stay <= 255 in magnitude through a handful of fp32 roundings of at most
255 * 2^-24 = 1.5e-5 each and are then divided by std * 255 >= 57: a few 1e-7 per rounding.  1e-5 is an order of magnitude over the
7.2e-7 between two CPU formulations of the same arithmetic and an order of magnitude under the 1.3e-4 that a source coordinate
computed with a separately rounded multiply and subtract (instead of one fused multiply-add) produces.
Measured on an MI355X: see profiles/device_clip_transform.md."""
import csv
import os
import random

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
DEV = "cuda"
TOL = 1e-5


def _run(batch):
    from jepa_amd.hip import ops
    frames, desc, boxes = batch.to(DEV)
    out = ops.clip_transform(frames, desc, boxes, batch.crop_size, batch.mean, batch.std)
    torch.cuda.synchronize()
    return out


def _collate(clips):
    return torch.utils.data.default_collate(clips)


def test_kernel_matches_every_fixture_case():
    from jepa_amd.app.vjepa.transforms import VideoTransform
    z = np.load(os.path.join(GOLDEN, "transform_micro.npz"))
    by_side = {}
    for n in (str(n) for n in z["case_names"]):
        seed = int(z[f"{n}/seed"])
        random.seed(seed)
        np.random.seed(seed)
        clip = VideoTransform(motion_shift=bool(z[f"{n}/shift"]), crop_size=int(z[f"{n}/side"]))(z[f"{n}/frames"])
        assert np.array_equal(clip.boxes.numpy(), z[f"{n}/boxes"]) and clip.flip == bool(z[f"{n}/flip"])
        by_side.setdefault(clip.crop_size, []).append((n, clip))
        out = _run(_collate([clip]))[0].cpu()                                  # alone ...
        err = float((out - torch.from_numpy(z[f"{n}/ref"])).abs().max())
        print(f"clip_transform vs reference, case {n}: max abs {err:.3e}")
        assert err <= TOL, (n, err)
    for side, group in by_side.items():                                         # ... and as one batch of mixed source sizes
        out = _run(_collate([c for _, c in group])).cpu()
        for k, (n, _) in enumerate(group):
            err = float((out[k] - torch.from_numpy(z[f"{n}/ref"])).abs().max())
            print(f"clip_transform vs reference, case {n} in a batch of {len(group)}: max abs {err:.3e}")
            assert err <= TOL, (n, side, err)


def _torch_reference(clip):
    """F.interpolate(bilinear, align_corners=False) of each frame's crop, flip(-1), (x - mean) / std: CPU torch, fp32."""
    import torch.nn.functional as F
    S = clip.crop_size
    x = clip.frames.to(torch.float32).permute(3, 0, 1, 2)          # [3,T,H,W]
    out = torch.zeros(3, x.shape[1], S, S)
    for t, (i, j, h, w) in enumerate(clip.boxes.tolist()):
        out[:, t:t + 1] = F.interpolate(x[:, t:t + 1, i:i + h, j:j + w], size=(S, S), mode="bilinear", align_corners=False)
    if clip.flip:
        out = out.flip(-1)
    mean, std = torch.tensor(clip.mean, dtype=torch.float32), torch.tensor(clip.std, dtype=torch.float32)
    return (out - mean[:, None, None, None]) / std[:, None, None, None]


@pytest.mark.parametrize("hw", [(720, 1280), (1080, 1920)])
@pytest.mark.parametrize("shift", [False, True])
def test_large_sources_match_cpu_torch(hw, shift):
    from jepa_amd.app.vjepa.transforms import VideoTransform
    torch.set_num_threads(min(torch.get_num_threads(), 16))
    seed = hw[0] + int(shift)
    random.seed(seed)
    np.random.seed(seed)
    g = torch.Generator().manual_seed(seed)
    vt = VideoTransform(crop_size=224, motion_shift=shift)
    clips = [vt(torch.randint(0, 256, (4, hw[0], hw[1], 3), generator=g, dtype=torch.uint8)) for _ in range(2)]
    clips[1].flip = not clips[0].flip                                           # one of each
    out = _run(_collate(clips)).cpu()
    for k, c in enumerate(clips):
        err = float((out[k] - _torch_reference(c)).abs().max())
        print(f"clip_transform vs CPU torch, source {hw} shift {shift} flip {c.flip} box {c.boxes[0].tolist()}: max abs {err:.3e}")
        assert err <= TOL, (hw, shift, k, err)


def test_whole_frame_box_reproduces_the_normalised_pixels():
    """h = w = S, unflipped: every lambda is 0 and the output is (pixel - mean) / std, within 2 ulp."""
    from jepa_amd.app.vjepa.transforms import RawClip, make_transforms
    S, T = 64, 3
    vt = make_transforms(crop_size=S)
    g = torch.Generator().manual_seed(11)
    frames = torch.randint(0, 256, (T, S, S, 3), generator=g, dtype=torch.uint8)
    boxes = torch.tensor([[0, 0, S, S]] * T, dtype=torch.int32)
    out = _run(_collate([RawClip(frames, boxes, False, S, vt.mean, vt.std)]))[0].cpu()
    mean, std = torch.tensor(vt.mean, dtype=torch.float32), torch.tensor(vt.std, dtype=torch.float32)
    want = (frames.to(torch.float32).permute(3, 0, 1, 2) - mean[:, None, None, None]) / std[:, None, None, None]
    ulp = torch.maximum(want.abs(), torch.tensor(2.0 ** -126)).log2().floor().exp2() * 2.0 ** -23
    worst = float(((out - want).abs() / ulp).max())
    print(f"whole-frame box: worst error {worst:.2f} ulp")
    assert worst <= 2.0, worst


def _raw_batches(n, B, T, S, num_clips, seed=9):
    from jepa_amd.app.vjepa.transforms import VideoTransform
    random.seed(seed)
    np.random.seed(seed)
    g = torch.Generator().manual_seed(seed)
    vt = [VideoTransform(crop_size=S), VideoTransform(crop_size=S, motion_shift=True)]
    sizes = [(40, 56), (90, 70), (33, 47), (128, 200), (64, 64), (25, 100), (150, 90)]
    host = []
    for k in range(n):
        raws = []
        for c in range(num_clips):
            clips = []
            for b in range(B):
                h, w = sizes[(3 * k + 2 * c + b) % len(sizes)]
                clips.append(vt[(k + b) % 2](torch.randint(0, 256, (T, h, w, 3), generator=g, dtype=torch.uint8)))
            raws.append(_collate(clips))
        host.append((raws, [torch.randint(0, 50, (B, 5 + k), generator=g)], [torch.randint(0, 50, (B, 9), generator=g)]))
    return host


@pytest.mark.parametrize("num_clips", [1, 2])
def test_prefetcher_runs_the_transform_on_raw_batches(num_clips):
    """RawClipBatches of changing source sizes (so a flat buffer that changes size every batch) through depth-2 slots while the
    compute stream is busy: every clip tensor bit-identical to ops.clip_transform on that batch, in torch.cat order over
    num_clips; masks as on the fp32 path (batch-repeated like train.py:398-406)."""
    from jepa_amd.engine.input import DevicePrefetcher
    from jepa_amd.src.utils.tensors import repeat_interleave_batch
    n, B, T, S = 6, 3, 4, 32
    host = _raw_batches(n, B, T, S, num_clips)
    assert len({raws[0].frames.numel() for raws, _, _ in host}) >= 4
    want = [torch.cat([_run(r) for r in raws], dim=0).cpu() for raws, _, _ in host]
    it = iter(host)
    pf = DevicePrefetcher(lambda: next(it), torch.device(DEV), batch_size=B, num_clips=num_clips, depth=2)
    busy = torch.randn(4096, 4096, device=DEV)
    for k in range(n):
        clips, me, mp = pf.next()
        first = clips.clone()
        for _ in range(3):
            busy = busy @ busy * 1e-3
        again = clips.clone()                    # after the busy work: the slot must not have been overwritten
        torch.cuda.synchronize()
        assert clips.shape == (B * num_clips, 3, T, S, S) and clips.dtype == torch.float32
        assert torch.equal(first.cpu(), want[k]) and torch.equal(again.cpu(), want[k]), k
        assert torch.equal(me[0].cpu(), repeat_interleave_batch(host[k][1][0], B, repeat=num_clips))
        assert torch.equal(mp[0].cpu(), repeat_interleave_batch(host[k][2][0], B, repeat=num_clips))
    raw_bytes = sum(r.frames.numel() for raws, _, _ in host for r in raws)
    assert raw_bytes < pf.bytes_copied < raw_bytes + 64 * 1024       # the uint8 frames + the small tables and masks, nothing else
    with pytest.raises(StopIteration):
        pf.next()


def test_prefetcher_refuses_a_bad_box_before_copying():
    from jepa_amd.engine.input import DevicePrefetcher
    host = _raw_batches(1, 2, 4, 32, 1)
    host[0][0][0].boxes[1, 2, 2] = 10_000
    it = iter(host)
    pf = DevicePrefetcher(lambda: next(it), torch.device(DEV), batch_size=2)
    with pytest.raises(ValueError):
        pf.next()
    assert pf.bytes_copied == 0


def _frames_args(folder, motion_shift):
    from tests.test_train_loop_gpu import tiny_args
    args = tiny_args(folder, epochs=2)
    args['data']['dataset_type'] = 'synthetic_frames'
    args['data_aug'] = {'random_resize_aspect_ratio': [0.75, 1.35], 'random_resize_scale': [0.3, 1.0], 'motion_shift': motion_shift,
                        'reprob': 0.0, 'auto_augment': False}
    args['optimization']['ipe'] = 3
    return args


def _losses(path):
    with open(path) as f:
        rows = list(csv.DictReader(f))
    return [(r['epoch'], r['itr'], r['loss'], r['loss-jepa'], r['reg-loss']) for r in rows]


@pytest.mark.parametrize("motion_shift", [False, True])
def test_main_trains_on_uint8_frames(tmp_path, motion_shift):
    from jepa_amd.app.vjepa.train import main
    runs = []
    for name in ("a", "b"):
        folder = str(tmp_path / name)
        main(_frames_args(folder, motion_shift))
        rows = _losses(os.path.join(folder, 'jepa_r0.csv'))
        assert len(rows) == 6
        assert all(np.isfinite(float(r[2])) and float(r[2]) > 0 for r in rows)
        ck = torch.load(os.path.join(folder, 'jepa-latest.pth.tar'), map_location='cpu')
        assert ck['epoch'] == 2 and 'module.backbone.blocks.0.attn.qkv.weight' in ck['encoder']
        runs.append(rows)
    assert runs[0] == runs[1]                    # seeded draws, seeded frames: the same run twice


def test_out_of_scope_augmentations_raise_from_main(tmp_path):
    from jepa_amd.app.vjepa.train import main
    for key, val in (('auto_augment', True), ('reprob', 0.25)):
        args = _frames_args(str(tmp_path), False)
        args['data_aug'][key] = val
        with pytest.raises(NotImplementedError):
            main(args)
