"""The frozen eval's uint8 input path on the GPU: vj_clip_transform_pre (normalise first, then crop / bilinear resize / flip) and
vj_clip_erase (RandomErasing as a copy) against the reference's transforms (tests/golden/eval_transform_micro.npz,
tools/make_golden_eval_transform.py) and CPU torch, engine/input.py EvalPrefetcher against the direct calls, and `main` on
`dataset_type: synthetic_frames`.

Bound of the resized (training) cases, max abs <= 2e-6: see tests/eval_transform_util.py BOUND.  The validation views are crops
without a resize and the erased boxes are copies: both are compared bit for bit.
Measured on an MI355X: see profiles/eval_uint8_views.md."""
import copy

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from . import eval_transform_util as U

pytestmark = pytest.mark.gpu

DEV = "cuda"


def _collate(clips):
    return torch.utils.data.default_collate(clips)


def _run(batch, erase=True):
    """The direct calls on one RawClipBatch -> fp32 [R,3,T,S,S] on the device."""
    from jepa_amd.hip import ops
    assert batch.pre
    frames, desc, boxes = batch.to(DEV)
    out = ops.clip_transform(frames, desc, boxes, batch.crop_size, batch.mean, batch.std, pre=True)
    if erase and batch.erased:
        ops.clip_erase(out, batch.ebox.to(DEV), batch.noise.to(DEV), batch.noise_off.to(DEV))
    torch.cuda.synchronize()
    return out


def _filler(like):
    """A clip of another source size from the transform constants of `like`, to mix the source sizes of a batch."""
    from jepa_amd.app.vjepa.transforms import RawClip
    T, H, W, _ = like.frames.shape
    V, S = like.num_views, like.crop_size
    g = torch.Generator().manual_seed(H * W)
    frames = torch.randint(0, 256, (T, H + 9, W + 14, 3), generator=g, dtype=torch.uint8)
    boxes = torch.tensor([3, 5, H, W], dtype=torch.int32).repeat(V, T, 1)
    return RawClip(frames, boxes if V > 1 or like.boxes.dim() == 3 else boxes[0], True, S, like.mean, like.std, pre=True)


def test_kernels_match_every_fixture_case_alone_and_in_mixed_batches():
    cases = U.all_cases()
    worst, by_side = 0.0, {}
    for n, clip, ref in cases:
        out = _run(_collate([clip])).cpu().numpy()                                  # alone ...
        assert out.shape == ref.shape, n
        err = float(np.abs(out - ref).max())
        worst = max(worst, err)
        print(f"clip_transform_pre (+ erase) vs reference, case {n}: max abs {err:.3e}")
        assert err <= U.BOUND, (n, err)
        if not n.startswith("train"):
            assert np.array_equal(out, ref), n                                      # a crop: bit for bit
        elif clip.noise is not None:
            t, l, h, w = clip.ebox
            assert np.array_equal(out[0][:, :, t:t + h, l:l + w], clip.noise.numpy().transpose(1, 0, 2, 3)), n
        by_side.setdefault((clip.crop_size, clip.num_views), []).append((n, clip, ref))
    for (side, V), group in by_side.items():                                         # ... and as one batch of mixed source sizes
        clips = [c for _, c, _ in group]
        if len({tuple(c.frames.shape) for c in clips}) < 2:                          # the fixture's cases of this side share a source size
            clips.append(_filler(clips[0]))
        B = len(clips)
        assert B >= 2 and len({tuple(c.frames.shape) for c in clips}) >= 2
        out = _run(_collate(clips)).cpu().numpy()
        assert out.shape[0] == V * B
        for k, (n, clip, ref) in enumerate(group):
            got = out[k::B]                                                          # view-major rows: view v of clip k is row v * B + k
            err = float(np.abs(got - ref).max())
            worst = max(worst, err)
            print(f"clip_transform_pre (+ erase) vs reference, case {n} in a batch of {B} at side {side}: max abs {err:.3e}")
            assert err <= U.BOUND, (n, side, err)
            if not n.startswith("train"):
                assert np.array_equal(got, ref), n
            elif clip.noise is not None:
                t, l, h, w = clip.ebox
                assert np.array_equal(got[0][:, :, t:t + h, l:l + w], clip.noise.numpy().transpose(1, 0, 2, 3)), n
    print(f"clip_transform_pre (+ erase) vs reference: worst max abs {worst:.3e} (bound {U.BOUND:.0e})")


@pytest.mark.parametrize("hw,S,V", [((224, 398), 224, 3), ((398, 224), 224, 3), ((256, 455), 224, 1), ((455, 256), 224, 1)])
def test_validation_views_are_bit_identical_to_cpu_torch(hw, S, V):
    """Full-size validation sources: a 256x455 frame under the centre crop (short side int(224 * 256 / 224) = 256), and what the
    reference's Resize(224) leaves of it, 224x398, under the three-view transform; landscape and portrait.  Every view equals
    CPU torch's (u / 255 - m) / s of the cropped pixels exactly."""
    from jepa_amd.evals.video_classification_frozen.utils import make_transforms
    g = torch.Generator().manual_seed(hw[0] * 1000 + V)
    frames = torch.randint(0, 256, (4,) + hw + (3,), generator=g, dtype=torch.uint8)
    clip = make_transforms(training=False, crop_size=S, num_views_per_clip=V)(frames)
    batch = _collate([clip])
    assert len(batch) == V and batch.frames.numel() == -(-frames.numel() // 16) * 16
    out = _run(batch).cpu()
    plain = U.normalised_plain(frames, clip.mean, clip.std)
    starts = [int(round((max(hw) - S) / 2.))] if V == 1 else [i * ((max(hw) - S) // (V - 1)) for i in range(V)]
    short0 = 0 if V > 1 else int(round((min(hw) - S) / 2.))
    for v, s in enumerate(starts):
        want = plain[:, :, s:s + S, short0:short0 + S] if hw[0] > hw[1] else plain[:, :, short0:short0 + S, s:s + S]
        assert torch.equal(out[v], want), (hw, v)


def _erase_clip(S, ebox, seed, T=3, hw=(20, 27), flip=False):
    from jepa_amd.app.vjepa.transforms import RawClip
    g = torch.Generator().manual_seed(seed)
    frames = torch.randint(0, 256, (T,) + hw + (3,), generator=g, dtype=torch.uint8)
    boxes = torch.tensor([[1, 2, 17, 23]] * T, dtype=torch.int32)
    mean, std = tuple(torch.tensor(U.NORMALIZE[0]).tolist()), tuple(torch.tensor(U.NORMALIZE[1]).tolist())
    noise = None if ebox[2] == 0 else torch.randn(T, 3, ebox[2], ebox[3], generator=g)
    return RawClip(frames, boxes, flip, S, mean, std, pre=True, ebox=ebox, noise=noise)


@pytest.mark.parametrize("S", [16, 32])
def test_erase_writes_the_noise_and_nothing_else(S):
    """Boxes at the top edge, ending at the bottom edge, at the right edge, with left and w not multiples of 4, of one pixel, of
    nearly the whole clip; an erased clip next to one that is not; a batch with none (nothing launched)."""
    boxes = [(0, 3, 5, 6), (S - 7, 1, 7, 3), (2, S - 5, 3, 5), (S - 1, S - 1, 1, 1), (0, 0, 1, 1), (0, 0, S - 1, S - 1), (0, 0, 0, 0),
             (5, 6, 7, 9)]
    clips = [_erase_clip(S, b, 100 + k, flip=bool(k % 2)) for k, b in enumerate(boxes)]
    batch = _collate(clips)
    assert batch.erased and batch.ebox[6].tolist() == [0, 0, 0, 0]
    plain = _run(batch, erase=False).cpu()
    out = _run(batch).cpu()
    for k, (c, (top, left, h, w)) in enumerate(zip(clips, boxes)):
        mask = torch.zeros(S, S, dtype=torch.bool)
        mask[top:top + h, left:left + w] = True
        if h:
            assert torch.equal(out[k][:, :, top:top + h, left:left + w], c.noise.permute(1, 0, 2, 3)), (S, k)
        assert torch.equal(out[k][:, :, ~mask], plain[k][:, :, ~mask]), (S, k)
    none = _collate([_erase_clip(S, (0, 0, 0, 0), 7), _erase_clip(S, (0, 0, 0, 0), 8)])
    assert not none.erased
    a = _run(none, erase=False)
    from jepa_amd.hip import ops
    b = ops.clip_erase(a.clone(), none.ebox.to(DEV), none.noise.to(DEV), none.noise_off.to(DEV))      # empty noise: no launch
    torch.cuda.synchronize()
    assert torch.equal(a, b)


def _eval_batches(S=32, T=4):
    """Three host batches in the eval loader's layout with flat buffers of changing size: training (one view, some clips
    erased), three-view validation, centre-crop validation; two segments each."""
    from jepa_amd.evals.video_classification_frozen.utils import make_transforms
    U.seed_all(21)
    g = torch.Generator().manual_seed(21)
    src = lambda h, w: torch.randint(0, 256, (T, h, w, 3), generator=g, dtype=torch.uint8)   # noqa: E731
    train = make_transforms(training=True, reprob=0.6, crop_size=S, random_resize_scale=(0.08, 1.0))
    views = make_transforms(training=False, crop_size=S, num_views_per_clip=3)
    centre = make_transforms(training=False, crop_size=S)
    short = int(S * 256 / 224)
    plans = [(train, [(40, 56), (90, 70), (33, 47)]), (views, [(S, 57), (61, S)]), (centre, [(short, 64), (50, short), (short, short)])]
    host = []
    for k, (tf, sizes) in enumerate(plans):
        items = [([tf(src(h, w)), tf(src(h, w))], b % 4, [torch.arange(T) * 4, torch.arange(T) * 4 + 16]) for b, (h, w) in enumerate(sizes)]
        host.append(_collate(items))
    return host


def test_eval_prefetcher_returns_what_the_direct_calls_return():
    from jepa_amd.engine.input import EvalPrefetcher
    host = _eval_batches()
    assert len({segs[0].frames.numel() for segs, _, _ in host}) == 3 and any(s.erased for s in host[0][0])
    want = [[_run(s).cpu() for s in segs] for segs, _, _ in host]
    pf = EvalPrefetcher(host, torch.device(DEV))
    assert len(pf) == 3
    busy = torch.randn(4096, 4096, device=DEV)
    for epoch in range(2):
        seen = 0
        for k, (clips, labels, idx) in enumerate(pf):
            segs, lab, ci = host[k]
            first = [[v.clone() for v in seg] for seg in clips]
            for _ in range(3):
                busy = busy @ busy * 1e-3
            again = [[v.clone() for v in seg] for seg in clips]      # after the busy work: the slot must not have been overwritten
            torch.cuda.synchronize()
            assert len(clips) == len(segs) == 2
            for i, raw in enumerate(segs):
                V, B = raw.num_views, len(raw) // raw.num_views
                assert len(clips[i]) == V
                for v in range(V):
                    assert clips[i][v].shape == (B, 3, 4, 32, 32) and clips[i][v].dtype == torch.float32 and clips[i][v].is_cuda
                    assert torch.equal(first[i][v].cpu(), want[k][i][v * B:(v + 1) * B]), (epoch, k, i, v)
                    assert torch.equal(again[i][v].cpu(), want[k][i][v * B:(v + 1) * B]), (epoch, k, i, v)
            assert labels.is_cuda and torch.equal(labels.cpu(), lab) and all(torch.equal(a.cpu(), b) for a, b in zip(idx, ci))
            seen += 1
        assert seen == 3
    raw_bytes = 2 * sum(s.frames.numel() + s.noise.numel() * 4 * s.erased for segs, _, _ in host for s in segs)
    assert raw_bytes < pf.bytes_copied < raw_bytes + 2 * 16 * 1024       # uint8 frames once per clip + noise + the small tables
    with pytest.raises(TypeError):
        next(iter(EvalPrefetcher([([torch.zeros(1)], torch.zeros(1), [torch.zeros(1)])], torch.device(DEV))))


def _views_on_the_cpu(raw):
    """CPU torch: the fp32 views [R,3,T,S,S] of one RawClipBatch, the way the reference makes them (normalise, crop, F.interpolate,
    flip, erase)."""
    S, T, out = raw.crop_size, raw.num_frames, []
    for r in range(len(raw)):
        plain = U.normalised_plain(raw.clip_frames(r), raw.mean, raw.std)
        frames = []
        for t in range(T):
            i, j, h, w = (int(v) for v in raw.boxes[r, t])
            crop = plain[:, t:t + 1, i:i + h, j:j + w]
            frames.append(crop if (h, w) == (S, S) else F.interpolate(crop, size=(S, S), mode='bilinear', align_corners=False))
        x = torch.cat(frames, dim=1)
        if int(raw.desc[r, 3]):
            x = x.flip(-1)
        top, left, h, w = (int(v) for v in raw.ebox[r])
        if h > 0:
            off = int(raw.noise_off[r])
            x = x.clone()
            x[:, :, top:top + h, left:left + w] = raw.noise[off:off + T * 3 * h * w].view(T, 3, h, w).permute(1, 0, 2, 3)
        out.append(x)
    return torch.stack(out)


class _CpuViews:
    """Stands in for EvalPrefetcher: the same loader, every view made on the CPU by torch and handed over as fp32 host tensors
    (the path of `dataset_type: synthetic`)."""

    def __init__(self, loader, device):
        self.loader = loader

    def __len__(self):
        return len(self.loader)

    def __iter__(self):
        for segs, labels, idx in self.loader:
            clips = []
            for raw in segs:
                x, B = _views_on_the_cpu(raw), len(raw) // raw.num_views
                clips.append([x[v * B:(v + 1) * B].contiguous() for v in range(raw.num_views)])
            yield clips, labels, idx


@pytest.mark.parametrize("bank", [False, True])
def test_main_on_uint8_frames_agrees_with_views_made_on_the_cpu(bank, tmp_path, monkeypatch):
    """main() on a micro synthetic_frames config, one training and one validation iteration, single probe and a bank of two:
    finite records, and the training-loss history of the same run fed fp32 views that CPU torch made from the same frames and
    draws, within the 2e-2 relative that tests/test_eval_micro_gpu.py applies to loss records."""
    from tests.test_eval_multihead_gpu import setup_eval
    records = []
    for arm in ("uint8", "cpu"):
        E, cfg = setup_eval("video", str(tmp_path / arm), monkeypatch)
        cfg['data'].update(dataset_type='synthetic_frames', synthetic_length=4, num_views_per_segment=3)
        cfg['optimization'].update(num_epochs=1)
        if bank:
            cfg['optimization']['multihead_kwargs'] = [{'lr': 0.01}, {'lr': 0.003, 'weight_decay': 0.1}]
        if arm == "cpu":
            monkeypatch.setattr(E, "EvalPrefetcher", _CpuViews)
        U.seed_all(0)
        records.append(E.main(copy.deepcopy(cfg)))
        monkeypatch.undo()
    a, b = records
    for rec in records:
        assert len(rec['train_history']) == 1 and len(rec['train_acc']) == 1 and len(rec['val_acc']) == 1
        assert np.isfinite(np.array(rec['train_acc'] + rec['val_acc'], dtype=np.float64)).all()
    la, lb = (np.array([h[1] for h in r['train_history']], dtype=np.float64).reshape(-1) for r in (a, b))
    assert np.isfinite(la).all() and (la > 0).all()
    print(f"training loss, uint8 arm {la.tolist()} vs CPU-view arm {lb.tolist()}")
    assert la.shape == lb.shape == ((2,) if bank else (1,))
    assert (np.abs(la - lb) < 2e-2 * np.abs(lb)).all(), (la, lb)
    assert [h[0] for h in a['train_history']] == [h[0] for h in b['train_history']]
