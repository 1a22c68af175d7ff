"""vj_clip_randaug on the GPU: RandAugment on uint8 frames against what the reference's PIL path made of them
(tests/golden/randaug_micro.npz, tools/make_golden_randaug.py), through engine/input.py EvalPrefetcher to the eval's final fp32
clips, and the video eval's `main` with `data.rand_augment: true`.

The augmented frames are compared with np.array_equal: the arithmetic is integer, fp32 and fp64 with every operation rounded on
its own, as PIL's is, and tests/test_randaug_host.py shows on the CPU that this arithmetic gives PIL's bytes.  The final clips keep
the bound of the eval's resized training cases (tests/eval_transform_util.py BOUND); erased boxes are copies, bit for bit."""
import copy

import numpy as np
import pytest
import torch

from . import eval_transform_util as EU
from . import randaug_util as U

pytestmark = pytest.mark.gpu

DEV = "cuda"
BAND = 4096


def _pack(cases, extra=()):
    """One flat buffer (4 KB bands around it, clips on 16-byte boundaries, padding and bands filled with 0xA5) holding the frames
    of `cases` and of `extra` (frames without a plan) -> (buffer, desc, ops, args, spans)."""
    z = U.fixture()
    clips = [(z[f"{n}/frames"], z[f"{n}/ops"], z[f"{n}/args"]) for n in cases]
    clips += [(f, np.zeros(8, np.int32), np.zeros((8, 6))) for f in extra]
    T = clips[0][0].shape[0]
    offs, total = [], 0
    for f, _, _ in clips:
        assert f.shape[0] == T
        offs.append(total)
        total += -(-f.size // 16) * 16
    buf = torch.full((BAND + total + BAND,), 0xA5, dtype=torch.uint8)
    for (f, _, _), off in zip(clips, offs):
        buf[BAND + off:BAND + off + f.size] = torch.from_numpy(f.reshape(-1))
    desc = torch.tensor([[off, f.shape[1], f.shape[2], 0] for (f, _, _), off in zip(clips, offs)], dtype=torch.int64)
    ops = torch.from_numpy(np.stack([o for _, o, _ in clips]).astype(np.int32))
    args = torch.from_numpy(np.stack([a for _, _, a in clips]).astype(np.float64))
    return buf, desc, ops, args, [(off, f.size) for (f, _, _), off in zip(clips, offs)], total


def _run(buf, desc, ops_t, args_t, total, T):
    """ops.clip_randaug on the middle of `buf` with a banded workspace -> (buffer, workspace with its bands) on the host."""
    from jepa_amd.hip import ops
    dev = buf.to(DEV)
    need = ops.clip_randaug_ws_bytes(total, desc.shape[0], T)
    ws = torch.full((BAND + need + BAND,), 0x5A, dtype=torch.uint8, device=DEV)
    ops.clip_randaug(dev[BAND:BAND + total], desc.to(DEV), T, ops_t.to(DEV), args_t.to(DEV), ws=ws[BAND:BAND + need])
    torch.cuda.synchronize()
    return dev.cpu(), ws.cpu(), need


def _by_frames():
    groups = {}
    for n in U.names():
        groups.setdefault(U.fixture()[f"{n}/frames"].shape[0], []).append(n)
    return groups


def test_every_fixture_case_alone():
    z = U.fixture()
    seen = set()
    for n in U.names():
        buf, desc, ops_t, args_t, spans, total = _pack([n])
        out, _, _ = _run(buf, desc, ops_t, args_t, total, z[f"{n}/frames"].shape[0])
        off, size = spans[0]
        got = out[BAND + off:BAND + off + size].numpy().reshape(z[f"{n}/aug"].shape)
        diff = int((got != z[f"{n}/aug"]).sum())
        print(f"clip_randaug vs reference, case {n} ops {z[f'{n}/ops'].tolist()}: {diff} differing bytes")
        assert np.array_equal(got, z[f"{n}/aug"]), (n, diff)
        seen.update(int(v) for v in z[f"{n}/ops"])
    assert seen == set(range(16))


def test_one_batch_of_all_cases_and_what_must_stay_untouched():
    """Every case of one frame count in one batch (clips of different sizes), with two clips that carry no plan and one row whose
    extent leaves the buffer: equal bytes again; the rows without a plan, the padding between clips, the 4 KB bands around the
    frame buffer and around the workspace keep every byte; a second run gives the same bytes."""
    z = U.fixture()
    rng = np.random.RandomState(5)
    for T, cases in sorted(_by_frames().items()):
        extra = [rng.randint(0, 256, (T, 18, 25, 3)).astype(np.uint8), rng.randint(0, 256, (T, 33, 16, 3)).astype(np.uint8)]
        buf, desc, ops_t, args_t, spans, total = _pack(cases, extra)
        assert len({tuple(z[f"{n}/frames"].shape) for n in cases}) >= 2 and any(size % 16 for _, size in spans)
        # a row with an operation whose clip would end behind the buffer: skipped
        desc = torch.cat([desc, torch.tensor([[(total - 16) // 16 * 16, 50, 50, 0]], dtype=torch.int64)])
        ops_t = torch.cat([ops_t, torch.tensor([[3, 4, 11, 0, 0, 0, 0, 0]], dtype=torch.int32)])
        args_t = torch.cat([args_t, torch.ones((1, 8, 6), dtype=torch.float64)])
        out, ws, need = _run(buf, desc, ops_t, args_t, total, T)
        again, _, _ = _run(buf, desc, ops_t, args_t, total, T)
        assert torch.equal(out, again)
        keep = torch.ones(buf.numel(), dtype=torch.bool)
        for k, n in enumerate(cases):
            off, size = spans[k]
            got = out[BAND + off:BAND + off + size].numpy().reshape(z[f"{n}/aug"].shape)
            assert np.array_equal(got, z[f"{n}/aug"]), (T, n, int((got != z[f"{n}/aug"]).sum()))
            keep[BAND + off:BAND + off + size] = False
        assert torch.equal(out[keep], buf[keep])                      # rows without a plan, padding, both bands
        assert bool((buf[keep] == 0xA5).any()) and int(keep.sum()) >= 2 * BAND + sum(f.size for f in extra)
        assert bool((ws[:BAND] == 0x5A).all()) and bool((ws[BAND + need:] == 0x5A).all())
        print(f"clip_randaug, {len(cases)} cases + 2 plain clips + 1 skipped row of {T} frames in one batch: equal bytes")


def _train_batch():
    """The fixture's train cases through the eval's own transform (RandAugment attribute set, the case's seed) as one host batch."""
    from jepa_amd.app.vjepa.randaugment import RandAugmentDraw
    from jepa_amd.evals.video_classification_frozen.utils import make_transforms
    z = U.fixture()
    clips, names = [], [str(n) for n in z["train_names"]]
    for n in names:
        tf = make_transforms(training=True, reprob=float(z[f"{n}/reprob"]), crop_size=int(z[f"{n}/side"]))
        tf.rand_augment = RandAugmentDraw(str(z[f"{n}/config"]))
        U.seed_all(int(z[f"{n}/seed"]))
        clips.append(tf(z[f"{n}/frames"]))
    return names, clips, torch.utils.data.default_collate(clips)


def test_prefetcher_gives_the_reference_clips():
    """uint8 fixture frames -> EvalPrefetcher (upload, vj_clip_randaug, vj_clip_transform_pre, vj_clip_erase on the copy stream) ->
    fp32 clips against the reference's VideoTransform(training=True, auto_augment=True) output."""
    from jepa_amd.engine.input import EvalPrefetcher
    from jepa_amd.hip import ops
    z = U.fixture()
    names, clips, batch = _train_batch()
    assert batch.augmented and batch.erased and len({tuple(c.frames.shape) for c in clips}) >= 2
    host = [([batch], torch.arange(len(clips)), [torch.arange(4)])] * 3
    calls, real = [], ops.clip_randaug

    def counting(frames, desc, T, aug_ops, aug_args, **kw):
        calls.append(tuple(aug_ops.shape))
        return real(frames, desc, T, aug_ops, aug_args, **kw)

    ops.clip_randaug = counting
    try:
        pf = EvalPrefetcher(host, torch.device(DEV))
        outs = []
        for segs, labels, idx in pf:
            torch.cuda.synchronize()
            outs.append(segs[0][0].cpu().numpy())
        stores = [{k: v.data_ptr() for k, v in d.items() if k[0] == "aug_ws"} for d in pf._dev]
        for segs, labels, idx in pf:                                   # a second epoch allocates no new workspace
            pass
        torch.cuda.synchronize()
        assert stores == [{k: v.data_ptr() for k, v in d.items() if k[0] == "aug_ws"} for d in pf._dev]
    finally:
        ops.clip_randaug = real
    live = int((batch.aug_ops != 0).any(0).sum())
    assert len(calls) == 6 and all(c == (len(clips), live) for c in calls) and live < 8       # only the layers with an operation
    assert np.array_equal(batch.clip_frames(0).numpy(), z[f"{names[0]}/frames"])              # the host batch is not touched
    for out in outs:
        for k, n in enumerate(names):
            ref = z[f"{n}/ref"]
            err = float(np.abs(out[k] - ref).max())
            print(f"prefetcher with RandAugment vs reference, case {n}: max abs {err:.3e} (bound {EU.BOUND:.0e})")
            assert err <= EU.BOUND, (n, err)
            t, l, h, w = (int(v) for v in z[f"{n}/ebox"])
            if h:
                assert np.array_equal(out[k][:, :, t:t + h, l:l + w], z[f"{n}/noise"].transpose(1, 0, 2, 3)), n
    # no operation anywhere: no upload, no launch
    from jepa_amd.app.vjepa.transforms import RawClip
    plain = torch.utils.data.default_collate([RawClip(c.frames, c.boxes, c.flip, c.crop_size, c.mean, c.std, pre=True,
                                                      aug_ops=np.zeros(8, np.int32), aug_args=np.zeros((8, 6))) for c in clips])
    assert plain.aug_ops is not None and not plain.augmented
    ops.clip_randaug = counting
    try:
        pf = EvalPrefetcher([([plain], torch.arange(len(clips)), [torch.arange(4)])], torch.device(DEV))
        before = len(calls)
        for segs, labels, idx in pf:
            pass
        torch.cuda.synchronize()
        assert len(calls) == before and not any(k[0] in ("aug_ops", "aug_args", "aug_ws") for d in pf._dev for k in d)
    finally:
        ops.clip_randaug = real


def test_main_with_rand_augment(tmp_path, monkeypatch):
    """The video eval's main() on the micro config with uint8 frames and `data.rand_augment: true`: two epochs, the same record run
    to run, another record than without the key (which launches nothing of it), and -- the key absent, the config as committed --
    still the committed single-probe record."""
    import json
    from jepa_amd.hip import ops
    from tests.test_eval_multihead_gpu import GOLDEN, setup_eval, single_probe_record
    calls, real = [], ops.clip_randaug

    def counting(*a, **kw):
        calls.append(1)
        return real(*a, **kw)

    monkeypatch.setattr(ops, "clip_randaug", counting)
    records, launched = {}, {}
    for arm, key in (("on_a", True), ("on_b", True), ("off", None)):
        E, cfg = setup_eval("video", str(tmp_path / arm), monkeypatch)
        cfg['data'].update(dataset_type='synthetic_frames')
        if key is not None:
            cfg['data']['rand_augment'] = key
        del calls[:]
        U.seed_all(0)
        rec = E.main(copy.deepcopy(cfg))
        records[arm], launched[arm] = rec, len(calls)
        assert len(rec['train_acc']) == 2 and len(rec['val_acc']) == 2 and len(rec['train_history']) == 8
        assert np.isfinite(np.array([h[1] for h in rec['train_history']], dtype=np.float64)).all()
    losses = {arm: [h[1] for h in rec['train_history']] for arm, rec in records.items()}
    print("training losses with RandAugment", losses["on_a"], "without", losses["off"], "launches", launched)
    assert launched["on_a"] > 0 and launched["on_b"] == launched["on_a"] and launched["off"] == 0
    # run to run at the bound the committed record is held to below (rel 1e-4 on losses); the augmentation must move them by more
    assert losses["on_a"] == pytest.approx(losses["on_b"], rel=1e-4)
    assert records["on_a"]['train_acc'] == pytest.approx(records["on_b"]['train_acc'], abs=1e-3)
    assert records["on_a"]['val_acc'] == pytest.approx(records["on_b"]['val_acc'], abs=1e-3)
    moved = max(abs(a - b) / abs(b) for a, b in zip(losses["on_a"], losses["off"]))
    print(f"largest relative change of a training loss through RandAugment: {moved:.3e}")
    assert moved > 1e-3
    gold = json.load(open(GOLDEN))["video"]
    rec = single_probe_record("video", str(tmp_path / "gold"), monkeypatch)
    assert rec['lrs'] == gold['lrs'] and rec['losses'] == pytest.approx(gold['losses'], rel=1e-4)
    assert rec['train_acc'] == pytest.approx(gold['train_acc'], abs=1e-3) and rec['val_acc'] == pytest.approx(gold['val_acc'], abs=1e-3)
