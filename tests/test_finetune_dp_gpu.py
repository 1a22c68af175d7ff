"""GPU: data-parallel encoder fine-tuning (engine.finetune.EncoderFineTuner with world_size > 1, engine.dp.GradReducer on
dp.finetune_bucket_plan, the two fine-tuning evals on two ranks).

Two ranks are two spawned processes on cuda:0 with a gloo group (the form of tests/test_dp_gpu.py).  Exactly two: a two-term fp32
sum does not depend on the order of its terms, so the reduced gradient arena is the sum of the ranks' own arenas bit for bit and
every comparison below is torch.equal or structural -- no tolerance anywhere.  The micro encoder (D = 64, 8 x 64 x 64), the probe
and the clips are those of tests/finetune_util.py.  The gloo group has a one-minute timeout, so a mismatched collective raises; the
parent joins with a limit, kills a child that is still alive and fails, and retries nothing."""
import os
import queue
import socket
import sys
import time
from datetime import timedelta

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

pytestmark = pytest.mark.gpu
LR, WD, CLIP = 1e-3, 0.05, 1.0
LABELS = ([3, 7], [1, 4])


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _spawn(target, world, *args, limit=200):
    """`world` processes running target(rank, world, port, q, *args); each reports (rank, result) through the queue, a traceback
    string standing for a failure.  -> {rank: result}.  A child alive after the limit is killed and the test fails."""
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=target, args=(r, world, port, q) + args) for r in range(world)]
    for p in procs:
        p.start()
    msgs, deadline, hung = {}, time.monotonic() + limit, []
    try:
        while len(msgs) < world and time.monotonic() < deadline:
            try:
                rank, m = q.get(timeout=1.0)
            except queue.Empty:
                if not any(p.is_alive() for p in procs) and q.empty():
                    break       # a child died without a word
                continue
            msgs[rank] = m
    finally:
        for p in procs:
            p.join(max(0.0, min(20.0, deadline - time.monotonic())))
            if p.is_alive():
                hung.append(p.pid)
                p.kill()
                p.join()
    assert not hung, f"children {hung} were still alive after {limit} s and were killed; reports so far: {msgs}"
    assert sorted(msgs) == list(range(world)), (msgs, [p.exitcode for p in procs])
    bad = {r: m for r, m in msgs.items() if isinstance(m, str)}
    assert not bad, "\n".join(f"rank {r}:\n{m}" for r, m in bad.items())
    assert all(p.exitcode == 0 for p in procs), [p.exitcode for p in procs]
    return msgs


def _group(rank, world, port, backend="gloo"):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    os.environ["VJ_FORCE_DP"] = "0"
    torch.cuda.set_device(0)
    if backend == "nccl":
        dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device("cuda", 0))
    else:
        dist.init_process_group("gloo", rank=rank, world_size=world, timeout=timedelta(seconds=60))
    return dist


def _reported(fn):
    """A worker body: its result, or its traceback, goes to the parent through the queue."""
    def worker(rank, world, port, q, *args):
        try:
            q.put((rank, fn(rank, world, port, *args)))
        except BaseException:   # noqa: BLE001
            import traceback
            q.put((rank, traceback.format_exc()))
    worker.__name__ = worker.__qualname__ = fn.__name__      # spawn finds the target by its module-level name: the wrapper
    worker.__module__ = fn.__module__
    return worker


def _inputs(rank, case):
    """The rank's own batch of two: clips of the fixture, or (case 'still') seeded images."""
    from tests.finetune_util import _clips
    from tests.golden_util import MICRO
    if case == "still":
        x = torch.randn(2, 3, MICRO["crop"], MICRO["crop"], generator=torch.Generator().manual_seed(3 + rank))
    else:
        x = _clips(2)[rank]
    return x.to("cuda"), torch.tensor(LABELS[rank], device="cuda")


def _fresh_encoder(case):
    from tests.finetune_util import _encoder
    enc = _encoder()
    if case == "still":
        enc.train_on_any_input()
    if case in ("mlp", "block"):
        enc.set_activation_recompute(case)
    return enc


def _backward(enc, clf, x, labels):
    import torch.nn.functional as F
    clf.zero_grad(set_to_none=True)
    loss = F.cross_entropy(clf(enc(x)), labels)
    loss.backward()
    torch.cuda.synchronize()
    return float(loss.detach())


def _local_and_reduced(rank, world, dist, case):
    """The rank's own gradient arena from a plain tuner on a fresh encoder, the arena of a data-parallel tuner on another fresh
    encoder after the same backward, and the all-gathered own arenas of both ranks."""
    from jepa_amd.engine.finetune import EncoderFineTuner
    from tests.finetune_util import _classifier
    clf = _classifier()                     # the same seed, so the same probe, on both ranks
    x, labels = _inputs(rank, case)
    plain = EncoderFineTuner(_fresh_encoder(case), layer_decay=0.75)
    assert plain.reducer is None and plain.encoder.grad_reducer is None
    _backward(plain.encoder, clf, x, labels)
    mine = plain.arena.G.clone()
    tuner = EncoderFineTuner(_fresh_encoder(case), layer_decay=0.75, world_size=world)
    assert tuner.reducer is not None and tuner.reducer.enabled and tuner.encoder.grad_reducer is tuner.reducer
    assert torch.equal(tuner.arena.P, plain.arena.P)          # (the broadcast left the fixture's weights)
    _backward(tuner.encoder, clf, x, labels)
    parts = [torch.empty_like(mine) for _ in range(world)]
    dist.all_gather(parts, mine)
    assert torch.equal(parts[rank], mine)
    return plain, tuner, parts


@_reported
def _sum_worker(rank, world, port, case):
    dist = _group(rank, world, port)
    plain, tuner, parts = _local_and_reduced(rank, world, dist, case)
    red = tuner.reducer
    assert not torch.equal(parts[0], parts[1])                                   # the ranks saw different data
    # a bucket that went out before its gradients were written would have reduced the fresh arena's zeros, and the local
    # gradients written afterwards would stand there alone
    wrong = [n for n, s in tuner.arena.slots.items()
             if not torch.equal(tuner.arena.grad(n), (parts[0] + parts[1])[s.off:s.off + s.numel].view(s.shape))]
    assert not wrong, wrong
    assert torch.equal(tuner.arena.G, parts[0] + parts[1])
    depth = len(tuner.encoder.blocks)
    assert len(red.buckets) == depth + 1 and len(red.tail) == depth + 1
    assert len(red.launched) == len(red.buckets) + len(red.tail)
    assert red.launched[:depth + 1] == [red.buckets[("enc", li)][0] for li in list(range(depth - 1, -1, -1)) + [-1]]
    assert red.launched[depth + 1:] == red.tail
    dist.barrier()
    dist.destroy_process_group()
    return {"launched": list(red.launched)}


@pytest.mark.timeout(300)
@pytest.mark.parametrize("case", ["none", "block", "still"])
def test_reduced_gradient_is_the_sum_of_the_ranks_own(case):
    """recompute none / block on clips, and one still-image batch on an encoder with train_on_any_input()."""
    msgs = _spawn(_sum_worker, 2, case)
    assert msgs[0]["launched"] == msgs[1]["launched"]


@_reported
def _step_worker(rank, world, port):
    from jepa_amd.engine.finetune import EncoderFineTuner
    dist = _group(rank, world, port)
    plain, tuner, parts = _local_and_reduced(rank, world, dist, "none")
    tuner.step(LR, WD, clip=CLIP)
    norm, bad = tuner.grad_stats()
    ref = EncoderFineTuner(_fresh_encoder("none"), layer_decay=0.75)
    ref.arena.G.copy_(parts[0] + parts[1])
    ref.step(LR, WD, clip=CLIP, grad_scale=2.0)        # the one-rank update of the mean: the sum under a scale of 2
    for name in ("P", "M1", "M2", "Pb"):
        assert torch.equal(getattr(tuner.arena, name), getattr(ref.arena, name)), name
    assert tuner.opt_step == 1 and bad == 0
    assert norm == ref.grad_stats()[0] / 2          # the norm of the averaged gradient
    assert not torch.equal(tuner.arena.P, plain.arena.P)      # (the plain tuner never stepped: the fixture's weights)
    other = tuner.arena.P.clone()
    dist.broadcast(other, 0)
    assert torch.equal(other, tuner.arena.P), "the ranks' weights diverged"
    dist.barrier()
    dist.destroy_process_group()
    return {"done": True}       # (a string would stand for a traceback)


@pytest.mark.timeout(300)
def test_update_is_the_one_rank_update_of_the_mean():
    _spawn(_step_worker, 2)


@_reported
def _nonfinite_worker(rank, world, port):
    from jepa_amd.engine.finetune import EncoderFineTuner
    from tests.finetune_util import _classifier
    dist = _group(rank, world, port)
    clf = _classifier()
    x, labels = _inputs(rank, "none")
    if rank == 1:
        x[0, 0, 0, 0, 0] = float("inf")
    tuner = EncoderFineTuner(_fresh_encoder("none"), layer_decay=0.75, world_size=world)
    before = (tuner.arena.P.clone(), tuner.arena.M1.clone(), tuner.arena.M2.clone())
    loss = _backward(tuner.encoder, clf, x, labels)
    assert (loss == loss) == (rank == 0)               # rank 0's own loss is finite: only the reduction tells it
    tuner.step(LR, WD, clip=CLIP)
    assert tuner.opt_step == 0
    assert all(torch.equal(a, b) for a, b in zip(before, (tuner.arena.P, tuner.arena.M1, tuner.arena.M2)))
    assert tuner.grad_stats()[1] > 0
    dist.barrier()
    dist.destroy_process_group()
    return {"done": True}       # (a string would stand for a traceback)


@pytest.mark.timeout(300)
def test_nonfinite_gradient_on_one_rank_skips_the_step_on_both():
    _spawn(_nonfinite_worker, 2)


@_reported
def _one_rank_rccl_worker(rank, world, port):
    """Own process: an RCCL (`nccl`) group of one; the forced reducer must leave two iterations bit-identical to the plain tuner's
    (a SUM over one rank is the identity: any difference is an ordering or stream fault of the bucket path)."""
    from jepa_amd.engine.finetune import EncoderFineTuner
    from tests.finetune_util import _classifier, _clips
    dist = _group(rank, world, port, backend="nccl")
    res, info = {}, {}
    for mode in ("plain", "dp"):
        os.environ["VJ_FORCE_DP"] = "1" if mode == "dp" else "0"
        tuner = EncoderFineTuner(_fresh_encoder("none"), layer_decay=0.75)
        assert (tuner.reducer is not None) == (mode == "dp") and tuner.world == 1
        clf = _classifier()
        losses = []
        for clips in _clips(2):
            losses.append(_backward(tuner.encoder, clf, clips.to("cuda"), torch.tensor(LABELS[0], device="cuda")))
            tuner.step(LR, WD, clip=CLIP)
        torch.cuda.synchronize()
        if mode == "dp":
            red = tuner.reducer
            assert len(red.launched) == len(red.buckets) + len(red.tail)
            info = {"route": red.route, "coll_check": None if red.coll_check is None else red.coll_check.get("verdict")}
        res[mode] = (losses, tuner.arena.G.clone(), tuner.arena.P.clone())
    os.environ["VJ_FORCE_DP"] = "0"
    dist.destroy_process_group()
    assert res["dp"][0] == res["plain"][0], (res["dp"][0], res["plain"][0])
    assert torch.equal(res["dp"][1], res["plain"][1]) and torch.equal(res["dp"][2], res["plain"][2])
    return info


@pytest.mark.timeout(300)
def test_forced_reducer_at_one_rccl_rank_leaves_the_iterations_bit_identical():
    info = _spawn(_one_rank_rccl_worker, 1)[0]
    print("one-rank RCCL route:", info)
    assert info["route"] in ("sync", "capi")


# ------------------------------------------------------------------------------------------------------------------ the evals
CKPT_KEYS = ['batch_size', 'classifier', 'encoder', 'encoder_opt', 'epoch', 'lr', 'opt', 'scaler', 'world_size']


def _video_cfg(folder):
    from tests.finetune_util import _eval_cfg
    cfg = _eval_cfg(folder)
    cfg['data']['synthetic_length'] = 4
    cfg['optimization']['num_epochs'] = 2
    cfg['optimization']['finetune'].update(drop_path=0.1, mix={'prob': 1.0, 'seed': 0})
    return cfg


def _image_cfg(folder):
    from tests.test_still_finetune_gpu import _eval_cfg
    return _eval_cfg(folder)


@_reported
def _eval_worker(rank, world, port, root):
    from jepa_amd.evals.image_classification_finetune import eval as IFT
    from jepa_amd.evals.video_classification_finetune import eval as FT
    from jepa_amd.src.models import vision_transformer as vit
    from tests.finetune_util import _micro_vit
    dist = _group(rank, world, port)
    vit.vit_micro = lambda **kw: _micro_vit()
    tuners, saves, real_save = [], [], torch.save
    drawn, real_entries = [], vit.VisionTransformer._drop_path_entries

    def entries(self, x, inp):
        got = real_entries(self, x, inp)
        if self.last_drop_path_scales is not None:
            drawn.append(self.last_drop_path_scales.clone())
        return got

    vit.VisionTransformer._drop_path_entries = entries

    class Recording(FT.EncoderFineTuner):
        def __init__(self, *a, **kw):
            super().__init__(*a, **kw)
            tuners.append(self)

    FT.EncoderFineTuner = Recording
    torch.save = lambda obj, path, *a, **kw: (saves.append(str(path)), real_save(obj, path, *a, **kw))[1]
    initial = Recording(_fresh_encoder("none"), layer_decay=0.75).arena.P.clone()
    tuners.clear()
    out = {}
    for name, main, cfg in (("video", FT.main, _video_cfg(os.path.join(root, "video"))),
                            ("image", IFT.main, _image_cfg(os.path.join(root, "image")))):
        rec = main(cfg)
        tuner = tuners[-1]
        red = tuner.reducer
        assert tuner.world == world and red is not None and len(red.launched) == len(red.buckets) + len(red.tail)
        assert len(rec['train_history']) == 2 and all(ls == ls for _, ls in rec['train_history'])      # an iteration per epoch
        assert tuner.opt_step == 2
        assert tuner.encoder.drop_path_generator.initial_seed() == rank
        mine = tuner.arena.P.clone()
        other = mine.clone()
        dist.broadcast(other, 0)
        assert torch.equal(mine, other), f"{name}: the ranks' encoders diverged"
        assert not torch.equal(mine, initial), f"{name}: the encoder did not move"
        # the video run's two training forwards drew their drops (from the generator checked above); the image run has rate 0
        assert len(drawn) == (2 if name == "video" else 0), (name, len(drawn))
        drawn.clear()
        out[name] = [lr for lr, _ in rec['train_history']]
    out["saves"] = list(saves)
    dist.barrier()
    dist.destroy_process_group()
    if rank == 0:       # what the two ranks left, then a one-rank run resumes from it
        for name, sub in (("video", "video_classification_finetune"), ("image", "image_classification_finetune")):
            ck = torch.load(os.path.join(root, name, sub, "micro_ft", "micro-latest.pth.tar"), map_location="cpu", weights_only=False)
            out[name + "_ckpt"] = (sorted(ck), ck['world_size'], ck['epoch'], float(ck['encoder_opt']['state'][0]['step']))
        os.environ.pop("RANK")
        os.environ.pop("WORLD_SIZE")
        cfg = _video_cfg(os.path.join(root, "video"))
        cfg['optimization']['num_epochs'] = 3
        rec = FT.main(cfg, resume_preempt=True)
        assert tuners[-1].world == 1 and tuners[-1].reducer is None and tuners[-1].opt_step == 2 + 2
        out["resumed"] = (rec['start_epoch'], len(rec['train_history']))
    return out


@pytest.mark.timeout(400)
def test_both_evals_on_two_ranks(tmp_path):
    from tests.golden_util import load_micro, micro_weights
    enc_w = micro_weights(load_micro())[0]
    for name in ("video", "image"):
        os.makedirs(tmp_path / name)
        torch.save({'target_encoder': {'module.backbone.' + k: v for k, v in enc_w.items()}, 'epoch': 10},
                   tmp_path / name / 'micro-latest.pth.tar')
    msgs = _spawn(_eval_worker, 2, str(tmp_path), limit=360)
    assert msgs[0]["video"] == msgs[1]["video"] and msgs[0]["image"] == msgs[1]["image"]        # one schedule on both ranks
    assert msgs[1]["saves"] == [] and len(msgs[0]["saves"]) >= 4                               # only rank 0 wrote
    assert msgs[0]["resumed"] == (2, 2)          # one epoch of 4 items in batches of 2 on one rank
    for name, sub in (("video", "video_classification_finetune"), ("image", "image_classification_finetune")):
        out = tmp_path / name / sub / "micro_ft"
        assert sorted(os.listdir(out)) == ["micro-latest.pth.tar", "micro_r0.csv"]
        ck = torch.load(out / "micro-latest.pth.tar", map_location="cpu", weights_only=False)
        assert msgs[0][name + "_ckpt"] == (CKPT_KEYS, 2, 2, 2.0)        # the present keys, written at world_size 2
        assert sorted(ck) == CKPT_KEYS
        if name == "video":       # rewritten by the resumed one-rank run
            assert ck['world_size'] == 1 and ck['epoch'] == 3
        moved = [n for n, v in ck['encoder'].items() if not torch.equal(v, enc_w[n])]
        assert 'pos_embed' not in moved and len(moved) > 0
