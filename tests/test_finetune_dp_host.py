"""CPU: the host side of data-parallel encoder fine-tuning -- the bucket plan of a tuner's arena (engine.dp.finetune_bucket_plan) on
the micro encoder and on a depth-24 layout, the generalised GradReducer walking an explicit plan over a fake arena in a two-rank
gloo group, and the per-rank drop-path / mix seeds of the fine-tuning evals."""
import os
import socket
import sys
from datetime import timedelta
from functools import partial
from types import SimpleNamespace

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests.golden_util import MICRO  # noqa: E402


def _micro_named():
    """The micro ViT of tests/finetune_util.py (whose module needs the golden fixture's loaders only), built on the CPU."""
    from jepa_amd.src.models.vision_transformer import VisionTransformer
    c = MICRO
    m = VisionTransformer(img_size=c["crop"], patch_size=c["patch"], num_frames=c["frames"], tubelet_size=c["tubelet"],
                          embed_dim=c["embed_dim"], depth=c["depth"], num_heads=c["heads"], mlp_ratio=4, qkv_bias=True,
                          norm_layer=partial(torch.nn.LayerNorm, eps=1e-6), uniform_power=True)
    return list(m.named_parameters()), len(m.blocks)


def _depth24_named():
    from jepa_amd.src.models.vision_transformer import vit_large
    with torch.device("meta"):
        m = vit_large(img_size=224, patch_size=16, num_frames=16, tubelet_size=2, uniform_power=True)
    return list(m.named_parameters()), len(m.blocks)


def _layout(named, depth):
    from jepa_amd.engine import optstate
    groups = optstate.layer_decay_groups(named, depth, 0.75)
    return groups, optstate.layout([members for _, members in groups])


def _tail(plan, total):
    """What a plan leaves to the reducer's finish(): its gaps in [0, total) (the gloo test holds GradReducer.tail against this)."""
    tail, pos = [], 0
    for lo, hi in sorted(r for rs in plan.values() for r in rs):
        if lo > pos:
            tail.append((pos, lo))
        pos = max(pos, hi)
    if pos < total:
        tail.append((pos, total))
    return tail


@pytest.mark.parametrize("which", ["micro", "depth24"])
def test_bucket_plan_tiles_the_arena_and_keeps_small_tensors_out(which):
    from jepa_amd.engine import dp, optstate
    named, depth = _micro_named() if which == "micro" else _depth24_named()
    assert depth == (MICRO["depth"] if which == "micro" else 24)
    groups, (slots, ranges, total) = _layout(named, depth)
    plan = dp.finetune_bucket_plan(slots, ranges, total)
    # one bucket per block and one for the patch embedding, each exactly one decayed range
    assert sorted(plan) == sorted([("enc", li) for li in range(-1, depth)])
    assert all(len(rs) == 1 for rs in plan.values())
    decayed = {g["layer_id"]: r for (g, _), r in zip(groups, ranges) if not g.get("WD_exclude", False)}
    nodecay = [r for (g, _), r in zip(groups, ranges) if g.get("WD_exclude", False)]
    assert len(nodecay) == depth + 2
    for li in range(-1, depth):
        assert plan[("enc", li)] == [decayed[li + 1]]
    mats = ("attn.qkv.weight", "attn.proj.weight", "mlp.fc1.weight", "mlp.fc2.weight")
    for li in range(depth):
        lo, hi = plan[("enc", li)][0]
        inside = sorted(n for n, s in slots.items() if lo <= s.off < hi)
        assert inside == sorted(f"blocks.{li}.{m}" for m in mats)
    lo, hi = plan[("enc", -1)][0]
    assert [n for n, s in slots.items() if lo <= s.off < hi] == ["patch_embed.proj.weight"]
    # buckets and tail tile [0, total) exactly once
    tail = _tail(plan, total)
    cover = torch.zeros(total, dtype=torch.int32)
    for rs in list(plan.values()) + [tail]:
        for lo, hi in rs:
            cover[lo:hi] += 1
    assert bool((cover == 1).all())
    # no no-decay tensor is in a block bucket: all of them, and nothing else, lie in the tail
    params = dict(named)
    in_tail = sorted(n for n, s in slots.items() if any(lo <= s.off < hi for lo, hi in tail))
    assert in_tail == sorted(n for n in slots if optstate.is_no_decay(n, params[n]))
    for r in nodecay:
        assert any(lo <= r[0] and r[1] <= hi for lo, hi in tail), r
    # the last block's small tensors and the final norm's are neighbours and go out as one collective
    assert len(tail) == depth + 1
    # a walk in backward order launches one decayed range per hook, the last block's first
    walk = [plan[("enc", li)] for li in list(range(depth - 1, -1, -1)) + [-1]]
    assert all(len(w) == 1 for w in walk)
    assert [w[0] for w in walk] == [decayed[lid] for lid in list(range(depth, 0, -1)) + [0]]


def test_bucket_plan_refuses_another_layout():
    from jepa_amd.engine import dp, optstate
    named, depth = _micro_named()
    decay = [(n, p) for n, p in named if p.requires_grad and not optstate.is_no_decay(n, p)]
    small = [(n, p) for n, p in named if p.requires_grad and optstate.is_no_decay(n, p)]
    slots, ranges, total = optstate.layout([decay, small])      # the Trainer's kind of layout: every layer in one range
    with pytest.raises(ValueError, match="layer_decay_groups"):
        dp.finetune_bucket_plan(slots, ranges, total)


# ------------------------------------------------------------------------------------------------ the reducer on an explicit plan
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, q):
    try:
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
        import torch.distributed as dist
        from jepa_amd.engine import dp
        dist.init_process_group("gloo", rank=rank, world_size=world, timeout=timedelta(seconds=60))
        named, depth = _micro_named()
        _, (slots, ranges, total) = _layout(named, depth)
        arena = SimpleNamespace(slots=slots, group_ranges=ranges, total=total, G=torch.zeros(total), P=torch.zeros(total))
        plan = dp.finetune_bucket_plan(slots, ranges, total)
        red = dp.GradReducer(arena, None, None, world, plan=plan)
        assert red.enabled and red.route == "blocking" and red.buckets == plan
        assert red.tail == _tail(plan, total)
        order = []
        for step in range(2):
            arena.G.copy_(torch.randint(-8, 9, (total,), generator=torch.Generator().manual_seed(10 * step + rank)).float())
            red.begin()
            for li in range(depth - 1, -1, -1):
                red.layer_done("enc", li)
            red.layer_done("enc", -1)
            red.layer_done("pred", 0)       # a hook nobody planned launches nothing
            red.finish()
            parts = [torch.randint(-8, 9, (total,), generator=torch.Generator().manual_seed(10 * step + r)).float()
                     for r in range(world)]
            assert torch.equal(arena.G, parts[0] + parts[1])         # small integers: every element summed exactly once
            assert len(red.launched) == len(red.buckets) + len(red.tail)
            assert red.launched == [plan[("enc", li)][0] for li in list(range(depth - 1, -1, -1)) + [-1]] + red.tail
            order.append(list(red.launched))
        dist.barrier()
        dist.destroy_process_group()
        q.put((rank, order))
    except BaseException:   # noqa: BLE001
        import traceback
        q.put((rank, traceback.format_exc()))


@pytest.mark.timeout(120)
def test_reducer_walks_an_explicit_plan_world2_gloo():
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    try:
        msgs = dict(q.get(timeout=100) for _ in range(2))
    finally:
        for p in procs:
            p.join(20)
            if p.is_alive():
                p.kill()
    assert all(isinstance(m, list) for m in msgs.values()), msgs
    assert msgs[0] == msgs[1]           # `launched` has the same order on both ranks
    assert all(p.exitcode == 0 for p in procs), [p.exitcode for p in procs]


def test_plan_and_trainer_ways_in_agree_on_the_trainers_arena():
    """The Trainer's construction goes through trainer_bucket_plan; handing its result in as an explicit plan gives the same
    buckets, in the same order, and the same tail."""
    from jepa_amd.engine import dp
    from tests.test_dp_gloo import _fake_arena
    arena, vit, pred = _fake_arena()
    plan = dp.trainer_bucket_plan(arena.slots, len(vit.blocks), len(pred.predictor_blocks), 2)
    a = dp.GradReducer(arena, vit, pred, 2, pred_layers_per_bucket=2)
    b = dp.GradReducer(arena, None, None, 2, plan=plan)
    assert list(a.buckets.items()) == list(b.buckets.items()) and a.tail == b.tail and a.tail


# ------------------------------------------------------------------------------------------------ per-rank seeds
def test_per_rank_seeds():
    from jepa_amd.evals.video_classification_finetune.eval import MIX_DEFAULTS, rank_seeds
    from jepa_amd.evals.video_classification_frozen import eval as frozen_eval
    one = rank_seeds(0, 1, MIX_DEFAULTS['seed'])
    assert one == (frozen_eval._GLOBAL_SEED, MIX_DEFAULTS['seed'])      # the one-rank run: the global seed, the section's mix seed
    r0, r1 = rank_seeds(0, 2, MIX_DEFAULTS['seed']), rank_seeds(1, 2, MIX_DEFAULTS['seed'])
    assert r0 == one
    assert r0[0] != r1[0] and r0[1] != r1[1]
    assert rank_seeds(1, 2, 7) == (frozen_eval._GLOBAL_SEED + 1, 8)
    assert rank_seeds(3, 4, 2 ** 32 - 1)[1] == 2                        # stays a seed np.random.RandomState takes
    with pytest.raises(ValueError):
        rank_seeds(2, 2)
    # the draws really differ
    import numpy as np
    assert np.random.RandomState(r0[1]).rand() != np.random.RandomState(r1[1]).rand()
    assert torch.rand(4, generator=torch.Generator().manual_seed(r0[0])).tolist() != \
        torch.rand(4, generator=torch.Generator().manual_seed(r1[0])).tolist()


def test_encoder_carries_no_reducer_by_default():
    from jepa_amd.src.models.vision_transformer import VisionTransformer
    m = VisionTransformer(img_size=32, patch_size=16, num_frames=4, tubelet_size=2, embed_dim=64, depth=1, num_heads=2,
                          norm_layer=partial(torch.nn.LayerNorm, eps=1e-6))
    assert m.grad_reducer is None and "grad_reducer" not in m.state_dict()
