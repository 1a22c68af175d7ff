"""CPU: the host side of encoder fine-tuning -- the (layer id, no-decay) grouping with its layer-wise learning-rate scales
(engine.optstate.layer_decay_groups), the `optimization.finetune` defaults, and what the eval and the tuner refuse."""
import os
import sys
from functools import partial

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _micro():
    from jepa_amd.src.models.vision_transformer import VisionTransformer
    return VisionTransformer(img_size=64, patch_size=16, num_frames=8, tubelet_size=2, embed_dim=64, depth=2, num_heads=2,
                             mlp_ratio=4, qkv_bias=True, norm_layer=partial(torch.nn.LayerNorm, eps=1e-6), uniform_power=True)


def _vit_large_named():
    """vit_large's parameter names and shapes without its 300 M weights."""
    from jepa_amd.src.models.vision_transformer import vit_large
    with torch.device("meta"):
        m = vit_large(img_size=224, patch_size=16, num_frames=16, tubelet_size=2, uniform_power=True)
    return list(m.named_parameters()), len(m.blocks)


def _check_groups(named, depth, layer_decay):
    from jepa_amd.engine import optstate
    groups = optstate.layer_decay_groups(named, depth, layer_decay)
    trainable = [n for n, p in named if p.requires_grad]
    seen = [n for _, members in groups for n, _ in members]
    assert sorted(seen) == sorted(trainable) and len(seen) == len(set(seen))     # every trainable parameter exactly once
    assert "pos_embed" not in seen and "pos_embed" in dict(named)
    assert len(groups) <= 2 * (depth + 2)
    assert [g["layer_id"] for g, _ in groups] == sorted(g["layer_id"] for g, _ in groups)
    params = dict(named)
    for g, members in groups:
        assert members
        lid = g["layer_id"]
        assert g["lr_scale"] == pytest.approx(layer_decay ** (depth + 1 - lid), rel=1e-12)
        nodecay = g.get("WD_exclude", False)
        assert (g.get("weight_decay", None) == 0) == nodecay
        for n, p in members:
            if n.startswith("patch_embed."):
                assert lid == 0
            elif n.startswith("blocks."):
                assert lid == int(n.split(".")[1]) + 1
            else:
                assert n in ("norm.weight", "norm.bias") and lid == depth + 1 and g["lr_scale"] == 1.0
            assert nodecay == (n.endswith(".bias") or params[n].dim() == 1) == optstate.is_no_decay(n, p), n
    # every group is one contiguous range, in the order of the groups
    slots, ranges, total = optstate.layout([members for _, members in groups])
    assert ranges[0][0] == 0 and ranges[-1][1] == total
    for (g, members), (lo, hi), nxt in zip(groups, ranges, ranges[1:] + [(total, total)]):
        assert hi == nxt[0]
        assert sorted(slots[n].off for n, _ in members)[0] == lo and all(lo <= slots[n].off < hi for n, _ in members)
    return groups


def test_grouping_of_the_micro_encoder():
    enc = _micro()
    groups = _check_groups(list(enc.named_parameters()), 2, 0.75)
    assert [(g["layer_id"], g.get("WD_exclude", False)) for g, _ in groups] == \
        [(0, False), (0, True), (1, False), (1, True), (2, False), (2, True), (3, True)]
    assert [g["lr_scale"] for g, _ in groups][:2] == [0.75 ** 3] * 2


def test_grouping_of_vit_large_names():
    named, depth = _vit_large_named()
    assert depth == 24
    groups = _check_groups(named, depth, 0.75)
    assert len(groups) == 2 * (depth + 2) - 1          # the final norm has no decayed tensor
    by_name = {n: g for g, members in groups for n, _ in members}
    assert by_name["patch_embed.proj.weight"]["lr_scale"] == pytest.approx(0.75 ** 25)
    assert by_name["blocks.23.mlp.fc2.weight"]["lr_scale"] == pytest.approx(0.75)
    assert by_name["norm.weight"]["lr_scale"] == 1.0


def test_grouping_leaves_frozen_tensors_out():
    from jepa_amd.engine import optstate
    enc = _micro()
    enc.blocks[0].attn.qkv.weight.requires_grad = False
    seen = [n for _, members in optstate.layer_decay_groups(enc.named_parameters(), 2, 0.5) for n, _ in members]
    assert "blocks.0.attn.qkv.weight" not in seen and "blocks.0.attn.qkv.bias" in seen


def test_groups_are_what_torch_adamw_takes():
    """An optimizer built from the groups holds the parameter ids that state_dict() of the tuner counts."""
    from jepa_amd.engine import optstate
    enc = _micro()
    groups = optstate.layer_decay_groups(enc.named_parameters(), 2, 0.75)
    opt = torch.optim.AdamW([dict(g, params=[p for _, p in members], lr=1e-3 * g["lr_scale"]) for g, members in groups])
    sd = opt.state_dict()
    assert [len(g["params"]) for g in sd["param_groups"]] == [len(members) for _, members in groups]
    assert [g["lr_scale"] for g in sd["param_groups"]] == [g["lr_scale"] for g, _ in groups]


def _cfg(folder, **opt):
    return {
        'pretrain': {'model_name': 'vit_micro', 'checkpoint_key': 'target_encoder', 'patch_size': 16, 'folder': folder,
                     'checkpoint': 'micro-latest.pth.tar', 'write_tag': 'micro', 'tubelet_size': 2, 'frames_per_clip': 8,
                     'uniform_power': True},
        'data': {'dataset_type': 'synthetic', 'dataset_train': None, 'dataset_val': None, 'num_classes': 4, 'frames_per_clip': 8,
                 'num_segments': 2, 'num_views_per_segment': 1, 'synthetic_length': 4},
        'optimization': dict({'resolution': 64, 'batch_size': 4, 'attend_across_segments': True, 'num_epochs': 1,
                              'weight_decay': 0.01, 'start_lr': 0.002, 'lr': 0.01, 'final_lr': 0.0, 'warmup': 0.0,
                              'use_bfloat16': False}, **opt),
        'tag': 'ft',
    }


def test_config_defaults():
    from jepa_amd.evals.video_classification_finetune.eval import parse_finetune
    ft = parse_finetune(_cfg("x")['optimization'])
    assert (ft.encoder_lr, ft.layer_decay, ft.encoder_weight_decay, ft.clip_grad) == (0.01, 0.75, 0.05, None)
    ft = parse_finetune(_cfg("x", finetune={'encoder_lr': 1e-4, 'layer_decay': 0.65, 'encoder_weight_decay': 0.0,
                                            'clip_grad': 1.0})['optimization'])
    assert (ft.encoder_lr, ft.layer_decay, ft.encoder_weight_decay, ft.clip_grad) == (1e-4, 0.65, 0.0, 1.0)
    assert parse_finetune(_cfg("x", finetune=None)['optimization']).layer_decay == 0.75
    with pytest.raises(ValueError, match="unknown keys"):
        parse_finetune(_cfg("x", finetune={'encoder_learning_rate': 1.0})['optimization'])


def test_multihead_kwargs_raise(tmp_path):
    from jepa_amd.evals.video_classification_finetune.eval import main
    with pytest.raises(ValueError, match="multihead_kwargs"):
        main(_cfg(str(tmp_path), multihead_kwargs=[{'lr': 0.01}, {'lr': 0.001}]))
    assert not os.listdir(tmp_path)          # refused before anything was set up


def test_image_encoders_raise(tmp_path):
    from jepa_amd.evals.video_classification_finetune.eval import main
    cfg = _cfg(str(tmp_path))
    cfg['pretrain']['frames_per_clip'] = 1
    with pytest.raises(NotImplementedError, match="frozen"):
        main(cfg)


def test_more_than_one_rank_raises():
    from jepa_amd.engine.finetune import EncoderFineTuner
    with pytest.raises(NotImplementedError, match="one rank"):
        EncoderFineTuner(_micro(), world_size=2)


def test_tuner_needs_a_gpu_and_a_video_encoder():
    from jepa_amd.engine.finetune import EncoderFineTuner
    from jepa_amd.src.models.vision_transformer import VisionTransformer
    with pytest.raises(ValueError, match="GPU"):
        EncoderFineTuner(_micro())
    img = VisionTransformer(img_size=32, patch_size=16, num_frames=1, embed_dim=64, depth=1, num_heads=2,
                            norm_layer=partial(torch.nn.LayerNorm, eps=1e-6))
    with pytest.raises(NotImplementedError, match="video"):
        EncoderFineTuner(img)
