"""What the fine-tuning GPU tests share (test_finetune_gpu, test_drop_path_gpu, test_mix_gpu, test_still_finetune_gpu): the micro
encoder of tests/golden/micro_step.npz, a seeded AttentiveClassifier, the clips, the CPU oracle's encoder gradients, the gradient
bound with the measurements behind it, and the micro configuration of the fine-tuning eval."""
from functools import partial

import torch
import torch.nn.functional as F

from tests.golden_util import MICRO, load_micro, micro_weights, rel_l2, step_inputs
from tests.step_util import oracle_cfg

DEV = "cuda"
C = 10
HEADS = MICRO["heads"]

# measured worst rel-L2 of an encoder parameter gradient against the fp32 CPU oracle on MI355X: plain (blocks.0.norm2.weight),
# aggregation concatenated and aggregation per segment (both patch_embed.proj.weight)
MEASURED_E2E = (7.32e-3, 7.03e-3, 6.37e-3)
BOUND = min(2 * max(MEASURED_E2E), 7e-2)        # 1.46e-2


def _micro_vit():
    from jepa_amd.src.models.vision_transformer import VisionTransformer
    c = MICRO
    return VisionTransformer(img_size=c["crop"], patch_size=c["patch"], num_frames=c["frames"], tubelet_size=c["tubelet"],
                             embed_dim=c["embed_dim"], depth=c["depth"], num_heads=c["heads"], mlp_ratio=4, qkv_bias=True,
                             norm_layer=partial(torch.nn.LayerNorm, eps=1e-6), uniform_power=True)


def _encoder(weights=None):
    enc = _micro_vit()
    enc.load_state_dict(micro_weights(load_micro())[0] if weights is None else weights, strict=True)
    return enc.to(DEV)


def _classifier(seed=5):
    from jepa_amd.src.models.attentive_pooler import AttentiveClassifier
    torch.manual_seed(seed)
    m = AttentiveClassifier(embed_dim=MICRO["embed_dim"], num_heads=HEADS, depth=1, num_classes=C)
    with torch.no_grad():
        for p in m.parameters():
            if p.dim() == 1:
                p.add_(0.05 * torch.randn_like(p))
    return m.to(DEV)


def _clips(n, seed=0):
    """n batches of 2 clips: the fixture's clips first, seeded draws of the same shape after them."""
    z = load_micro()
    out = [step_inputs(z, s)[0] for s in range(min(n, 2))]
    g = torch.Generator().manual_seed(100 + seed)
    out += [torch.randn(out[0].shape, generator=g) for _ in range(n - len(out))]
    return out


def _oracle_grads(enc_w, clf, segments, labels, across):
    """Encoder gradients of CE(classifier(features)) on the CPU: segments = list of [B,3,T,H,W]; across: the classifier sees the
    segments' tokens concatenated, otherwise the loss is the mean over the segments."""
    from oracle import probe_oracle as po
    from oracle import vjepa_oracle as O
    cfg = oracle_cfg(MICRO, 2)
    w = {k: v.clone().requires_grad_(k != "pos_embed") for k, v in enc_w.items()}
    cw = {n: p.detach().cpu().clone() for n, p in clf.named_parameters()}
    feats = [O.encoder_forward(w, c, cfg, masks=None) for c in segments]
    if across:
        loss = F.cross_entropy(po.attentive_classifier(cw, torch.cat(feats, dim=1), HEADS), labels)
    else:
        loss = sum(F.cross_entropy(po.attentive_classifier(cw, f, HEADS), labels) for f in feats) / len(feats)
    loss.backward()
    return float(loss.detach()), {k: v.grad for k, v in w.items() if v.grad is not None}


def _worst(tuner, ref):
    errs = {n: rel_l2(tuner.arena.grad(n).float().cpu(), g) for n, g in ref.items()}
    assert set(errs) == set(tuner.arena.slots)
    return max((e, n) for n, e in errs.items())


def _eval_cfg(folder):
    """The micro configuration behind tests/golden/eval_micro.npz (S = 2 segments, V = 2 validation views, B = 2, 10 classes, the
    micro encoder at 8 x 64 x 64) on the synthetic dataset: one fixed batch per epoch, 8 epochs = 8 iterations."""
    return {
        'pretrain': {'model_name': 'vit_micro', 'checkpoint_key': 'target_encoder', 'patch_size': 16, 'folder': folder,
                     'checkpoint': 'micro-latest.pth.tar', 'write_tag': 'micro', 'tubelet_size': 2, 'frames_per_clip': 8,
                     'uniform_power': True, 'use_sdpa': True, 'use_silu': False, 'tight_silu': False},
        'data': {'dataset_type': 'synthetic', 'dataset_train': None, 'dataset_val': None, 'num_classes': C, 'frames_per_clip': 8,
                 'num_segments': 2, 'num_views_per_segment': 2, 'synthetic_length': 2},
        'optimization': {'resolution': 64, 'batch_size': 2, 'attend_across_segments': True, 'num_epochs': 8,
                         'weight_decay': 0.01, 'start_lr': 0.002, 'lr': 0.01, 'final_lr': 0.0, 'warmup': 0.25,
                         'use_bfloat16': False,
                         'finetune': {'encoder_lr': 1e-3, 'layer_decay': 0.75, 'encoder_weight_decay': 0.05}},
        'tag': 'micro_ft',
    }
