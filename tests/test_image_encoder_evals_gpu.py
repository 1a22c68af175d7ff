"""GPU: both frozen evals' main() with an image (pretrain.frames_per_clip: 1) encoder on micro synthetic configs."""
import csv

import numpy as np
import pytest
import torch

from tests.image_vit_golden_util import fixture, micro_image_vit

pytestmark = pytest.mark.gpu
DEV = "cuda"
REFERENCE_CHECKPOINT_KEYS = ['batch_size', 'classifier', 'epoch', 'lr', 'opt', 'scaler', 'world_size']   # eval.py:247-255


def _micro_factory(**kw):
    from functools import partial
    from jepa_amd.src.models.vision_transformer import VisionTransformer
    kw.pop("use_sdpa", None)
    return VisionTransformer(embed_dim=64, depth=2, num_heads=2, mlp_ratio=4, qkv_bias=True,
                             norm_layer=partial(torch.nn.LayerNorm, eps=1e-6), **kw)


@pytest.fixture
def checkpoint(tmp_path, monkeypatch):
    """The fixture's micro image ViT saved as a pretraining checkpoint (Conv2d key shapes), and vit.vit_micro to build it."""
    from jepa_amd.src.models import vision_transformer as vit
    monkeypatch.setattr(vit, "vit_micro", _micro_factory, raising=False)
    enc = micro_image_vit(fixture())
    torch.save({'target_encoder': {'module.backbone.' + k: v for k, v in enc.state_dict().items()}, 'epoch': 10},
               tmp_path / 'micro-latest.pth.tar')
    return enc


def _pretrain(folder):
    # no tubelet_size and no frames_per_clip key beyond the explicit 1: the reference's defaults
    return {'model_name': 'vit_micro', 'checkpoint_key': 'target_encoder', 'patch_size': 8, 'folder': folder,
            'checkpoint': 'micro-latest.pth.tar', 'write_tag': 'micro', 'frames_per_clip': 1, 'use_sdpa': True, 'use_silu': False,
            'tight_silu': False}


OPT = {'batch_size': 4, 'num_epochs': 2, 'weight_decay': 0.01, 'start_lr': 0.002, 'lr': 0.01, 'final_lr': 0.0, 'warmup': 0.5,
       'use_bfloat16': False}


def _video_cfg(folder, across=True):
    return {'pretrain': _pretrain(folder),
            'data': {'dataset_type': 'synthetic', 'dataset_train': None, 'dataset_val': None, 'num_classes': 4, 'frames_per_clip': 4,
                     'num_segments': 2, 'num_views_per_segment': 2, 'synthetic_length': 12},
            'optimization': dict(OPT, resolution=32, attend_across_segments=across),
            'tag': 'micro_eval'}


def _image_cfg(folder):
    return {'pretrain': _pretrain(folder),
            'data': {'dataset_name': 'synthetic', 'num_classes': 4, 'root_path': None, 'image_folder': None, 'resolution': 32,
                     'synthetic_length': 12},
            'optimization': dict(OPT),
            'tag': 'micro_eval'}


def _check_outputs(out, rec, iters):
    from jepa_amd.src.models.attentive_pooler import AttentiveClassifier
    rows = list(csv.reader(open(out / "micro_r0.csv")))
    assert rows[0] == ["epoch", "loss", "acc"] and [r[0] for r in rows[1:]] == ["1", "2"]
    ck = torch.load(out / "micro-latest.pth.tar", map_location="cpu", weights_only=False)
    assert sorted(ck) == REFERENCE_CHECKPOINT_KEYS and ck['epoch'] == 2 and ck['scaler'] is None
    assert list(ck['classifier']) == ['module.' + k for k in AttentiveClassifier(embed_dim=64, num_heads=2, num_classes=4).state_dict()]
    hist = rec['train_history']
    assert len(hist) == iters and all(np.isfinite(ls) for _, ls in hist), hist
    assert len(rec['val_acc']) == 2 and all(0.0 <= a <= 100.0 for a in rec['train_acc'] + rec['val_acc'])


def test_video_eval_main_with_an_image_encoder(tmp_path, checkpoint):
    from jepa_amd.evals.video_classification_frozen import eval as E
    from jepa_amd.evals.video_classification_frozen.utils import FrameAggregation
    seen = []
    real = FrameAggregation.forward

    def spy(self, x, clip_indices=None):
        out = real(self, x, clip_indices)
        seen.append((len(x), len(x[0]), tuple(x[0][0].shape), [tuple(o.shape) for o in out],
                     torch.equal(self.model.pos_embed.cpu(), checkpoint.pos_embed),
                     torch.equal(self.model.patch_embed.proj.weight.cpu(), checkpoint.patch_embed.proj.weight)))
        return out

    FrameAggregation.forward = spy
    try:
        torch.manual_seed(0)
        rec = E.main(_video_cfg(str(tmp_path)))
    finally:
        FrameAggregation.forward = real
    _check_outputs(tmp_path / "video_classification_frozen" / "micro_eval", rec, iters=6)       # 2 epochs x 12 items / batch 4
    # training: 2 segments x 1 view; validation: 2 segments x 2 views; [B, S*T*N, D] per view; the checkpoint's weights were loaded
    assert seen[0] == (2, 1, (4, 3, 4, 32, 32), [(4, 2 * 4 * 16, 64)], True, True)
    assert seen[3] == (2, 2, (4, 3, 4, 32, 32), [(4, 2 * 4 * 16, 64)] * 2, True, True)


def test_video_eval_without_attend_across_segments_raises(tmp_path, checkpoint):
    from jepa_amd.evals.video_classification_frozen import eval as E
    with pytest.raises(ValueError, match="concatenated form"):
        E.main(_video_cfg(str(tmp_path), across=False))


def test_image_eval_main_with_an_image_encoder(tmp_path, checkpoint, monkeypatch):
    from jepa_amd.evals.image_classification_frozen import eval as E
    from jepa_amd.src.models.vision_transformer import VisionTransformer
    seen = []
    real = E.frozen_features

    def spy(encoder, imgs):
        out = real(encoder, imgs)
        direct = encoder(imgs)                                     # the image model is fed [B,3,H,W] itself: no hook, no wrapper
        seen.append((type(encoder) is VisionTransformer and not encoder.is_video, tuple(imgs.shape), tuple(out.shape),
                     torch.equal(out, direct)))
        return out

    monkeypatch.setattr(E, "frozen_features", spy)
    torch.manual_seed(0)
    rec = E.main(_image_cfg(str(tmp_path)))
    _check_outputs(tmp_path / "image_classification_frozen" / "micro_eval", rec, iters=6)
    assert len(seen) == 12 and all(s == (True, (4, 3, 32, 32), (4, 16, 64), True) for s in seen), seen
    # the features are those of the checkpoint's model, called directly
    enc = checkpoint.to(DEV)
    imgs = next(iter(E.make_dataloader(dataset_name='synthetic', root_path=None, image_folder=None, batch_size=4, world_size=1, rank=0,
                                       resolution=32, training=False, num_classes=4, synthetic_length=12)))[0].to(DEV)
    with torch.no_grad():
        assert real(_micro_loaded(tmp_path), imgs).equal(enc(imgs))


def _micro_loaded(folder):
    from jepa_amd.evals.image_classification_frozen.eval import init_model
    enc = init_model(device=torch.device(DEV), pretrained=str(folder / 'micro-latest.pth.tar'), model_name='vit_micro', patch_size=8,
                     crop_size=32, frames_per_clip=1)
    enc.eval()
    for p in enc.parameters():
        p.requires_grad = False
    return enc
