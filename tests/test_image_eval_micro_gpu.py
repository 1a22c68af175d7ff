"""GPU: the frozen image-classification eval against tests/golden/image_eval_micro.npz, recorded from the reference's own
run_one_epoch and init_opt (tools/make_golden_image_eval.py) on the micro encoder of micro_step.npz fed still images; B = 2,
10 classes.  The bounds are those of tests/test_eval_micro_gpu.py for the same quantities.  Then main() on a synthetic config."""
import csv
import os
from functools import partial

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
REFERENCE_CHECKPOINT_KEYS = ['batch_size', 'classifier', 'epoch', 'lr', 'opt', 'scaler', 'world_size']   # eval.py:217-225


def rel_l2(a, b):
    a, b = torch.as_tensor(a).detach().float().cpu().reshape(-1), torch.as_tensor(b).detach().float().cpu().reshape(-1)
    return float((a - b).norm() / (b.norm() + 1e-12))


def _encoder():
    from jepa_amd.src.models.vision_transformer import VisionTransformer
    from tests.golden_util import load_micro, micro_weights
    enc = VisionTransformer(img_size=64, patch_size=16, num_frames=8, tubelet_size=2, embed_dim=64, depth=2, num_heads=2,
                            mlp_ratio=4, qkv_bias=True, norm_layer=partial(torch.nn.LayerNorm, eps=1e-6), uniform_power=True)
    enc.load_state_dict(micro_weights(load_micro())[0], strict=True)
    enc.to(DEV).eval()
    for p in enc.parameters():
        p.requires_grad = False
    return enc


def _classifier(z, C):
    from jepa_amd.src.models.attentive_pooler import AttentiveClassifier
    clf = AttentiveClassifier(embed_dim=64, num_heads=2, depth=1, num_classes=C)
    assert list(clf.state_dict().keys()) == [str(k) for k in z["clf_keys"]]     # the reference's key list
    clf.load_state_dict({k: torch.from_numpy(z["clf0/" + k]) for k in clf.state_dict()}, strict=True)
    return clf.to(DEV)


def test_micro_image_eval_end_to_end_against_the_reference():
    """Features (rel-L2 <= 2e-2), logits (<= 3e-2), then 3 training iterations and 1 validation iteration of run_one_epoch with
    init_opt: every iteration's loss within 2e-2 relative, the same learning rates, the same accuracies, and the final classifier
    state by the step-count rule of tests/test_eval_micro_gpu.py."""
    from jepa_amd.evals.image_classification_frozen.eval import init_opt, run_one_epoch
    from tests.image_eval_golden_util import micro_images
    z = np.load(os.path.join(GOLDEN, "image_eval_micro.npz"))
    B, C, iters, T, crop = (int(x) for x in z["dims"])
    train, train_labels, val, val_labels = micro_images(z)
    enc = _encoder()
    with torch.no_grad():
        feat = enc(val.to(DEV))
    e = rel_l2(feat, z["feat"])
    print(f"features rel-L2 {e:.3e}")
    assert e < 2e-2, ("features", e)
    clf = _classifier(z, C)
    with torch.no_grad():
        logits = clf(feat)
    e = rel_l2(logits, z["logits0"])
    print(f"logits rel-L2 {e:.3e}")
    assert e < 3e-2, ("logits", e)
    crit = torch.nn.CrossEntropyLoss()
    loss0 = float(crit(logits, val_labels.to(DEV)))
    assert abs(loss0 - float(z["loss0"])) < 2e-2 * abs(float(z["loss0"]))
    assert float(100. * logits.max(dim=1).indices.eq(val_labels.to(DEV)).sum() / B) == float(z["top1_0"])

    start_lr, ref_lr, final_lr, warmup, num_epochs, wd, ipe = (float(x) for x in z["hp"])
    opt, scaler, sched, wd_sched = init_opt(classifier=clf, iterations_per_epoch=int(ipe), start_lr=start_lr, ref_lr=ref_lr,
                                            warmup=warmup, num_epochs=int(num_epochs), wd=wd, final_lr=final_lr, use_bfloat16=False)
    calls = []
    clf.register_forward_hook(lambda m, i, o: calls.append(o.detach().clone()))
    hist = []
    train_acc = run_one_epoch(DEV, True, enc, clf, scaler, opt, sched, wd_sched, [(train[k], train_labels[k]) for k in range(iters)],
                              False, history=hist)
    val_acc = run_one_epoch(DEV, False, enc, clf, scaler, opt, sched, wd_sched, [(val, val_labels)], False)
    assert len(calls) == iters + 1
    assert [lr for lr, _ in hist] == pytest.approx(list(z["iter_lr"]), rel=1e-12)
    for k, o in enumerate(calls):
        e = rel_l2(o, z["iter_logits"][k])
        print(f"iteration {k} logits rel-L2 {e:.3e}")
    losses = [ls for _, ls in hist] + [float(crit(calls[iters], val_labels.to(DEV)))]
    for k, (mine, ref) in enumerate(zip(losses, z["iter_loss"])):
        print(f"iteration {k} loss {mine:.6f} reference {float(ref):.6f}")
        assert abs(mine - float(ref)) < 2e-2 * abs(float(ref)), (k, mine, float(ref))
    assert [train_acc, val_acc] == pytest.approx(list(z["acc"]), abs=1e-9)
    # final state, the rule of tests/test_eval_micro_gpu.py: 1e-1 rel-L2 per tensor after three AdamW steps of lr ~1e-2; the key half
    # of xattn.kv.bias has a zero gradient analytically, so its steps are rounding noise on both sides, bounded by the steps themselves
    D = 64
    errs = {}
    for n, p in clf.state_dict(keep_vars=True).items():
        ref = torch.from_numpy(z["clf1/" + n])
        mine = p.detach().float().cpu()
        if n.endswith("xattn.kv.bias"):
            steps = float(np.sum(z["iter_lr"]))
            assert float((mine[:D] - ref[:D]).abs().max()) <= 2 * steps * 1.01, n
            mine, ref = mine[D:], ref[D:]
        errs[n] = rel_l2(mine, ref)
    worst = max((e, n) for n, e in errs.items())
    print(f"final classifier state: worst rel-L2 {worst}")
    assert worst[0] < 1e-1, (worst, errs)


def test_frozen_features_split_by_the_tokens_of_the_actual_input(monkeypatch):
    """The encoder call size follows the tokens the input makes, not the model's native num_patches; split calls equal one call."""
    from jepa_amd.evals.image_classification_frozen import eval as E
    enc = _encoder()
    imgs = torch.randn(5, 3, 96, 96, generator=torch.Generator().manual_seed(2)).to(DEV)      # 4 x 6 x 6 = 144 tokens, native 64
    seen = []
    monkeypatch.setattr(E, "max_clips_per_call", lambda width, tokens: seen.append((width, tokens)) or 2)
    with torch.no_grad():
        whole = enc(imgs)
        split = E.frozen_features(enc, imgs)
    assert seen == [(256, 144)] and torch.equal(split, whole)


def _cfg(folder, **over):
    cfg = {
        'pretrain': {'model_name': 'vit_tiny', 'checkpoint_key': 'target_encoder', 'patch_size': 16, 'folder': folder,
                     'checkpoint': 'tiny-latest.pth.tar', 'write_tag': 'tiny', 'tubelet_size': 2, 'frames_per_clip': 8,
                     'uniform_power': True, 'use_sdpa': True, 'use_silu': False, 'tight_silu': False},
        'data': {'dataset_name': 'synthetic', 'num_classes': 4, 'root_path': None, 'image_folder': None, 'resolution': 64,
                 'synthetic_length': 16},
        'optimization': {'batch_size': 4, 'num_epochs': 2, 'weight_decay': 0.01, 'start_lr': 0.002, 'lr': 0.01, 'final_lr': 0.0,
                         'warmup': 0.5, 'use_bfloat16': False},
        'tag': 'tiny_eval',
    }
    cfg.update(over)
    return cfg


def test_main_two_epochs_and_resume(tmp_path):
    from jepa_amd.evals.image_classification_frozen import eval as E
    from jepa_amd.src.models import vision_transformer as vit
    from jepa_amd.src.models.attentive_pooler import AttentiveClassifier
    torch.manual_seed(1)
    enc = vit.vit_tiny(img_size=64, patch_size=16, num_frames=8, tubelet_size=2, uniform_power=True)
    torch.save({'target_encoder': {'module.backbone.' + k: v for k, v in enc.state_dict().items()}, 'epoch': 10},
               tmp_path / 'tiny-latest.pth.tar')
    torch.manual_seed(0)
    rec = E.main(_cfg(str(tmp_path)))
    out = tmp_path / "image_classification_frozen" / "tiny_eval"
    rows = list(csv.reader(open(out / "tiny_r0.csv")))
    assert rows[0] == ["epoch", "loss", "acc"] and [r[0] for r in rows[1:]] == ["1", "2"]
    assert [float(r[1]) for r in rows[1:]] == pytest.approx(rec['train_acc'], abs=1e-5)
    assert [float(r[2]) for r in rows[1:]] == pytest.approx(rec['val_acc'], abs=1e-5)
    ck = torch.load(out / "tiny-latest.pth.tar", map_location="cpu", weights_only=False)
    assert sorted(ck) == REFERENCE_CHECKPOINT_KEYS and ck['epoch'] == 2 and ck['scaler'] is None
    assert ck['batch_size'] == 4 and ck['world_size'] == 1 and ck['lr'] == 0.01
    assert list(ck['classifier']) == ['module.' + k for k in AttentiveClassifier(embed_dim=192, num_heads=3, num_classes=4).state_dict()]
    hist = rec['train_history']
    assert rec['start_epoch'] == 0 and len(hist) == 8            # 2 epochs x 16 items / batch 4
    assert all(np.isfinite(ls) for _, ls in hist)
    # resumed with resume_checkpoint: true and one more epoch to go, it continues from the saved epoch with the saved classifier
    cfg = _cfg(str(tmp_path), resume_checkpoint=True)
    cfg['optimization']['num_epochs'] = 3
    rec2 = E.main(cfg)
    assert rec2['start_epoch'] == 2 and len(rec2['train_history']) == 4 and len(rec2['val_acc']) == 1
    ck2 = torch.load(out / "tiny-latest.pth.tar", map_location="cpu", weights_only=False)
    assert ck2['epoch'] == 3
    step = ck2['opt']['state'][0]['step']
    assert int(step) == 12                                        # the optimizer state came from the checkpoint: 8 + 4 steps
