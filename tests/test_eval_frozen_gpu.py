"""GPU: the frozen video-classification eval (jepa_amd/evals/video_classification_frozen) on the HIP path.

The attentive probe at the ViT-H/16-384 K400 16x8x3 shape (8 segments x 4608 tokens = 36 864 keys, past the single-workgroup
backward's 19 132) against the fp32 oracle; ClipAggregation's layout; the chunked frozen forward; one training and one validation
iteration at the real H/16-384 K400 geometry; and main() with a preemption and resume."""
import csv
import math
import os
from functools import partial

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"


def rel_l2(a, b):
    a, b = a.detach().float().reshape(-1), b.detach().float().reshape(-1)
    return float((a - b).norm() / (b.norm() + 1e-12))


def _micro_vit(**kw):
    """The micro encoder of the fixtures (D = 64, depth 2, 2 heads, 8 x 64 x 64 clips, 64 tokens per clip)."""
    from jepa_amd.src.models.vision_transformer import VisionTransformer
    args = dict(img_size=64, patch_size=16, num_frames=8, tubelet_size=2, embed_dim=64, depth=2, num_heads=2, mlp_ratio=4.0,
                qkv_bias=True, norm_layer=partial(torch.nn.LayerNorm, eps=1e-6), uniform_power=True)
    args.update(kw)
    return VisionTransformer(**args)


def test_probe_at_vith16_384_k400_shape_against_oracle():
    """B = 4 samples of 36 864 keys, D = 1280, 16 heads (head_dim 80), 400 classes: logits and every gradient against
    oracle/probe_oracle.py in fp32 (the bounds of tests/test_probe_gpu.py).  The probe backward runs the split kernels."""
    from oracle import probe_oracle as po
    from jepa_amd.src.models.attentive_pooler import AttentiveClassifier
    B, N, D, H, C = 4, 36864, 1280, 16, 400
    torch.manual_seed(7)
    m = AttentiveClassifier(embed_dim=D, num_heads=H, depth=1, num_classes=C).to(DEV)
    with torch.no_grad():
        for p in m.parameters():
            if p.dim() == 1:
                p.add_(0.05 * torch.randn_like(p))
    x = torch.randn(B, N, D, device=DEV)
    labels = torch.randint(0, C, (B,), device=DEV)
    w = {n: p.detach().clone() for n, p in m.named_parameters()}
    o_loss, o_logits, o_grads = po.probe_loss_and_grads(w, x, labels, H)
    logits = m(x)
    assert rel_l2(logits, o_logits) < 1e-2, rel_l2(logits, o_logits)
    loss = torch.nn.CrossEntropyLoss()(logits, labels)
    assert abs(float(loss.detach()) - float(o_loss)) < 2e-2 * max(1.0, abs(float(o_loss)))
    loss.backward()
    for n, p in m.named_parameters():
        if n not in o_grads:
            assert p.grad is None, n
            continue
        e = rel_l2(p.grad, o_grads[n])
        assert e < 2e-2, (n, e)


class _StubEncoder(torch.nn.Module):
    """Returns a fixed feature table row per clip (clip identity = its first pixel), fp32 like a plain torch encoder."""

    def __init__(self, table, N, D):
        super().__init__()
        self.table, self.embed_dim, self.num_heads, self.num_patches = table, D, 2, N
        self.calls = []

    def forward(self, x):
        self.calls.append(x.shape[0])
        return self.table[x[:, 0, 0, 0, 0].long()]


@pytest.mark.parametrize("across", [True, False])
def test_clip_aggregation_layout(across):
    """The aggregated tensors equal the reference's torch.cat / reshape layout (utils.py:125-159) of the encoder features rounded
    to bf16, exactly; with a small call cap the encoder runs in several calls and nothing changes."""
    from jepa_amd.evals.video_classification_frozen.utils import ClipAggregation
    S, V, B, N, D, T = 3, 2, 4, 16, 64, 4
    table = torch.randn(S * V * B, N, D, device=DEV)
    clips = [[torch.zeros(B, 3, T, 8, 8, device=DEV) for _ in range(V)] for _ in range(S)]
    for i in range(S):
        for j in range(V):
            clips[i][j][:, 0, 0, 0, 0] = torch.arange(B, device=DEV, dtype=torch.float32) + (i * V + j) * B
    # the reference's arithmetic on the same features
    feats = table.to(torch.bfloat16)
    eff_B = B * V
    ref = [[feats[i * eff_B + j * B:i * eff_B + (j + 1) * B] for i in range(S)] for j in range(V)]
    if across:
        ref = [torch.cat([o.reshape(B, T // 2, N // (T // 2), D) for o in r], dim=1).flatten(1, 2) for r in ref]
    for cap in (None, 5):
        enc = _StubEncoder(table, N, D)
        agg = ClipAggregation(enc, tubelet_size=2, attend_across_segments=across)
        if cap is not None:
            agg.max_clips_per_call = cap
        out = agg(clips)
        assert enc.calls == ([S * V * B] if cap is None else [5, 5, 5, 5, 4])
        assert len(out) == V
        for j in range(V):
            if across:
                assert out[j].dtype == torch.bfloat16 and out[j].shape == (B, S * N, D)
                assert torch.equal(out[j], ref[j]), (cap, j)
            else:
                assert len(out[j]) == S
                for i in range(S):
                    assert torch.equal(out[j][i], ref[j][i]), (cap, i, j)


def test_chunked_frozen_forward_equals_one_call():
    """The frozen forward split into several encoder calls (the real cap keeps fc1's M x 4D output below 2^31 elements: 91
    ViT-H/16-384 clips) gives the features of one call, bit for bit."""
    from jepa_amd.evals.video_classification_frozen.utils import ClipAggregation, max_clips_per_call
    assert max_clips_per_call(4 * 1280, 4608) == 91 and 91 * 4608 * 4 * 1280 < 2 ** 31
    torch.manual_seed(3)
    enc = _micro_vit().to(DEV)
    for p in enc.parameters():
        p.requires_grad = False
    S, V, B = 2, 3, 2
    g = torch.Generator().manual_seed(4)
    clips = [[torch.randn(B, 3, 8, 64, 64, generator=g).to(DEV) for _ in range(V)] for _ in range(S)]
    with torch.no_grad():
        one = ClipAggregation(enc, attend_across_segments=True)(clips)
        agg = ClipAggregation(enc, attend_across_segments=True)
        agg.max_clips_per_call = 5   # 12 clips in calls of 5, 5, 2
        chunked = agg(clips)
    for a, b in zip(one, chunked):
        assert a.shape == (B, S * 64, 64) and torch.equal(a, b)


def test_train_and_val_iteration_at_vith16_384_k400_geometry():
    """One training and one validation iteration of run_one_epoch at the real H/16-384 K400 16x8x3 geometry (a depth-2 ViT-H
    trunk): 8 x 1 clips per sample to train, 8 x 3 to validate (96 clips: two encoder calls), B = 4, 36 864 probe keys."""
    from jepa_amd.evals.video_classification_frozen.eval import init_opt, run_one_epoch
    from jepa_amd.evals.video_classification_frozen.utils import ClipAggregation
    from jepa_amd.src.models.attentive_pooler import AttentiveClassifier
    from jepa_amd.src.models.vision_transformer import VisionTransformer
    torch.manual_seed(0)
    vit = VisionTransformer(img_size=384, patch_size=16, num_frames=16, tubelet_size=2, embed_dim=1280, depth=2, num_heads=16,
                            norm_layer=partial(torch.nn.LayerNorm, eps=1e-6), uniform_power=True).to(DEV)
    enc = ClipAggregation(vit, tubelet_size=2, attend_across_segments=True).to(DEV).eval()
    for p in enc.parameters():
        p.requires_grad = False
    assert enc.max_clips_per_call == 91
    clf = AttentiveClassifier(embed_dim=1280, num_heads=16, depth=1, num_classes=400).to(DEV)
    opt, scaler, sched, wd_sched = init_opt(clf, iterations_per_epoch=1, start_lr=1e-3, ref_lr=1e-3, warmup=0, num_epochs=1,
                                            wd=0.01)
    B, S = 4, 8
    labels = torch.randint(0, 400, (B,))
    idx = [torch.arange(16) for _ in range(S)]

    def batch(V):
        return [[torch.randn(B, 3, 16, 384, 384, device=DEV) for _ in range(V)] for _ in range(S)], labels, idx

    hist = []
    acc = run_one_epoch(DEV, True, enc, clf, scaler, opt, sched, wd_sched, [batch(1)], False, 1, S, True, history=hist)
    assert len(hist) == 1 and math.isfinite(hist[0][1]) and 0.0 <= acc <= 100.0
    assert all(p.grad is None for p in clf.parameters())   # zero_grad after the step
    vacc = run_one_epoch(DEV, False, enc, clf, scaler, opt, sched, wd_sched, [batch(3)], False, 3, S, True)
    assert 0.0 <= vacc <= 100.0
    assert all(torch.isfinite(p).all() for p in clf.parameters())


REFERENCE_CHECKPOINT_KEYS = ['batch_size', 'classifier', 'epoch', 'lr', 'opt', 'scaler', 'world_size']   # eval.py:247-255


def _micro_cfg(folder):
    return {
        'pretrain': {'model_name': 'vit_micro', 'checkpoint_key': 'target_encoder', 'patch_size': 16, 'folder': folder,
                     'checkpoint': 'micro-latest.pth.tar', 'write_tag': 'micro', 'tubelet_size': 2, 'frames_per_clip': 8,
                     'uniform_power': True, 'use_sdpa': True, 'use_silu': False, 'tight_silu': False},
        'data': {'dataset_type': 'synthetic', 'dataset_train': None, 'dataset_val': None, 'num_classes': 4, 'frames_per_clip': 8,
                 'num_segments': 2, 'num_views_per_segment': 2, 'synthetic_length': 16},
        'optimization': {'resolution': 64, 'batch_size': 4, 'attend_across_segments': True, 'num_epochs': 2,
                         'weight_decay': 0.01, 'start_lr': 0.002, 'lr': 0.01, 'final_lr': 0.0, 'warmup': 0.5,
                         'use_bfloat16': False},
        'tag': 'micro_eval',
    }


def test_main_two_epochs_with_preemption_and_resume(tmp_path, monkeypatch):
    from jepa_amd.evals.video_classification_frozen import eval as E
    from jepa_amd.src.models import vision_transformer as vit
    from jepa_amd.src.models.attentive_pooler import AttentiveClassifier
    monkeypatch.setattr(vit, "vit_micro", lambda **kw: _micro_vit(**{k: v for k, v in kw.items() if k != "use_sdpa"}),
                        raising=False)
    torch.manual_seed(1)
    enc_sd = {'module.backbone.' + k: v for k, v in _micro_vit().state_dict().items()}
    for run in ("a", "b"):
        os.makedirs(tmp_path / run)
        torch.save({'target_encoder': enc_sd, 'epoch': 10}, tmp_path / run / 'micro-latest.pth.tar')

    # uninterrupted (the classifier's initialisation draws from the global generator, seeded once at import as in the reference:
    # both runs start from the same seed so that the resumed run can be compared with this one)
    torch.manual_seed(0)
    rec = E.main(_micro_cfg(str(tmp_path / "a")))
    out = tmp_path / "a" / "video_classification_frozen" / "micro_eval"
    rows = list(csv.reader(open(out / "micro_r0.csv")))
    assert rows[0] == ["epoch", "loss", "acc"] and [r[0] for r in rows[1:]] == ["1", "2"]
    assert [float(r[1]) for r in rows[1:]] == pytest.approx(rec['train_acc'], abs=1e-5)
    assert [float(r[2]) for r in rows[1:]] == pytest.approx(rec['val_acc'], abs=1e-5)
    ck = torch.load(out / "micro-latest.pth.tar", map_location="cpu", weights_only=False)
    assert sorted(ck) == REFERENCE_CHECKPOINT_KEYS and ck['epoch'] == 2 and ck['scaler'] is None
    ref_keys = ['module.' + k for k in AttentiveClassifier(embed_dim=64, num_heads=2, num_classes=4).state_dict()]
    assert list(ck['classifier']) == ref_keys
    hist = rec['train_history']
    assert len(hist) == 8   # 2 epochs x 16 items / batch 4
    assert hist[-1][1] < hist[0][1], [h[1] for h in hist]

    # preempted after epoch 1, then resumed: the schedules are replayed start_epoch * ipe times
    real = E.run_one_epoch
    calls = []

    def preempt(*a, **kw):
        calls.append(1)
        if len(calls) == 3:
            raise KeyboardInterrupt("preempted")
        return real(*a, **kw)

    monkeypatch.setattr(E, "run_one_epoch", preempt)
    torch.manual_seed(0)
    with pytest.raises(KeyboardInterrupt):
        E.main(_micro_cfg(str(tmp_path / "b")))
    monkeypatch.setattr(E, "run_one_epoch", real)
    rec_b = E.main(_micro_cfg(str(tmp_path / "b")), resume_preempt=True)
    assert rec_b['start_epoch'] == 1 and len(rec_b['train_history']) == 4
    assert rec_b['train_history'][0][0] == hist[4][0]
    assert rec_b['train_history'][0][1] == pytest.approx(hist[4][1], rel=1e-2)
    rows_b = list(csv.reader(open(tmp_path / "b" / "video_classification_frozen" / "micro_eval" / "micro_r0.csv")))
    assert [r[0] for r in rows_b if r[0] != "epoch"] == ["1", "2"]
