"""GPU: the frozen video-classification eval against tests/golden/eval_micro.npz, recorded from the reference's own ClipAggregation,
run_one_epoch and init_opt (tools/make_golden_eval.py) on the micro encoder of micro_step.npz.  S = 2 segments, V = 2 views, B = 2,
10 classes, attend_across_segments=True."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def rel_l2(a, b):
    a, b = torch.as_tensor(a).detach().float().cpu().reshape(-1), torch.as_tensor(b).detach().float().cpu().reshape(-1)
    return float((a - b).norm() / (b.norm() + 1e-12))


def _fixture():
    from tests.eval_golden_util import micro_clips
    z = np.load(os.path.join(GOLDEN, "eval_micro.npz"))
    S, V, B, C, iters, T, crop = (int(x) for x in z["dims"])
    train, train_labels, val, val_labels = micro_clips(int(z["clip_seed"]), S, V, B, C, iters, T, crop, z["clips_sha256"])
    return z, (S, V, B, C, iters, T), (train, train_labels, val, val_labels)


def _batch(clips, labels, T):
    idx = [torch.arange(s * T * 4, (s + 1) * T * 4, 4).repeat(clips.shape[2], 1) for s in range(clips.shape[0])]
    return [[clips[s, v] for v in range(clips.shape[1])] for s in range(clips.shape[0])], labels, idx


def _encoder():
    from functools import partial
    from jepa_amd.evals.video_classification_frozen.utils import ClipAggregation
    from jepa_amd.src.models.vision_transformer import VisionTransformer
    from tests.golden_util import load_micro, micro_weights
    enc = VisionTransformer(img_size=64, patch_size=16, num_frames=8, tubelet_size=2, embed_dim=64, depth=2, num_heads=2,
                            mlp_ratio=4, qkv_bias=True, norm_layer=partial(torch.nn.LayerNorm, eps=1e-6), uniform_power=True)
    enc.load_state_dict(micro_weights(load_micro())[0], strict=True)
    enc.to(DEV)
    for p in enc.parameters():
        p.requires_grad = False
    return enc, ClipAggregation(enc, tubelet_size=2, attend_across_segments=True).eval()


def _classifier(z, C):
    from jepa_amd.src.models.attentive_pooler import AttentiveClassifier
    clf = AttentiveClassifier(embed_dim=64, num_heads=2, depth=1, num_classes=C)
    assert list(clf.state_dict().keys()) == [str(k) for k in z["clf_keys"]]     # the reference's key list
    clf.load_state_dict({k: torch.from_numpy(z["clf0/" + k]) for k in clf.state_dict()}, strict=True)
    return clf.to(DEV)


class _FixtureEncoder(torch.nn.Module):
    """Returns the fixture's feature of each clip; a clip is identified by its position in the concatenated input."""

    def __init__(self, feat):
        super().__init__()
        self.feat, self.embed_dim, self.num_heads, self.num_patches = feat, feat.shape[2], 2, feat.shape[1]
        self.seen = 0

    def forward(self, x):
        f = self.feat[self.seen:self.seen + x.shape[0]]
        self.seen += x.shape[0]
        return f


@pytest.mark.parametrize("cap", [None, 3])
def test_clip_aggregation_of_the_fixture_features(cap):
    """Fed the reference encoder's features, ClipAggregation returns the reference's aggregation rounded to bf16, exactly (also when
    the frozen forward is split into calls of 3 clips)."""
    from jepa_amd.evals.video_classification_frozen.utils import ClipAggregation
    z, (S, V, B, C, iters, T), (_, _, val, val_labels) = _fixture()
    stub = _FixtureEncoder(torch.from_numpy(z["feat"]).to(DEV))
    agg = ClipAggregation(stub, tubelet_size=2, attend_across_segments=True)
    if cap is not None:
        agg.max_clips_per_call = cap
    clips, _, idx = _batch(val.to(DEV), val_labels, T)
    out = agg(clips, idx)
    assert stub.seen == S * V * B and len(out) == V
    for j in range(V):
        ref = torch.from_numpy(z[f"agg/v{j}"]).to(torch.bfloat16)
        assert out[j].dtype == torch.bfloat16 and torch.equal(out[j].cpu(), ref), j


def test_micro_eval_end_to_end_against_the_reference():
    """Features (rel-L2 <= 2e-2, the micro fixture's bound), logits of each view (<= 3e-2), then 3 training iterations and 1
    validation iteration of run_one_epoch with init_opt: every iteration's loss within 2e-2 relative, the same learning rates, the
    same accuracies, and the final classifier state (see the bound below)."""
    from jepa_amd.evals.video_classification_frozen.eval import init_opt, run_one_epoch
    z, (S, V, B, C, iters, T), (train, train_labels, val, val_labels) = _fixture()
    enc, agg = _encoder()
    vclips, _, vidx = _batch(val.to(DEV), val_labels, T)
    with torch.no_grad():
        feat = enc(torch.cat([torch.cat(xi, dim=0) for xi in vclips], dim=0))
        e = rel_l2(feat, z["feat"])
        assert e < 2e-2, ("features", e)
        views = agg(vclips, vidx)
    clf = _classifier(z, C)
    with torch.no_grad():
        logits = [clf(o) for o in views]
    for j, lg in enumerate(logits):
        e = rel_l2(lg, z[f"logits/v{j}"])
        assert e < 3e-2, ("logits", j, e)
    crit = torch.nn.CrossEntropyLoss()
    loss0 = float(sum(crit(lg, val_labels.to(DEV)) for lg in logits) / V)
    assert abs(loss0 - float(z["loss0"])) < 2e-2 * abs(float(z["loss0"]))

    start_lr, ref_lr, final_lr, warmup, num_epochs, wd, ipe = (float(x) for x in z["hp"])
    opt, scaler, sched, wd_sched = init_opt(classifier=clf, iterations_per_epoch=int(ipe), start_lr=start_lr, ref_lr=ref_lr,
                                            warmup=warmup, num_epochs=int(num_epochs), wd=wd, final_lr=final_lr, use_bfloat16=False)
    calls = []
    clf.register_forward_hook(lambda m, i, o: calls.append(o.detach().clone()))
    hist = []
    train_acc = run_one_epoch(DEV, True, agg, clf, scaler, opt, sched, wd_sched, [_batch(train[k], train_labels[k], T)
                                                                                  for k in range(iters)], False, 1, S, True,
                              history=hist)
    val_acc = run_one_epoch(DEV, False, agg, clf, scaler, opt, sched, wd_sched, [_batch(val, val_labels, T)], False, V, S, True)
    assert [lr for lr, _ in hist] == pytest.approx(list(z["iter_lr"]), rel=1e-12)
    losses = [ls for _, ls in hist] + [float(sum(crit(o, val_labels.to(DEV)) for o in calls[iters:]) / V)]
    for k, (mine, ref) in enumerate(zip(losses, z["iter_loss"])):
        assert abs(mine - float(ref)) < 2e-2 * abs(float(ref)), (k, mine, float(ref))
    assert [train_acc, val_acc] == pytest.approx(list(z["acc"]), abs=1e-9)
    # final state.  After three AdamW steps of lr ~1e-2 every parameter has moved by about +-lr per element (the init std is 2e-2), and
    # for small gradients the step's sign follows the gradient's sign, so bf16 gradient rounding shows most on the small biases: 1e-1
    # rel-L2 per tensor (measured worst 8.3e-2, norm2.bias; weights <= 2.7e-2).  The key half of xattn.kv.bias has a zero gradient
    # analytically (a constant added to every key cancels in the softmax), so its steps are rounding noise on both sides: bounded by
    # the learning-rate steps themselves
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
    assert worst[0] < 1e-1, (worst, errs)
