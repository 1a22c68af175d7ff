"""GPU: fine-tuning the video encoder end to end through the attentive probe.

The micro encoder of tests/golden/micro_step.npz at full length (masks=None) under an EncoderFineTuner, a seeded
AttentiveClassifier and cross-entropy:
  - every encoder parameter gradient against oracle.vjepa_oracle.encoder_forward + oracle.probe_oracle.attentive_classifier
    under torch autograd on the CPU, plain and through ClipAggregation (2 segments x 1 view, concatenated and not);
  - EncoderFineTuner.step: the layer-wise learning-rate wiring, three steps against torch.optim.AdamW, the bf16 / transposed
    shadows after a step;
  - main() of the fine-tuning eval on a micro synthetic config: loss, changed tensors, checkpoint round trip, resume;
  - the saved activations are released after an iteration.

Gradient bound.  Measured worst rel-L2 over the encoder's tensors (MI355X): 7.3e-3 (MEASURED_E2E in tests/finetune_util.py); the asserted bound is
twice that, 1.46e-2, under the cap of 7e-2 that tests/test_step_gpu.py::test_module_autograd_path_matches_oracle allows the same autograd path."""
import copy
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests.finetune_util import BOUND, DEV, _classifier, _clips, _encoder, _eval_cfg, _micro_vit, _oracle_grads, _worst  # noqa: E402
from tests.golden_util import MICRO, load_micro, micro_weights, rel_l2  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def setup():
    """One encoder under a tuner, one classifier, the fixture's weights for the oracle."""
    from jepa_amd.engine.finetune import EncoderFineTuner
    enc_w = micro_weights(load_micro())[0]
    enc = _encoder()
    tuner = EncoderFineTuner(enc, layer_decay=0.75)
    return enc_w, enc, tuner, _classifier()


def test_end_to_end_gradients_against_the_oracle(setup):
    enc_w, enc, tuner, clf = setup
    clips = _clips(1)[0]
    labels = torch.tensor([3, 7])
    assert enc._needs_grad() and all(p.grad.data_ptr() == tuner.arena.grad(n).data_ptr() for n, p in enc.named_parameters()
                                     if p.requires_grad)
    clf.zero_grad(set_to_none=True)
    loss = F.cross_entropy(clf(enc(clips.to(DEV))), labels.to(DEV))
    loss.backward()
    ref_loss, ref = _oracle_grads(enc_w, clf, [clips], labels, True)
    assert abs(float(loss.detach()) - ref_loss) < 2e-2 * abs(ref_loss)
    worst = _worst(tuner, ref)
    print("end-to-end worst encoder gradient rel-L2", worst)
    assert worst[0] < BOUND, worst


@pytest.mark.parametrize("across", [True, False])
def test_clip_aggregation_with_gradients(setup, across):
    from jepa_amd.evals.video_classification_frozen.utils import ClipAggregation
    enc_w, enc, tuner, clf = setup
    segs = _clips(2)
    labels = torch.tensor([1, 8])
    agg = ClipAggregation(enc, tubelet_size=2, attend_across_segments=across)
    x = [[c.to(DEV)] for c in segs]
    # -- under no_grad: what the frozen path gives, computed directly from the encoder's no-grad forward
    with torch.no_grad():
        out = agg(x)
        f = enc(torch.cat([c.to(DEV) for c in segs], dim=0))
    assert f.dtype == torch.bfloat16 and not f.requires_grad
    if across:
        assert len(out) == 1 and torch.equal(out[0], torch.cat([f[:2], f[2:]], dim=1)) and not out[0].requires_grad
    else:
        assert len(out) == 1 and len(out[0]) == 2 and torch.equal(out[0][0], f[:2]) and torch.equal(out[0][1], f[2:])
    # -- with gradients
    clf.zero_grad(set_to_none=True)
    out = agg(x)
    if across:
        assert out[0].requires_grad and out[0].shape == (2, 2 * MICRO["num_patches"], MICRO["embed_dim"])
        loss = F.cross_entropy(clf(out[0]), labels.to(DEV))
    else:
        loss = sum(F.cross_entropy(clf(o), labels.to(DEV)) for o in out[0]) / 2
    loss.backward()
    ref_loss, ref = _oracle_grads(enc_w, clf, segs, labels, across)
    assert abs(float(loss.detach()) - ref_loss) < 2e-2 * abs(ref_loss)
    worst = _worst(tuner, ref)
    print("aggregation across=%s worst encoder gradient rel-L2" % across, worst)
    assert worst[0] < BOUND, worst


def test_clip_aggregation_refuses_a_second_encoder_call_with_gradients(setup):
    from jepa_amd.evals.video_classification_frozen.utils import ClipAggregation
    _, enc, _, _ = setup
    agg = ClipAggregation(enc, tubelet_size=2, attend_across_segments=True)
    agg.max_clips_per_call = 3
    x = [[c.to(DEV)] for c in _clips(2)]
    with pytest.raises(ValueError, match="max_clips_per_call = 3"):
        agg(x)
    with torch.no_grad():
        assert agg(x)[0].shape[0] == 2       # the frozen path splits the call instead


def _backward(enc, clf, clips, labels, scale=1.0):
    clf.zero_grad(set_to_none=True)
    loss = F.cross_entropy(clf(enc(clips.to(DEV))), labels.to(DEV))
    (loss * scale).backward()
    return float(loss.detach())


def test_first_step_moves_every_tensor_by_its_layers_learning_rate():
    """Adam's first step is lr * g / (|g| + eps): with wd = 0, |dp| = lr * lr_scale wherever |g| >> eps = 1e-8.  The micro model's
    gradients of this loss are small (median |g| of blocks.0.attn.qkv.weight ~1e-6, where eps alone takes 0.8 % off the step), so
    the loss is scaled by 2^12 to keep eps below 1e-5 of the median gradient: the step then shows the learning rate alone."""
    from jepa_amd.engine.finetune import EncoderFineTuner
    enc, clf = _encoder(), _classifier()
    tuner = EncoderFineTuner(enc, layer_decay=0.75)
    _backward(enc, clf, _clips(1)[0], torch.tensor([3, 7]), scale=4096.0)
    before = {n: p.detach().clone() for n, p in enc.named_parameters()}
    lr = 1e-2
    tuner.step(lr, 0.0)
    assert tuner.opt_step == 1 and tuner.grad_stats()[1] == 0 and tuner.grad_stats()[0] > 0
    scale = {n: g["lr_scale"] for g in tuner.param_groups for p in g["params"] for n, q in enc.named_parameters() if q is p}
    depth = MICRO["depth"]
    for n, p in enc.named_parameters():
        if n == "pos_embed":
            assert torch.equal(p, before[n])
            continue
        lid = 0 if n.startswith("patch_embed") else int(n.split(".")[1]) + 1 if n.startswith("blocks") else depth + 1
        assert scale[n] == pytest.approx(0.75 ** (depth + 1 - lid))
        ratio = float(((p.detach() - before[n]).abs() / (lr * scale[n])).median())
        assert abs(ratio - 1.0) < 1e-3, (n, ratio)
        assert torch.equal(tuner.arena.bf16(n), p.detach().to(torch.bfloat16)), n


def test_three_steps_against_torch_adamw_and_the_shadows():
    from jepa_amd.engine import optstate
    from jepa_amd.engine.finetune import EncoderFineTuner
    enc, clf = _encoder(), _classifier()
    tuner = EncoderFineTuner(enc, layer_decay=0.75)
    ref = _micro_vit()
    ref.load_state_dict(micro_weights(load_micro())[0], strict=True)
    ref.pos_embed.requires_grad = False
    groups = optstate.layer_decay_groups(ref.named_parameters(), MICRO["depth"], 0.75)
    opt = torch.optim.AdamW([dict(g, params=[p for _, p in members]) for g, members in groups], lr=1.0, betas=(0.9, 0.999),
                            eps=1e-8, weight_decay=0.05)
    ref_p = dict(ref.named_parameters())
    labels = torch.tensor([3, 7])
    for k, (clips, lr) in enumerate(zip(_clips(3), (1e-3, 2e-3, 1.5e-3))):
        _backward(enc, clf, clips, labels)
        for n in tuner.arena.slots:
            ref_p[n].grad = tuner.arena.grad(n).detach().cpu().clone()
        for g in opt.param_groups:
            g["lr"] = lr * g["lr_scale"]
        opt.step()
        tuner.step(lr, 0.05)
        for n, p in enc.named_parameters():
            d = (p.detach().cpu() - ref_p[n].detach()).abs().max()
            assert torch.allclose(p.detach().cpu(), ref_p[n].detach(), rtol=1e-5, atol=1e-6), (k, n, float(d))
    assert tuner.opt_step == 3
    # the optimizer state is torch.optim.AdamW's: ids, moments and step
    sd, rsd = tuner.state_dict(), opt.state_dict()
    assert [g["params"] for g in sd["param_groups"]] == [g["params"] for g in rsd["param_groups"]]
    for i, st in rsd["state"].items():
        assert float(sd["state"][i]["step"]) == 3.0
        assert torch.allclose(sd["state"][i]["exp_avg"].cpu(), st["exp_avg"], rtol=1e-5, atol=1e-9), i
        assert torch.allclose(sd["state"][i]["exp_avg_sq"].cpu(), st["exp_avg_sq"], rtol=1e-5, atol=1e-12), i
    # the shadows are current: a fresh encoder loaded from the updated state dict computes the same bits, forward (bf16 shadows)
    # and backward (transposed shadows)
    fresh = _encoder({k: v.detach().cpu().clone() for k, v in enc.state_dict().items()})
    x = _clips(1)[0].to(DEV)
    with torch.no_grad():
        assert torch.equal(enc(x), fresh(x))
    _backward(enc, clf, x, labels)
    mine = {n: tuner.arena.grad(n).clone() for n in tuner.arena.slots}
    _backward(fresh, clf, x, labels)
    for n, p in fresh.named_parameters():
        if p.requires_grad:
            assert torch.equal(p.grad, mine[n]), (n, rel_l2(mine[n].cpu(), p.grad.cpu()))
    # a step on a non-finite gradient is skipped: weights, moments and the step count stay
    tuner.arena.grad("norm.bias")[0] = float("nan")
    snap = (tuner.arena.P.clone(), tuner.arena.M1.clone(), tuner.arena.M2.clone())
    tuner.step(1e-3, 0.05)
    assert tuner.opt_step == 3 and tuner.grad_stats()[1] == 1
    assert all(torch.equal(a, b) for a, b in zip(snap, (tuner.arena.P, tuner.arena.M1, tuner.arena.M2)))
    # state_dict round trip
    other = EncoderFineTuner(_encoder(), layer_decay=0.75)
    other.load_state_dict(copy.deepcopy(sd))
    assert other.opt_step == 3 and torch.equal(other.arena.M1, snap[1]) and torch.equal(other.arena.M2, snap[2])
    tuner.zero_grad()
    assert torch.count_nonzero(tuner.arena.G) == 0 and enc.norm.bias.grad.data_ptr() == tuner.arena.grad("norm.bias").data_ptr()


def test_an_iteration_releases_what_it_saved():
    from jepa_amd.engine.finetune import EncoderFineTuner
    enc, clf = _encoder(), _classifier()
    tuner = EncoderFineTuner(enc, layer_decay=0.75)
    clips, labels = _clips(1)[0].to(DEV), torch.tensor([3, 7]).to(DEV)

    def iteration():
        loss = F.cross_entropy(clf(enc(clips)), labels)
        loss.backward()
        tuner.step(1e-3, 0.05)

    iteration()     # workspaces, scratch buffers and the classifier's .grad tensors are allocated once
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    iteration()
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated() == before


# ------------------------------------------------------------------------------------------------------------------ the eval
def _final_state(folder):
    ck = torch.load(os.path.join(folder, "video_classification_finetune", "micro_ft", "micro-latest.pth.tar"),
                    map_location="cpu", weights_only=False)
    return ck, {**{"encoder." + k: v for k, v in ck["encoder"].items()}, **{"classifier." + k: v for k, v in ck["classifier"].items()}}


def test_main_trains_the_encoder_checkpoints_and_resumes(tmp_path, monkeypatch):
    from jepa_amd.evals.video_classification_finetune import eval as FT
    from jepa_amd.evals.video_classification_frozen import eval as E
    from jepa_amd.src.models import vision_transformer as vit
    monkeypatch.setattr(vit, "vit_micro", lambda **kw: _micro_vit(), raising=False)
    enc_w = micro_weights(load_micro())[0]
    tuners = []

    class Recording(FT.EncoderFineTuner):
        def __init__(self, *a, **kw):
            super().__init__(*a, **kw)
            tuners.append(self)

    monkeypatch.setattr(FT, "EncoderFineTuner", Recording)
    for run in ("a", "a2", "b"):
        os.makedirs(tmp_path / run)
        torch.save({'target_encoder': {'module.backbone.' + k: v for k, v in enc_w.items()}, 'epoch': 10},
                   tmp_path / run / 'micro-latest.pth.tar')

    # -- 8 uninterrupted iterations
    torch.manual_seed(0)
    rec = FT.main(_eval_cfg(str(tmp_path / "a")))
    hist = rec['train_history']
    assert len(hist) == 8 and hist[-1][1] < hist[0][1], hist
    ck, state_a = _final_state(tmp_path / "a")
    assert sorted(ck) == ['batch_size', 'classifier', 'encoder', 'encoder_opt', 'epoch', 'lr', 'opt', 'scaler', 'world_size']
    assert ck['epoch'] == 8 and list(ck['encoder']) == list(_micro_vit().state_dict())
    assert float(ck['encoder_opt']['state'][0]['step']) == 8.0
    tuner = tuners[-1]
    changed = 0
    for n in tuner.arena.slots:      # every tensor that has a gradient moved
        if torch.count_nonzero(tuner.arena.grad(n)) > 0:
            assert not torch.equal(ck['encoder'][n], enc_w[n]), n
            changed += 1
    assert changed == len(tuner.arena.slots)
    assert torch.equal(ck['encoder']['pos_embed'], enc_w['pos_embed'])
    # the frozen eval reads the fine-tuned encoder back
    loaded = E.load_pretrained(_micro_vit(), str(tmp_path / "a" / "video_classification_finetune" / "micro_ft" / "micro-latest.pth.tar"),
                               checkpoint_key='encoder')
    for n, p in tuner.encoder.state_dict().items():
        assert torch.equal(loaded.state_dict()[n], p.cpu()), n

    # -- the same run again: is the loop bit-reproducible?
    torch.manual_seed(0)
    FT.main(_eval_cfg(str(tmp_path / "a2")))
    _, state_a2 = _final_state(tmp_path / "a2")
    spread = {n: float((state_a[n].double() - state_a2[n].double()).abs().max()) for n in state_a}
    reproducible = all(torch.equal(state_a[n], state_a2[n]) for n in state_a)
    print("two uninterrupted runs bit-identical:", reproducible, "max spread", max(spread.values()))

    # -- 4 + 4: preempted at the start of epoch 5 (the 9th epoch call: a training and a validation call per epoch), then resumed
    real, calls = E.run_one_epoch, []

    def preempt(*a, **kw):
        calls.append(1)
        if len(calls) == 9:
            raise KeyboardInterrupt("preempted")
        return real(*a, **kw)

    monkeypatch.setattr(E, "run_one_epoch", preempt)
    torch.manual_seed(0)
    with pytest.raises(KeyboardInterrupt):
        FT.main(_eval_cfg(str(tmp_path / "b")))
    monkeypatch.setattr(E, "run_one_epoch", real)
    rec_b = FT.main(_eval_cfg(str(tmp_path / "b")), resume_preempt=True)
    assert rec_b['start_epoch'] == 4 and len(rec_b['train_history']) == 4
    assert [lr for lr, _ in rec_b['train_history']] == [lr for lr, _ in hist[4:]]
    _, state_b = _final_state(tmp_path / "b")
    if reproducible:      # measured on MI355X: this is the case that holds
        assert [ls for _, ls in rec_b['train_history']] == [ls for _, ls in hist[4:]]
        for n in state_a:
            assert torch.equal(state_b[n], state_a[n]), n
    else:                 # a third run may lie as far from the first as the second does, and somewhat further: 4 x their spread
        for n in state_a:
            d = float((state_b[n].double() - state_a[n].double()).abs().max())
            assert d <= 4 * spread[n] + 1e-12, (n, d, spread[n])
