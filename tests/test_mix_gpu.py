"""GPU: mixup / cutmix / label smoothing of encoder fine-tuning, from the two kernels up to the eval.

  - vj_clip_mix against the float64 restatement of tests/mix_ref_util.py: own and swapped elements bit for bit, blended ones within
    2^-22 (|lam x_i| + |(1 - lam) x_j|) (three fp32 roundings), guard elements around the buffer untouched;
  - vj_soft_ce against float64: loss, gradient and soft-max, and their structure (rows of the gradient sum to 0, probabilities
    are not negative, eps = 0 with lam = 1 is the hard cross-entropy);
  - SoftTargetCrossEntropy's backward;
  - the micro encoder under an EncoderFineTuner on mixed clips and soft targets against the oracle under torch autograd;
  - main() of the fine-tuning eval with the `mix` section.

Bounds of vj_soft_ce.  Measured on MI355X over every case of mix_ref_util.soft_ce_cases at C in SOFT_CE_CLASSES and both row
strides, against the float64 reference: MEASURED_SOFT_CE below (worst |loss - ref| / max(1, |ref|), worst |dlogits - ref|; the
soft-max output is held to the gradient's bound).  Asserted: twice the measured figure (the margin for box-to-box differences in
the exponential's and logarithm's code path that the other per-element tests of this package use), capped at 1e-5.  The cap is one
that torch's own fp32 log_softmax-based soft cross-entropy meets against float64 on these very inputs, C = 8142 with +-80 logits
included (tests/test_mix_host.py::test_torch_fp32_soft_cross_entropy_stays_inside_the_cap: worst 7.6e-7 / 1.6e-6): the inputs
were not shrunk and the cap was not widened."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests import mix_ref_util as R  # noqa: E402
from tests.golden_util import MICRO, load_micro, micro_weights  # noqa: E402
from tests.finetune_util import BOUND, C, _classifier, _clips, _encoder, _eval_cfg, _micro_vit, _oracle_grads, _worst  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"

# measured on MI355X: (worst |loss - ref| / max(1, |ref|), worst |dlogits - ref|) of vj_soft_ce against float64
# (the loss figure is C = 1 with a logit of 80, where the loss is 0 and its three terms cancel; the gradient figure C = 400; the
# soft-max output was within 7.89e-8)
MEASURED_SOFT_CE = (2.31e-7, 8.10e-8)
LOSS_BOUND, GRAD_BOUND = (min(2 * m, R.SOFT_CE_CAP) for m in MEASURED_SOFT_CE)          # 4.62e-7, 1.62e-7


# ------------------------------------------------------------------------------------------------------------------- vj_clip_mix
GUARD = 64      # floats in front of and behind the clips (256 bytes: the clips stay 16-byte aligned)


def _plans(B, H, W):
    """name -> (lam [B], box [B,4]); `exact`: every element keeps its own or takes its partner's bits."""
    one, empty = np.ones(B, np.float32), np.zeros((B, 4), np.int32)

    def boxes(*rows):
        return np.array([rows[b % len(rows)] for b in range(B)], np.int32)

    return {
        "identity": (one, empty),
        "mixup 0.3": (np.full(B, 0.3, np.float32), empty),
        "per-sample lam": (np.array([0.3, 0.9, 1.0, 0.5][:B], np.float32), empty),
        "cutmix, edges off the chunks": (one, boxes((1, H - 1, 3, W - 3))),
        "full swap": (one, boxes((0, H, 0, W))),
        "empty box, lam < 1": (np.full(B, 0.6, np.float32), boxes((2, 2, 0, W), (0, H, 5, 5))),
        "one column": (one, boxes((0, H, 5, 6))),
        "per-sample lam and boxes": (np.array([1.0, 0.25, 0.7, 1.0][:B], np.float32),
                                     boxes((1, H - 1, 3, W - 3), (0, 2, 0, 4), (H - 1, H, 1, W - 1), (0, 0, 0, 0))),
    }


@pytest.mark.parametrize("B", [1, 2, 3, 4])
@pytest.mark.parametrize("shape", [(3, 8, 8), (6, 64, 64), (2, 5, 12)], ids=lambda s: "x".join(map(str, s)))
def test_clip_mix_against_float64(shape, B):
    from jepa_amd.hip import ops
    P, H, W = shape
    rng = np.random.RandomState(1000 * B + P * H * W)
    n = B * P * H * W
    for name, (lam, box) in _plans(B, H, W).items():
        x = rng.randn(B, P, H, W).astype(np.float32)
        if (lam == 1).all():                      # the bit-exact plans carry a negative zero and a denormal in every sample
            x[:, 0, 0, 0] = -0.0
            x[:, P - 1, H - 1, W - 2] = np.float32(1e-40)
            assert (x[:, P - 1, H - 1, W - 2] != 0).all()
        buf = torch.cat([torch.full((GUARD,), 3.5), torch.from_numpy(x).reshape(-1), torch.full((GUARD,), -7.25)]).to(DEV)
        view = buf[GUARD:GUARD + n].view(B, P, H, W)
        assert view.data_ptr() % 16 == 0
        lam_d, box_d = ops.mix_tables(lam, box, H, W, DEV)
        out = ops.clip_mix(view, lam_d, box_d)
        assert out.data_ptr() == view.data_ptr()
        got = buf.cpu().numpy()
        assert (got[:GUARD] == 3.5).all() and (got[GUARD + n:] == -7.25).all(), (name, "guard elements")
        got = got[GUARD:GUARD + n].reshape(B, P, H, W)
        try:
            worst = R.check_clip_mix(got, x, lam, box)
        except AssertionError as e:
            raise AssertionError(f"{name}: {e}") from None
        if name in ("identity", "full swap"):
            want = x if name == "identity" or B == 1 else np.where(np.arange(B)[:, None, None, None] * 2 + 1 == B, x, x[::-1])
            assert np.array_equal(got.view(np.int32), want.view(np.int32)), name
        if B % 2:
            assert np.array_equal(got[B // 2].view(np.int32), x[B // 2].view(np.int32)), (name, "the middle sample")
        assert torch.equal(lam_d.cpu(), torch.from_numpy(lam)) and torch.equal(box_d.cpu(), torch.from_numpy(box))
        if worst:
            print(f"B={B} {shape} {name}: worst blended error {worst:.3f} of the bound")


def test_clip_mix_on_clip_shaped_views_and_its_argument_checks():
    from jepa_amd.hip import ops
    x = torch.randn(2, 3, 4, 8, 8, device=DEV)
    keep = x.clone()
    lam, box = ops.mix_tables([1.0, 1.0], [[2, 6, 0, 8]] * 2, 8, 8, DEV)
    ops.clip_mix(x, lam, box)                      # [B,3,T,S,S]: the box in every frame and channel
    assert torch.equal(x[0, :, :, 2:6], keep[1, :, :, 2:6]) and torch.equal(x[1, :, :, 2:6], keep[0, :, :, 2:6])
    assert torch.equal(x[:, :, :, :2], keep[:, :, :, :2]) and torch.equal(x[:, :, :, 6:], keep[:, :, :, 6:])
    with pytest.raises(ValueError, match="not a table uploaded by ops.mix_tables"):
        ops.clip_mix(x, lam, box.clone())
    with pytest.raises(ValueError, match="validated for"):
        ops.clip_mix(torch.zeros(2, 3, 16, 16, device=DEV), lam, box)
    with pytest.raises(ValueError, match="do not match"):
        ops.clip_mix(torch.zeros(3, 3, 8, 8, device=DEV), lam, box)
    with pytest.raises(ValueError, match="contiguous"):
        ops.clip_mix(x.transpose(1, 2), lam, box)
    with pytest.raises(TypeError):
        ops.clip_mix(x.double(), lam, box)
    from jepa_amd.hip.lib import HipKernelError
    odd = torch.zeros(2, 3, 8, 6, device=DEV)
    with pytest.raises(HipKernelError, match="multiple of 4"):
        ops.clip_mix(odd, *ops.mix_tables([1.0, 1.0], [[0, 0, 0, 0]] * 2, 8, 6, DEV))
    assert ops.clip_mix(x[:0], *ops.mix_tables([], np.zeros((0, 4)), 8, 8, DEV)).shape[0] == 0      # no sample: no launch


# -------------------------------------------------------------------------------------------------------------------- vj_soft_ce
_measured = {}


@pytest.mark.parametrize("pad", [0, 3], ids=["ld=C", "ld=C+3"])
@pytest.mark.parametrize("C_", R.SOFT_CE_CLASSES)
def test_soft_ce_against_float64(C_, pad):
    from jepa_amd.hip import ops
    worst = [0.0, 0.0, 0.0]
    for name, z, a, b, lam, eps in R.soft_ce_cases(C_):
        Rr = z.shape[0]
        ref = R.soft_ce_ref(z, a, b, lam, eps)
        store = torch.full((Rr, C_ + pad), float("nan"))
        store[:, :C_] = torch.from_numpy(z)
        logits = store.to(DEV)[:, :C_]
        assert logits.stride(0) == C_ + pad
        tables = ops.soft_ce_tables(a, b, lam, C_, DEV)
        loss, dl, p = ops.soft_ce(logits, *tables, float(eps), probs=True)
        assert loss.shape == (Rr,) and dl.shape == (Rr, C_) and p.shape == (Rr, C_) and dl.is_contiguous()
        try:
            errs = R.check_soft_ce(loss.cpu().numpy(), dl.cpu().numpy(), p.cpu().numpy(), ref, LOSS_BOUND, GRAD_BOUND)
        except AssertionError as e:
            raise AssertionError(f"C={C_} {name}: {e}") from None
        worst = [max(w, e) for w, e in zip(worst, errs)]
        # without the soft-max output: the same loss and gradient, bit for bit
        loss2, dl2, none = ops.soft_ce(logits, *tables, float(eps))
        assert none is None and torch.equal(loss2, loss) and torch.equal(dl2, dl)
        if eps == 0 and (lam == 1).all():
            # the hard cross-entropy's reference, and its gradient
            zd = torch.tensor(z, dtype=torch.float64, requires_grad=True)
            hard = F.cross_entropy(zd, torch.from_numpy(a).long(), reduction='none')
            hard.sum().backward()
            el, ed, _ = R.soft_ce_errors(loss.cpu().numpy(), dl.cpu().numpy(), None, (hard.detach().numpy(), zd.grad.numpy(), None))
            assert el <= LOSS_BOUND and ed <= GRAD_BOUND, (name, "hard cross-entropy", el, ed)
    _measured[(C_, pad)] = worst
    print(f"vj_soft_ce C={C_} ld=C+{pad}: worst loss error {worst[0]:.3e} (rel. to max(1, |ref|)), worst dlogits error {worst[1]:.3e}, "
          f"worst probs error {worst[2]:.3e}")
    if len(_measured) == 2 * len(R.SOFT_CE_CLASSES):
        tot = [max(w[k] for w in _measured.values()) for k in range(3)]
        print(f"vj_soft_ce over all cases: loss {tot[0]:.3e}, dlogits {tot[1]:.3e}, probs {tot[2]:.3e}; asserted {LOSS_BOUND:.3e} / {GRAD_BOUND:.3e}")


def test_soft_ce_argument_checks():
    from jepa_amd.hip import ops
    z = torch.randn(3, 10, device=DEV)
    a, b, lam = ops.soft_ce_tables([1, 2, 3], [3, 2, 1], [0.5, 1.0, 0.0], 10, DEV)
    loss, dl, p = ops.soft_ce(z, a, b, lam, 0.1)
    assert p is None and loss.shape == (3,)
    with pytest.raises(ValueError, match="not a table uploaded by ops.soft_ce_tables"):
        ops.soft_ce(z, a.clone(), b, lam, 0.1)
    with pytest.raises(ValueError, match="validated for 10 classes"):
        ops.soft_ce(torch.randn(3, 12, device=DEV), a, b, lam, 0.1)
    with pytest.raises(ValueError, match="smoothing"):
        ops.soft_ce(z, a, b, lam, 1.0)
    with pytest.raises(ValueError, match="expected a contiguous"):
        ops.soft_ce(z[:2], a, b, lam, 0.1)
    with pytest.raises(ValueError, match="unit column stride"):
        ops.soft_ce(torch.randn(10, 3, device=DEV).t(), a, b, lam, 0.1)
    with pytest.raises(TypeError):
        ops.soft_ce(z.double(), a, b, lam, 0.1)
    empty = ops.soft_ce(z[:0], *ops.soft_ce_tables([], [], [], 10, DEV), 0.1, probs=True)
    assert empty[0].shape == (0,) and empty[1].shape == (0, 10) and empty[2].shape == (0, 10)


# ---------------------------------------------------------------------------------------------------------------------- autograd
def test_soft_target_cross_entropy_backward():
    from jepa_amd.evals.mix import SoftTargetCrossEntropy
    from jepa_amd.hip import ops
    Rr, Cc, g = 3, 65, 2.5
    rng = np.random.RandomState(5)
    z = (3.0 * rng.randn(Rr, Cc)).astype(np.float32)
    a, b, lam = np.array([4, 9, 64], np.int32), np.array([7, 9, 0], np.int32), np.array([0.3, 0.8, 1.0], np.float32)
    tables = ops.soft_ce_tables(a, b, lam, Cc, DEV)
    w = torch.tensor(z, device=DEV, requires_grad=True)
    logits = w * 1.0                                 # a non-leaf, as the classifier's output is
    loss, p = SoftTargetCrossEntropy.apply(logits, *tables, 0.1, True)
    assert loss.requires_grad and not p.requires_grad and loss.dim() == 0
    rows, dl, p2 = ops.soft_ce(logits.detach(), *tables, 0.1, probs=True)
    assert torch.equal(loss.detach(), rows.mean()) and torch.equal(p, p2)
    (loss * g).backward()
    assert torch.equal(w.grad, dl * (torch.tensor(g, device=DEV) / Rr))            # dlogits * g / R, the one torch multiply
    ref_loss, ref_dl, _ = R.soft_ce_ref(z, a, b, lam, np.float32(0.1))
    assert abs(float(loss.detach()) - ref_loss.mean()) <= LOSS_BOUND * max(1.0, abs(ref_loss.mean()))
    assert np.abs(w.grad.cpu().numpy().astype(np.float64) - ref_dl * g / Rr).max() <= GRAD_BOUND * g / Rr + 2.0 ** -24
    # without the soft-max output, and under no_grad
    loss2, none = SoftTargetCrossEntropy.apply(logits.detach().requires_grad_(), *tables, 0.1)
    assert none is None and torch.equal(loss2.detach(), loss.detach())
    with torch.no_grad():
        assert not SoftTargetCrossEntropy.apply(logits, *tables, 0.1)[0].requires_grad


# -------------------------------------------------------------------------------------------------- end to end on the micro encoder
@pytest.fixture(scope="module")
def setup():
    from jepa_amd.engine.finetune import EncoderFineTuner
    enc_w = micro_weights(load_micro())[0]
    enc = _encoder()
    tuner = EncoderFineTuner(enc, layer_decay=0.75)
    return enc_w, enc, tuner, _classifier()


EPS = np.float32(0.1)
E2E_PLANS = {      # B = 2: (pixel lam, box, the target's lam)
    "mixup": (np.full(2, 0.3, np.float32), np.zeros((2, 4), np.int32), np.full(2, 0.3, np.float32)),
    "cutmix": (np.ones(2, np.float32), np.tile(np.array([5, 37, 10, 50], np.int32), (2, 1)),
               np.full(2, 1.0 - 32 * 40 / 4096.0, np.float32)),
}


@pytest.mark.parametrize("across", [True, False])
@pytest.mark.parametrize("plan", list(E2E_PLANS))
def test_mixed_clips_and_soft_targets_against_the_oracle(setup, plan, across):
    """Two segments of the fixture's 2 clips [2,3,8,64,64], mixed on the device with one plan and aggregated; the oracle gets the
    clips mixed in float64 and the soft targets as class probabilities."""
    from jepa_amd.evals.mix import SoftTargetCrossEntropy
    from jepa_amd.evals.video_classification_frozen.utils import ClipAggregation
    from jepa_amd.hip import ops
    enc_w, enc, tuner, clf = setup
    pixel_lam, box, lam = E2E_PLANS[plan]
    segs = _clips(2)
    labels = np.array([1, 8], np.int32)
    S = segs[0].shape[-1]
    # -- the reference's inputs
    mixed = []
    for c in segs:
        x = c.numpy().reshape(2, -1, S, S)
        ref, _, _ = R.clip_mix_ref(x, pixel_lam, box)
        mixed.append(torch.from_numpy(ref.astype(np.float32)).view_as(c))
        assert not torch.equal(mixed[-1], c)
    target = torch.from_numpy(R.soft_target(labels, labels[::-1], lam, EPS, C)).float()
    # -- the device
    lam_d, box_d = ops.mix_tables(pixel_lam, box, S, S, DEV)
    x = [[c.to(DEV)] for c in segs]
    for (v,), c in zip(x, segs):
        ops.clip_mix(v, lam_d, box_d)
        R.check_clip_mix(v.cpu().numpy().reshape(2, -1, S, S), c.numpy().reshape(2, -1, S, S), pixel_lam, box)
    tables = ops.soft_ce_tables(labels, labels[::-1].copy(), lam, C, DEV)
    agg = ClipAggregation(enc, tubelet_size=2, attend_across_segments=across)
    clf.zero_grad(set_to_none=True)
    out = agg(x)
    views = out if across else out[0]
    loss = sum(SoftTargetCrossEntropy.apply(clf(o), *tables, float(EPS))[0] for o in views) / len(views)
    loss.backward()
    ref_loss, ref = _oracle_grads(enc_w, clf, mixed, target, across)
    worst = _worst(tuner, ref)
    print(f"{plan} across={across}: loss {float(loss):.6f} oracle {ref_loss:.6f} rel {abs(float(loss) - ref_loss) / abs(ref_loss):.2e}; "
          f"worst encoder gradient rel-L2 {worst}")
    assert abs(float(loss.detach()) - ref_loss) < 2e-2 * abs(ref_loss)
    assert worst[0] < BOUND, worst


# ---------------------------------------------------------------------------------------------------------------------- the eval
def test_main_with_mix(tmp_path, monkeypatch):
    from jepa_amd.evals.video_classification_finetune import eval as FT
    from jepa_amd.evals.video_classification_frozen import eval as E
    from jepa_amd.hip import ops
    from jepa_amd.src.models import vision_transformer as vit
    monkeypatch.setattr(vit, "vit_micro", lambda **kw: _micro_vit(), raising=False)
    enc_w = micro_weights(load_micro())[0]
    launches = []
    real_mix = ops.clip_mix
    monkeypatch.setattr(ops, "clip_mix", lambda *a, **kw: (launches.append(1), real_mix(*a, **kw))[1])

    def run(name, mix, epochs=4, **kw):
        os.makedirs(tmp_path / name, exist_ok=True)
        torch.save({'target_encoder': {'module.backbone.' + k: v for k, v in enc_w.items()}, 'epoch': 10},
                   tmp_path / name / 'micro-latest.pth.tar')
        cfg = _eval_cfg(str(tmp_path / name))
        cfg['optimization']['num_epochs'] = epochs
        if mix is not None:
            cfg['optimization']['finetune']['mix'] = mix
        torch.manual_seed(0)
        del launches[:]
        return FT.main(cfg, **kw)

    plain = run("plain", None)
    assert not launches
    off = run("off", {'mixup_alpha': 0.0, 'cutmix_alpha': 0.0, 'label_smoothing': 0.0})
    assert not launches and off == plain                # all three knobs at 0: the record of the run without the key
    recipe = {'mixup_alpha': 0.8, 'cutmix_alpha': 1.0, 'prob': 1.0, 'switch_prob': 0.5, 'label_smoothing': 0.1, 'seed': 0}
    mixed = run("mixed", recipe)
    assert len(launches) == 4 * 2                       # 4 training iterations of 2 segments; validation mixes nothing
    losses, base = [ls for _, ls in mixed['train_history']], [ls for _, ls in plain['train_history']]
    assert len(losses) == 4 and all(np.isfinite(losses)) and all(a != b for a, b in zip(losses, base))
    assert [lr for lr, _ in mixed['train_history']] == [lr for lr, _ in plain['train_history']]
    ck = torch.load(tmp_path / "mixed" / "video_classification_finetune" / "micro_ft" / "micro-latest.pth.tar", map_location="cpu",
                    weights_only=False)
    assert ck['epoch'] == 4 and sum(not torch.equal(v, enc_w[n]) for n, v in ck['encoder'].items()) == len(enc_w) - 1
    # smoothing alone: the soft-target loss without a clip_mix launch
    smooth = run("smooth", {'mixup_alpha': 0.0, 'cutmix_alpha': 0.0}, epochs=1)
    assert not launches and smooth['train_history'][0][1] != plain['train_history'][0][1]
    # preempted at the start of epoch 3 (the 5th epoch call), then resumed: the schedule continues and the run ends
    real, calls = E.run_one_epoch, []

    def preempt(*a, **kw):
        calls.append(1)
        if len(calls) == 5:
            raise KeyboardInterrupt("preempted")
        return real(*a, **kw)

    monkeypatch.setattr(E, "run_one_epoch", preempt)
    with pytest.raises(KeyboardInterrupt):
        run("resumed", recipe)
    monkeypatch.setattr(E, "run_one_epoch", real)
    cfg = _eval_cfg(str(tmp_path / "resumed"))
    cfg['optimization']['num_epochs'] = 4
    cfg['optimization']['finetune']['mix'] = recipe
    rec = FT.main(cfg, resume_preempt=True)
    assert rec['start_epoch'] == 2 and len(rec['train_history']) == 2 and all(np.isfinite(ls) for _, ls in rec['train_history'])
    assert [lr for lr, _ in rec['train_history']] == [lr for lr, _ in mixed['train_history'][2:]]
    # the first two epochs of the preempted run saw the plans of the uninterrupted one; the resumed ones draw a fresh stream
    ck = torch.load(tmp_path / "resumed" / "video_classification_finetune" / "micro_ft" / "micro-latest.pth.tar", map_location="cpu",
                    weights_only=False)
    assert ck['epoch'] == 4 and float(ck['encoder_opt']['state'][0]['step']) == 4.0
