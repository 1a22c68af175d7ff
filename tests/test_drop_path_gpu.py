"""GPU: stochastic depth of encoder fine-tuning, from the two row kernels up to the eval.

  - vj_drop_path_add / vj_drop_path_scale bit for bit against float64 expressions whose exactness is checked on the CPU first;
  - the per-kernel block chain under an EncoderFineTuner against tests/drop_path_ref_util.py (the oracle's fp32 encoder with the two
    scales per block) under torch autograd: loss and every encoder gradient, with explicit scales and with drawn ones (block 0
    then keeps its fused residual adds and bias sums beside a scaled block 1);
  - exact consequences of a dropped branch (zero gradients of exactly its tensors: the fused bias-sum routes must be off for a
    scaled Linear), of a fully dropped sample, and of the feature being off;
  - the draws; main() of the fine-tuning eval with `drop_path`.

Gradient bound.  Measured worst rel-L2 over the encoder's tensors against the fp32 reference (MI355X): MEASURED_DROP below, explicit
scales and drawn scales; the asserted bound is twice the larger, under the cap of 7e-2 that the autograd-path tests share
(tests/test_finetune_gpu.py, tests/test_step_gpu.py::test_module_autograd_path_matches_oracle)."""
import os
import sys
from functools import partial

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests import drop_path_ref_util as R  # noqa: E402
from tests.golden_util import MICRO, load_micro, micro_weights, rel_l2  # noqa: E402
from tests.step_util import oracle_cfg  # noqa: E402
from tests.finetune_util import HEADS, _classifier, _clips, _eval_cfg  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16 = torch.bfloat16
DEPTH = MICRO["depth"]

# measured worst rel-L2 of an encoder parameter gradient against the fp32 CPU reference on MI355X: explicit scales
# (blocks.1.norm1.weight), drawn scales (blocks.0.norm1.weight); the loss was within 7.4e-5 and 9.1e-5 relative
MEASURED_DROP = (7.77e-3, 6.33e-3)
BOUND = min(2 * max(MEASURED_DROP), 7e-2)       # 1.55e-2


def _vit(**kw):
    from jepa_amd.src.models.vision_transformer import VisionTransformer
    c = MICRO
    return VisionTransformer(img_size=c["crop"], patch_size=c["patch"], num_frames=c["frames"], tubelet_size=c["tubelet"],
                             embed_dim=c["embed_dim"], depth=c["depth"], num_heads=c["heads"], mlp_ratio=4, qkv_bias=True,
                             norm_layer=partial(torch.nn.LayerNorm, eps=1e-6), uniform_power=True, **kw)


def _encoder(**kw):
    enc = _vit(**kw)
    enc.load_state_dict(micro_weights(load_micro())[0], strict=True)
    return enc.to(DEV)


def _inv(keep):
    """1 / keep as the fp32 value a draw produces."""
    return float(torch.tensor(1.0, dtype=torch.float32) / torch.tensor(keep, dtype=torch.float32))


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int16)


# ------------------------------------------------------------------------------------------------------------------ the kernels
def _scale_patterns(B):
    alt = [_inv(0.8) if b % 2 == 0 else 0.0 for b in range(B)]
    mixed = [_inv(0.7)] * B
    if B > 1:
        mixed[B - 1] = 0.0
    return {"kept": [1.0] * B, "dropped": [0.0] * B, "alternating": alt, "keep0.9": [_inv(0.9)] * B, "keep0.7": mixed}


def _int_mantissa(t, bits):
    """t (float64 tensor holding values of a `bits`-bit significand) = m * 2^e with integer m: (m int64, e int64)."""
    m, e = torch.frexp(t)
    mi = torch.ldexp(m, torch.full_like(e, bits)).to(torch.int64)
    assert torch.equal(torch.ldexp(mi.double(), e - bits), t)
    return mi, e.to(torch.int64) - bits


def _product_is_exact(s, v):
    """s fp32 (24-bit significand) times v bf16 (8 bits) has at most 32 significant bits, so the float64 product is the exact one:
    checked here in integer arithmetic for the drawn values.  Returns the float64 product."""
    sd, vd = s.double(), v.double()
    ms, es = _int_mantissa(sd, 24)
    mv, ev = _int_mantissa(vd, 8)
    p = sd * vd
    assert torch.equal(torch.ldexp((ms * mv).double(), (es + ev).to(torch.int32)), p)
    return p


def _sum_is_exact(a, b):
    """float64 a + b without a rounding error (Knuth's TwoSum error term is zero everywhere).  Returns the sum."""
    t = a + b
    bb = t - a
    err = (a - (t - bb)) + (b - bb)
    assert torch.count_nonzero(err) == 0
    return t


@pytest.mark.parametrize("B", [1, 5])
@pytest.mark.parametrize("S", [1, 3, 197])
@pytest.mark.parametrize("D", [8, 64, 1288])
def test_kernels_bit_for_bit(D, S, B):
    from jepa_amd.hip import ops
    g = torch.Generator().manual_seed(1000 * D + 10 * S + B)
    M = B * S
    x = torch.randn(M, D, generator=g).to(BF16)
    y = (0.5 * torch.randn(M, D, generator=g)).to(BF16)
    guard = torch.full((1, D), 1.5, dtype=BF16)
    for name, pat in _scale_patterns(B).items():
        s = torch.tensor(pat, dtype=torch.float32)
        rows = s.repeat_interleave(S)[:, None]                  # [M, 1]: the scale of every row
        dropped = (rows == 0).expand(M, D)
        # -- the references, and that they are what the kernels compute: exact float64 values, rounded to fp32 and then to bf16
        y0 = torch.where(dropped, torch.zeros_like(y), y)       # (dropped rows hold NaN on the device and are not part of the claim)
        p = _product_is_exact(rows.expand(M, D), y0)
        ref_add = _sum_is_exact(x.double(), p).float().to(BF16)
        ref_add = torch.where(dropped, x, ref_add)              # a dropped row: the bits of x
        assert torch.equal(_bits(ref_add), _bits((x.double() + rows.double() * y0.double()).float().to(BF16)))
        ref_scale = p.float().to(BF16)                          # a dropped row: +0 (0 * 0)
        assert torch.count_nonzero(_bits(ref_scale)[dropped]) == 0
        # -- the device buffers: NaN where the kernels must not read, a guard row behind the last one
        y_in = torch.where(dropped, torch.full_like(y, float("nan")), y)
        xb = torch.cat([x, guard]).to(DEV)
        yb = torch.cat([y_in, guard]).to(DEV)
        sd = s.to(DEV)
        out = ops.drop_path_add(xb[:M], yb[:M], sd, B, S)
        assert out.data_ptr() == yb.data_ptr()
        assert torch.equal(_bits(yb[:M]), _bits(ref_add)), (name, "add")
        assert torch.equal(_bits(xb), _bits(torch.cat([x, guard]))), (name, "add: x changed")
        assert torch.equal(_bits(yb[M:]), _bits(guard)), (name, "add: guard row")
        db = torch.cat([y_in, guard]).to(DEV)
        ob = torch.cat([torch.full_like(y, 7.0), guard]).to(DEV)
        ops.drop_path_scale(db[:M], sd, B, S, out=ob[:M])
        assert torch.equal(_bits(ob[:M]), _bits(ref_scale)), (name, "scale")
        assert torch.equal(_bits(db), _bits(torch.cat([y_in, guard]))), (name, "scale: dx changed")
        assert torch.equal(_bits(ob[M:]), _bits(guard)), (name, "scale: guard row")
        assert torch.equal(sd.cpu(), s)
    fresh = ops.drop_path_scale(db[:M], sd, B, S)               # out=None allocates
    assert torch.equal(_bits(fresh), _bits(ob[:M])) and fresh.data_ptr() != db.data_ptr()


def test_ops_check_their_arguments():
    from jepa_amd.hip import ops
    x = torch.zeros(6, 8, dtype=BF16, device=DEV)
    s = torch.ones(2, device=DEV)
    with pytest.raises(ValueError, match="do not match"):
        ops.drop_path_add(x, x.clone(), s, 3, 3)
    with pytest.raises(ValueError, match="do not match"):
        ops.drop_path_add(x, x.clone(), torch.ones(3, device=DEV), 2, 3)
    with pytest.raises(TypeError):
        ops.drop_path_scale(x.float(), s, 2, 3)
    with pytest.raises(TypeError):
        ops.drop_path_scale(x, s.double(), 2, 3)
    assert ops.drop_path_scale(x[:0], s[:0], 0, 3).shape == (0, 8)      # no rows: no launch


# ------------------------------------------------------------------------------------------------- block chain against the reference
@pytest.fixture(scope="module")
def setup():
    """One micro encoder under a tuner, one classifier, the fixture's weights for the reference."""
    from jepa_amd.engine.finetune import EncoderFineTuner
    enc_w = micro_weights(load_micro())[0]
    enc = _encoder()
    tuner = EncoderFineTuner(enc, layer_decay=0.75)
    return enc_w, enc, tuner, _classifier()


def _reference(enc_w, clf, clips, labels, scales):
    """(loss, encoder gradients) of CE(classifier(features)) on the CPU with the reference's scaled blocks."""
    from oracle import probe_oracle as po
    w = {k: v.clone().requires_grad_(k != "pos_embed") for k, v in enc_w.items()}
    cw = {n: p.detach().cpu().clone() for n, p in clf.named_parameters()}
    feats = R.encoder_forward(w, clips, oracle_cfg(MICRO, 2), scales.cpu())
    loss = F.cross_entropy(po.attentive_classifier(cw, feats, HEADS), labels)
    loss.backward()
    return float(loss.detach()), {k: v.grad for k, v in w.items() if v.grad is not None}


def _backward(enc, clf, clips, labels):
    clf.zero_grad(set_to_none=True)
    loss = F.cross_entropy(clf(enc(clips.to(DEV))), labels.to(DEV))
    loss.backward()
    return float(loss.detach())


def _against_reference(setup, scales, what):
    """scales: explicit fp32 [L, 2, 4], or None: drawn at rate 0.5 under a seeded generator."""
    enc_w, enc, tuner, clf = setup
    clips = torch.cat(_clips(2), dim=0)          # B = 4
    labels = torch.tensor([3, 7, 1, 8])
    enc.train()
    if scales is not None:
        enc.set_drop_path_scales(scales.to(DEV))
    loss = _backward(enc, clf, clips, labels)
    used = enc.last_drop_path_scales
    assert used is not None and used.shape == (DEPTH, 2, 4)
    if scales is not None:
        assert torch.equal(used.cpu(), scales)
    ref_loss, ref = _reference(enc_w, clf, clips, labels, used)
    errs = {n: rel_l2(tuner.arena.grad(n).float().cpu(), g) for n, g in ref.items()}
    assert set(errs) == set(tuner.arena.slots)
    worst = max((e, n) for n, e in errs.items())
    print(f"{what}: loss {loss:.6f} reference {ref_loss:.6f} rel {abs(loss - ref_loss) / abs(ref_loss):.2e}; worst encoder "
          f"gradient rel-L2 {worst}")
    assert abs(loss - ref_loss) < 1e-3 * abs(ref_loss), (loss, ref_loss)
    assert worst[0] < BOUND, worst
    return used


def test_explicit_scales_against_the_reference(setup):
    a, b = _inv(0.9), _inv(0.8)
    scales = torch.tensor([[[1.0, 0.0, a, a], [0.0, a, 1.0, a]],        # block 0: attention, MLP
                           [[b, b, 0.0, b], [b, 0.0, b, 0.0]]])         # block 1
    assert all(0 < int((scales[i, j] == 0).sum()) < 4 for i in range(DEPTH) for j in range(2))     # kept and dropped everywhere
    _against_reference(setup, scales, "explicit scales")
    assert setup[1].__dict__["_drop_scales_next"] is None          # used once


def test_drawn_scales_against_the_reference(setup):
    """Rate 0.5 on depth 2: block 0 has rate 0, no scale, and keeps its fused residual adds and bias sums while block 1 is scaled."""
    enc = setup[1]
    enc.set_drop_path_rate(0.5)
    enc.drop_path_generator = torch.Generator(device=DEV).manual_seed(11)
    try:
        used = _against_reference(setup, None, "drawn scales").cpu()
    finally:
        enc.set_drop_path_rate(0.0)
        enc.drop_path_generator = None
    assert torch.equal(used[0], torch.ones(2, 4))
    assert 0 < int((used[1] == 0).sum()) < 8, used             # the seed gives kept and dropped samples in block 1


# ------------------------------------------------------------------------------------------------------------- exact consequences
def _names(l, branch):
    lin = ("attn.qkv", "attn.proj") if branch == 0 else ("mlp.fc1", "mlp.fc2")
    return {f"blocks.{l}.{m}.{t}" for m in lin for t in ("weight", "bias")} | \
        {f"blocks.{l}.norm{branch + 1}.{t}" for t in ("weight", "bias")}


@pytest.mark.parametrize("branch", [0, 1], ids=["attention", "mlp"])
@pytest.mark.parametrize("l", list(range(DEPTH)))
def test_a_dropped_branch_has_exactly_zero_gradients(setup, l, branch):
    """B = 1 with one branch of block l dropped: the tensors of that branch (its two Linears and the LayerNorm in front of them)
    get exactly zero gradients -- the bias of its last Linear included, which a fused column sum of a LayerNorm backward's output
    (proj.gb from norm2's, fc2.gb from the next block's norm1's or, for the last block, the final norm's) would fill with the
    unscaled stream's sums -- and every other tensor a non-zero one."""
    _, enc, tuner, clf = setup
    scales = torch.full((DEPTH, 2, 1), _inv(0.9))
    scales[l, branch, 0] = 0.0
    enc.train()
    enc.set_drop_path_scales(scales.to(DEV))
    tuner.arena.G.fill_(1.0)                    # a gradient nobody writes shows as non-zero
    _backward(enc, clf, _clips(1)[0][:1], torch.tensor([3]))
    zero = _names(l, branch)
    assert zero <= set(tuner.arena.slots)
    for n in tuner.arena.slots:
        nz = int(torch.count_nonzero(tuner.arena.grad(n)))
        assert (nz == 0) == (n in zero), (n, nz)


def test_a_fully_dropped_sample_and_its_neighbour(setup):
    from jepa_amd.hip import ops
    _, enc, _, _ = setup
    clips = _clips(1)[0].to(DEV)                 # B = 2
    scales = torch.full((DEPTH, 2, 2), _inv(0.9))
    scales[:, :, 0] = 0.0
    scales = scales.to(DEV)
    enc.train()
    enc.set_drop_path_scales(scales)
    f = enc(clips)
    assert f.requires_grad and torch.equal(enc.last_drop_path_scales, scales)
    # sample 0: the final LayerNorm of its embedded tokens (patch embedding + position rows), bit for bit
    ew = enc._hip_views(train=True)
    N = MICRO["num_patches"]
    x0 = ops.gemm_nt(ops.tubelet_pack(clips, MICRO["tubelet"], MICRO["patch"]), ew.patch.w, bias=ew.patch.b)
    ops.add_pos(x0, ew.pos, 2, N)
    ln = ops.layernorm_fwd(x0, ew.norm.g, ew.norm.b, 1e-6, save_stats=False)[0].view(2, N, -1)
    assert torch.equal(_bits(f[0]), _bits(ln[0]))
    assert not torch.equal(_bits(f[1]), _bits(ln[1]))
    # sample 1: its features from a B = 1 run with its scales
    enc.set_drop_path_scales(scales[:, :, 1:2])
    f1 = enc(clips[1:2])
    assert torch.equal(_bits(f[1]), _bits(f1[0]))
    # and they are not the undropped features
    with torch.no_grad():
        assert not torch.equal(_bits(f[1]), _bits(enc(clips)[1]))


def test_scales_must_fit_the_batch(setup):
    _, enc, _, _ = setup
    enc.train()
    enc.set_drop_path_scales(torch.ones(DEPTH, 2, 3, device=DEV))
    try:
        with pytest.raises(ValueError, match="do not fit a batch of 2"):
            enc(_clips(1)[0].to(DEV))
    finally:
        enc.set_drop_path_scales(None)


# ------------------------------------------------------------------------------------------------------------- no change when off
def test_off_means_bit_identical():
    plain, zero, pos = _encoder(), _encoder(drop_path_rate=0.0), _encoder(drop_path_rate=0.3)
    clf = _classifier()
    clips, labels = _clips(1)[0].to(DEV), torch.tensor([3, 7])
    for m in (plain, zero, pos):
        assert m.training
    with torch.no_grad():
        base = plain(clips)
        assert torch.equal(_bits(zero(clips)), _bits(base)) and torch.equal(_bits(pos(clips)), _bits(base))
    assert pos.last_drop_path_scales is None
    # rate 0 with gradients: features and gradients are the plain model's
    _backward(plain, clf, clips, labels)
    _backward(zero, clf, clips, labels)
    assert zero.last_drop_path_scales is None
    grads = {n: p.grad for n, p in plain.named_parameters() if p.requires_grad}
    assert len(grads) > 20
    for n, p in zero.named_parameters():
        if p.requires_grad:
            assert torch.equal(p.grad, grads[n]), n
    assert torch.equal(_bits(zero(clips)), _bits(plain(clips)))
    # a positive rate in eval(): no drops with gradients recorded either
    pos.eval()
    f = pos(clips)
    assert f.requires_grad and pos.last_drop_path_scales is None and torch.equal(_bits(f), _bits(plain(clips)))
    _backward(pos, clf, clips, labels)
    for n, p in pos.named_parameters():
        if p.requires_grad:
            assert torch.equal(p.grad, grads[n]), n
    # and in training mode it does drop
    pos.train()
    torch.manual_seed(5)
    drew = []
    for _ in range(4):
        pos(clips)
        drew.append(pos.last_drop_path_scales)
    assert all(d is not None for d in drew) and any(bool((d == 0).any()) for d in drew)


# ------------------------------------------------------------------------------------------------------------------------ draws
def test_draws():
    enc = _encoder(drop_path_rate=0.5)           # depth 2: rates 0 and 0.5, keep 1 and 0.5
    assert enc.drop_path_rates == [0.0, 0.5]
    clips = _clips(1)[0].to(DEV)

    def draw(n):
        out = []
        for _ in range(n):
            enc(clips)
            out.append(enc.last_drop_path_scales.cpu())
        return torch.stack(out)                  # [n, L, 2, B]

    enc.drop_path_generator = torch.Generator(device=DEV).manual_seed(7)
    a = draw(6)
    assert a.dtype == torch.float32 and a.shape == (6, 2, 2, 2)
    assert torch.equal(a[:, 0], torch.ones(6, 2, 2))                        # block 0 is never dropped
    assert bool(((a[:, 1] == 0) | (a[:, 1] == 2.0)).all())                  # 0 or 1 / keep
    assert 0 < int((a[:, 1] == 0).sum()) < 24
    enc.drop_path_generator = torch.Generator(device=DEV).manual_seed(7)
    assert torch.equal(draw(6), a)
    # without a generator of its own: the default CUDA generator
    enc.drop_path_generator = None
    torch.manual_seed(21)
    b = draw(3)
    torch.manual_seed(21)
    assert torch.equal(draw(3), b)
    # another keep: rate 0.2 -> 1 / 0.8 in fp32
    enc.set_drop_path_rate(0.2)
    c = draw(4)
    assert bool(((c[:, 1] == 0) | (c[:, 1] == _inv(0.8))).all()) and torch.equal(c[:, 0], torch.ones(4, 2, 2))


# ------------------------------------------------------------------------------------------------------------------------ the eval
def test_main_with_drop_path(tmp_path, monkeypatch):
    from jepa_amd.evals.video_classification_finetune import eval as FT
    from jepa_amd.src.models import vision_transformer as vit
    enc_w = micro_weights(load_micro())[0]
    calls, models = [], []

    def record(module, args, out):
        s = module.last_drop_path_scales
        calls.append(dict(x=args[0].detach().clone(), out=out.detach().clone(), grad=torch.is_grad_enabled(),
                          training=module.training, scales=None if s is None else s.cpu()))

    def micro(**kw):
        m = _vit()
        m.register_forward_hook(record)
        models.append(m)
        return m

    monkeypatch.setattr(vit, "vit_micro", micro, raising=False)
    torch.save({'target_encoder': {'module.backbone.' + k: v for k, v in enc_w.items()}, 'epoch': 10},
               tmp_path / 'micro-latest.pth.tar')
    cfg = _eval_cfg(str(tmp_path))
    cfg['optimization']['num_epochs'] = 2
    cfg['optimization']['finetune']['drop_path'] = 0.2
    torch.manual_seed(0)
    rec = FT.main(cfg)
    # a finite loss in every training iteration
    assert len(rec['train_history']) == 2 and all(ls == ls and abs(ls) < float("inf") for _, ls in rec['train_history'])
    enc = models[-1]
    assert enc.drop_path_rates == pytest.approx([0.0, 0.2]) and enc.training
    # the encoder moved
    ck = torch.load(tmp_path / "video_classification_finetune" / "micro_ft" / "micro-latest.pth.tar", map_location="cpu",
                    weights_only=False)
    moved = [n for n, v in ck['encoder'].items() if not torch.equal(v, enc_w[n])]
    assert len(moved) == len(enc_w) - 1 and 'pos_embed' not in moved, moved
    # training forwards record a backward and drop in block 1 only; validation forwards drop nothing
    train = [c for c in calls if c['grad']]
    val = [c for c in calls if not c['grad']]
    assert len(train) == 2 and val
    for c in train:
        assert c['training'] and c['scales'] is not None and torch.equal(c['scales'][0], torch.ones_like(c['scales'][0]))
        assert bool(((c['scales'][1] == 0) | (c['scales'][1] == _inv(0.8))).all())
    # the last validation batch, seen after the last update: its features are a no_grad forward's, in either mode
    last = val[-1]
    assert last['scales'] is None
    with torch.no_grad():
        assert torch.equal(_bits(enc(last['x'])), _bits(last['out']))
        enc.eval()
        assert torch.equal(_bits(enc(last['x'])), _bits(last['out']))
