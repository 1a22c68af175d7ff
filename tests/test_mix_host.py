"""CPU: the host side of mixup / cutmix / label smoothing -- the draws, the config section, the float64 references of
tests/mix_ref_util.py (against torch, and that their checkers reject planted errors) and the wrappers' refusal of CPU tensors."""
import os
import random
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests import mix_ref_util as R  # noqa: E402


def _draw(**kw):
    from jepa_amd.evals.mix import MixDraw
    args = dict(mixup_alpha=0.8, cutmix_alpha=1.0, prob=1.0, switch_prob=0.5, label_smoothing=0.1, num_classes=10, seed=3)
    args.update(kw)
    return MixDraw(**args)


def _same(p, q):
    return p.mixed == q.mixed and p.mode == q.mode and all(np.array_equal(getattr(p, k), getattr(q, k)) for k in ("lam", "box", "pixel_lam"))


# ------------------------------------------------------------------------------------------------------------------------- draws
def test_same_seed_same_plans_and_the_global_streams_stay():
    np.random.seed(11)
    random.seed(12)
    torch.manual_seed(13)
    before = (np.random.get_state()[1].copy(), random.getstate(), torch.get_rng_state().clone())
    a, b, c = _draw(), _draw(), _draw(seed=4)
    pa, pb, pc = [[d.draw(4, 224) for _ in range(32)] for d in (a, b, c)]
    assert all(_same(p, q) for p, q in zip(pa, pb))
    assert not all(_same(p, q) for p, q in zip(pa, pc))
    assert {p.mode for p in pa} == {"mixup", "cutmix"}
    assert np.array_equal(np.random.get_state()[1], before[0]) and random.getstate() == before[1]
    assert torch.equal(torch.get_rng_state(), before[2])
    for p in pa:
        assert p.lam.dtype == np.float32 and p.lam.shape == (4,) and p.box.dtype == np.int32 and p.box.shape == (4, 4)
        assert p.pixel_lam.dtype == np.float32 and (p.lam == p.lam[0]).all() and (p.box == p.box[0]).all()     # batch mode


def test_the_order_of_the_draws():
    """The plan is these draws of the MixDraw's own RandomState, in this order."""
    d = _draw(seed=21)
    rs = np.random.RandomState(21)
    for _ in range(40):
        p = d.draw(3, 64)
        assert rs.rand() < 1.0
        cutmix = rs.rand() < 0.5
        lam = rs.beta(1.0, 1.0) if cutmix else rs.beta(0.8, 0.8)
        if cutmix:
            cy, cx = rs.randint(64), rs.randint(64)
            cut = int(64 * np.sqrt(1.0 - lam))
            box = [max(cy - cut // 2, 0), min(cy + cut // 2, 64), max(cx - cut // 2, 0), min(cx + cut // 2, 64)]
            assert p.mode == "cutmix" and p.box[0].tolist() == box and (p.pixel_lam == 1).all()
        else:
            assert p.mode == "mixup" and (p.lam == np.float32(lam)).all() and (p.pixel_lam == np.float32(lam)).all()
            assert not p.box.any()
    # an unmixed batch consumes the first draw only
    d, rs = _draw(seed=22, prob=0.5), np.random.RandomState(22)
    mixed = []
    for _ in range(40):
        p = d.draw(2, 32)
        mixed.append(p.mixed)
        if rs.rand() < 0.5:
            c = rs.rand() < 0.5
            rs.beta(1.0, 1.0) if c else rs.beta(0.8, 0.8)
            if c:
                rs.randint(32), rs.randint(32)
            assert p.mixed
        else:
            assert not p.mixed and (p.lam == 1).all() and (p.pixel_lam == 1).all() and not p.box.any()
    assert 0 < sum(mixed) < 40
    assert d.rng.rand() == rs.rand()


@pytest.mark.parametrize("S", [7, 64, 224])
def test_cutmix_boxes_and_their_lam(S):
    d = _draw(mixup_alpha=0.0, seed=S)
    clipped = 0
    for _ in range(200):
        p = d.draw(2, S)
        assert p.mixed and p.mode == "cutmix"
        y0, y1, x0, x1 = (int(v) for v in p.box[0])
        assert 0 <= y0 <= y1 <= S and 0 <= x0 <= x1 <= S
        assert (p.lam == np.float32(1.0 - (y1 - y0) * (x1 - x0) / float(S * S))).all()        # exactly
        assert (p.pixel_lam == 1).all()
        clipped += (y1 - y0) != (x1 - x0)
    assert clipped > 0          # boxes cut by the border occur, and stayed inside


def test_prob_zero_never_mixes_and_one_alpha_fixes_the_mode():
    d = _draw(prob=0.0)
    assert not any(d.draw(4, 32).mixed for _ in range(100))
    assert {_draw(cutmix_alpha=0.0, seed=s).draw(4, 32).mode for s in range(30)} == {"mixup"}
    assert {_draw(mixup_alpha=0.0, seed=s).draw(4, 32).mode for s in range(30)} == {"cutmix"}
    # switch_prob at its ends fixes it too
    assert {_draw(switch_prob=0.0, seed=s).draw(4, 32).mode for s in range(30)} == {"mixup"}
    assert {_draw(switch_prob=1.0, seed=s).draw(4, 32).mode for s in range(30)} == {"cutmix"}
    # no alpha: smoothing only, and no draw is consumed
    d = _draw(mixup_alpha=0.0, cutmix_alpha=0.0)
    state = d.rng.get_state()[1].copy()
    assert not d.draw(4, 32).mixed and np.array_equal(d.rng.get_state()[1], state)
    for bad in (dict(mixup_alpha=-1.0), dict(prob=1.5), dict(switch_prob=-0.1), dict(label_smoothing=1.0), dict(num_classes=0)):
        with pytest.raises(ValueError):
            _draw(**bad)


# ------------------------------------------------------------------------------------------------------------------------ config
def test_parse_finetune_reads_and_validates_mix():
    from jepa_amd.evals.video_classification_finetune.eval import MIX_DEFAULTS, parse_finetune
    opt = {'lr': 0.01}
    assert parse_finetune(opt).mix is None
    assert parse_finetune(dict(opt, finetune={'drop_path': 0.1})).mix is None
    assert parse_finetune(dict(opt, finetune={'mix': None})).mix is None
    assert MIX_DEFAULTS == {'mixup_alpha': 0.8, 'cutmix_alpha': 1.0, 'prob': 1.0, 'switch_prob': 0.5, 'label_smoothing': 0.1, 'seed': 0}
    assert parse_finetune(dict(opt, finetune={'mix': {}})).mix == MIX_DEFAULTS
    got = parse_finetune(dict(opt, finetune={'mix': {'mixup_alpha': 0.0, 'seed': 5}, 'layer_decay': 0.65}))
    assert got.mix == dict(MIX_DEFAULTS, mixup_alpha=0.0, seed=5) and got.layer_decay == 0.65
    # all three knobs at 0: off
    assert parse_finetune(dict(opt, finetune={'mix': {'mixup_alpha': 0, 'cutmix_alpha': 0, 'label_smoothing': 0}})).mix is None
    assert parse_finetune(dict(opt, finetune={'mix': {'mixup_alpha': 0, 'cutmix_alpha': 0}})).mix is not None    # smoothing 0.1
    with pytest.raises(ValueError, match="unknown keys"):
        parse_finetune(dict(opt, finetune={'mix': {'mixup': 0.8}}))
    with pytest.raises(ValueError, match="unknown keys"):
        parse_finetune(dict(opt, finetune={'mixup': {}}))
    for bad in ({'mixup_alpha': -0.1}, {'cutmix_alpha': -1}, {'prob': 1.1}, {'prob': -0.1}, {'switch_prob': 2}, {'label_smoothing': 1.0},
                {'label_smoothing': -0.1}, {'mixup_alpha': 'high'}, {'seed': -1}, {'seed': 0.5}, {'prob': float('nan')}):
        with pytest.raises(ValueError, match="optimization.finetune.mix"):
            parse_finetune(dict(opt, finetune={'mix': bad}))
    with pytest.raises(ValueError, match="expected a mapping"):
        parse_finetune(dict(opt, finetune={'mix': True}))


def test_the_frozen_evals_do_not_read_the_key():
    import inspect

    from jepa_amd.evals import frozen
    from jepa_amd.evals.video_classification_frozen import eval as E
    assert "'mix'" not in inspect.getsource(frozen) and "'mix'" not in inspect.getsource(E.main)
    sig = inspect.signature(E.run_one_epoch)
    assert sig.parameters['mix'].kind is inspect.Parameter.KEYWORD_ONLY and sig.parameters['mix'].default is None


# -------------------------------------------------------------------------------------------------------------------- references
@pytest.mark.parametrize("C", [1, 10, 400])
def test_the_loss_reference_agrees_with_torch_in_float64(C):
    rng = np.random.RandomState(C)
    z = (3.0 * rng.randn(5, C)).astype(np.float32)
    a = rng.randint(C, size=5)
    b = rng.randint(C, size=5)
    lam = rng.rand(5).astype(np.float32)
    for eps in (0.0, 0.1):
        t = R.soft_target(a, b, lam, eps, C)
        assert np.allclose(t.sum(axis=1), 1.0, rtol=0, atol=1e-15)
        loss, dl, p = R.soft_ce_ref(z, a, b, lam, eps)
        zt = torch.tensor(z, dtype=torch.float64, requires_grad=True)
        want = F.cross_entropy(zt, torch.tensor(t), reduction='none')
        assert np.allclose(loss, want.detach().numpy(), rtol=1e-13, atol=1e-13)
        want.sum().backward()
        assert np.allclose(dl, zt.grad.numpy(), rtol=0, atol=1e-14)
        assert np.allclose(p, torch.softmax(zt.detach(), dim=1).numpy(), rtol=0, atol=1e-15)
    # eps = 0, lam = 1: the hard cross-entropy
    loss, _, _ = R.soft_ce_ref(z, a, b, np.ones(5, np.float32), 0.0)
    hard = F.cross_entropy(torch.tensor(z, dtype=torch.float64), torch.tensor(a), reduction='none')
    assert np.allclose(loss, hard.numpy(), rtol=1e-13, atol=1e-13)


@pytest.mark.parametrize("C", R.SOFT_CE_CLASSES)
def test_torch_fp32_soft_cross_entropy_stays_inside_the_cap(C):
    """The cap of 1e-5 on both bounds of vj_soft_ce (tests/test_mix_gpu.py) is one that torch's own fp32 log_softmax-based soft
    cross-entropy meets against float64 on the very inputs of the GPU test, C = 8142 with +-80 logits included: the inputs were
    not shrunk and the cap was not widened."""
    worst = [0.0, 0.0]
    for name, z, a, b, lam, eps in R.soft_ce_cases(C):
        ref = R.soft_ce_ref(z, a, b, lam, eps)
        zt = torch.tensor(z, requires_grad=True)
        t = torch.tensor(R.soft_target(a, b, lam, eps, C)).float()
        loss = torch.sum(-t * F.log_softmax(zt, dim=-1), dim=-1)
        loss.sum().backward()
        el, ed, _ = R.soft_ce_errors(loss.detach().numpy(), zt.grad.numpy(), None, ref)
        worst = [max(worst[0], el), max(worst[1], ed)]
        assert el <= R.SOFT_CE_CAP and ed <= R.SOFT_CE_CAP, (name, el, ed)
    print(f"C={C}: torch fp32 worst loss error {worst[0]:.3e} (rel. to max(1, |ref|)), worst dlogits error {worst[1]:.3e}")


def _soft_ce_outputs(C=65):
    name, z, a, b, lam, eps = [c for c in R.soft_ce_cases(C) if c[0] == "R=3 normal a!=b lam=0.25 eps=0.1"][0]
    ref = R.soft_ce_ref(z, a, b, lam, eps)
    return ref, [r.astype(np.float32) for r in ref]


def test_the_soft_ce_checker_rejects_planted_errors():
    ref, (loss, dl, p) = _soft_ce_outputs()
    R.check_soft_ce(loss, dl, p, ref, 1e-6, 1e-6)                     # the reference rounded to fp32 passes
    bad = dl.copy()
    bad[1, 17] += 1e-4
    with pytest.raises(AssertionError, match="dlogits off"):
        R.check_soft_ce(loss, bad, p, ref, R.SOFT_CE_CAP, R.SOFT_CE_CAP)
    bad = loss.copy()
    bad[2] *= 1.0 + 1e-4
    with pytest.raises(AssertionError, match="loss off"):
        R.check_soft_ce(bad, dl, p, ref, R.SOFT_CE_CAP, R.SOFT_CE_CAP)
    bad = p.copy()
    k = np.unravel_index(np.argmin(p), p.shape)
    assert p[k] < 5e-6                                                 # (so that the planted value stays inside the element bound)
    bad[k] = -1e-7
    with pytest.raises(AssertionError, match="negative probability"):
        R.check_soft_ce(loss, dl, bad, ref, R.SOFT_CE_CAP, R.SOFT_CE_CAP)
    bad = dl + np.float32(2e-7)                                        # inside the element bound, but the rows no longer sum to 0
    with pytest.raises(AssertionError, match="sum_c dlogits"):
        R.check_soft_ce(loss, bad, p, ref, R.SOFT_CE_CAP, R.SOFT_CE_CAP)


def _mixed(x, lam, box):
    """What the kernel may produce, made on the host: the reference rounded to fp32, own and partner bits where they belong."""
    ref, kind, _ = R.clip_mix_ref(x, lam, box)
    out = ref.astype(np.float32)
    out = np.where(kind == R.OWN, x, out)
    return np.where(kind == R.SWAPPED, x[::-1], out)


def test_the_clip_mix_checker_rejects_planted_errors():
    rng = np.random.RandomState(0)
    x = rng.randn(4, 2, 8, 12).astype(np.float32)
    x[0, 0, 0, 0] = -0.0
    box = np.tile(np.array([1, 7, 3, 9], np.int32), (4, 1))
    # cutmix: swapped inside, own outside
    lam = np.ones(4, np.float32)
    out = _mixed(x, lam, box)
    assert R.check_clip_mix(out, x, lam, box) == 0.0
    assert np.array_equal(out[0, :, 1:7, 3:9], x[3, :, 1:7, 3:9]) and np.array_equal(out[0, :, 0], x[0, :, 0])
    bad = out.copy()
    bad[1, 1, 4, 5] = x[1, 1, 4, 5]                                   # one pixel inside a box left unswapped
    with pytest.raises(AssertionError, match="own or take their partner's bits"):
        R.check_clip_mix(bad, x, lam, box)
    bad = out.copy()
    bad[0, 0, 0, 0] = 0.0                                              # the sign of a zero outside the box
    with pytest.raises(AssertionError, match="own or take their partner's bits"):
        R.check_clip_mix(bad, x, lam, box)
    # mixup with a box: blended outside
    lam = np.array([0.3, 0.3, 0.9, 0.3], np.float32)
    out = _mixed(x, lam, box)
    assert R.check_clip_mix(out, x, lam, box) <= 0.25                  # one rounding of the exact value: 2^-24 of 2^-22
    bad = out.copy()
    bad[2, 0, 0, 1] = np.float32(0.3) * x[2, 0, 0, 1] + np.float32(0.7) * x[1, 0, 0, 1]       # sample 2 blended with sample 1's lam
    with pytest.raises(AssertionError, match="blended element"):
        R.check_clip_mix(bad, x, lam, box)
    # odd B: the middle sample keeps its bits
    x3, lam3 = x[:3], np.full(3, 0.5, np.float32)
    out = _mixed(x3, lam3, box[:3])
    assert np.array_equal(out[1], x3[1])
    R.check_clip_mix(out, x3, lam3, box[:3])
    bad = out.copy()
    bad[1, 0, 0, 0] = 1.0
    with pytest.raises(AssertionError):
        R.check_clip_mix(bad, x3, lam3, box[:3])


# ---------------------------------------------------------------------------------------------------------------------- wrappers
def test_the_wrappers_refuse_cpu_tensors_and_bad_tables():
    from jepa_amd.hip import ops
    x = torch.zeros(2, 3, 8, 8)
    with pytest.raises(ValueError, match="must live on the GPU"):
        ops.clip_mix(x, torch.ones(2), torch.zeros(2, 4, dtype=torch.int32))
    with pytest.raises(ValueError, match="must live on the GPU"):
        ops.soft_ce(torch.zeros(2, 10), torch.zeros(2, dtype=torch.int32), torch.zeros(2, dtype=torch.int32), torch.ones(2), 0.1)
    with pytest.raises(TypeError):
        ops.clip_mix(x.double(), torch.ones(2), torch.zeros(2, 4, dtype=torch.int32))
    # the host tables are validated before anything is uploaded
    for box in ([[0, 9, 0, 8]], [[5, 4, 0, 8]], [[0, 8, -1, 8]], [[0, 8, 6, 5]], [[0, 8, 0, 12]]):
        with pytest.raises(ValueError, match="every box needs"):
            ops.mix_tables([1.0], box, 8, 8, "cpu")
    with pytest.raises(ValueError, match="expected"):
        ops.mix_tables([1.0, 1.0], [[0, 0, 0, 0]], 8, 8, "cpu")
    with pytest.raises(ValueError, match="finite"):
        ops.mix_tables([float("nan")], [[0, 0, 0, 0]], 8, 8, "cpu")
    for a, b in (([10], [0]), ([0], [-1]), ([3], [11])):
        with pytest.raises(ValueError, match="labels must lie"):
            ops.soft_ce_tables(a, b, [1.0], 10, "cpu")
    lam, box = ops.mix_tables([0.5, 0.5], [[0, 8, 0, 8]] * 2, 8, 8, "cpu")
    assert lam.dtype == torch.float32 and box.dtype == torch.int32 and box._vj_checked == (8, 8)
    a, b, lam = ops.soft_ce_tables([1, 2], [2, 1], [0.5, 0.5], 10, "cpu")
    assert a.dtype == torch.int32 and a._vj_checked == 10 and b._vj_checked == 10 and lam.dtype == torch.float32


def test_the_entry_points_check_their_arguments_on_the_host():
    """No GPU: every refusal comes before any HIP call (negative return code and a message naming the entry point)."""
    import ctypes

    from jepa_amd import build
    from jepa_amd.hip import lib as L
    build.build(verbose=False)
    lib = L.load_library()
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    off = ctypes.c_void_p(p.value + 4)

    def refused(rc, *words):
        msg = lib.vj_last_error()
        assert rc < 0 and all(w in msg for w in words), (rc, msg)

    refused(lib.vj_clip_mix(p, p, p, -1, 3, 8, 8, None), b"vj_clip_mix", b"bad dims")
    refused(lib.vj_clip_mix(p, p, p, 2, 3, 8, 6, None), b"vj_clip_mix", b"multiple of 4")
    refused(lib.vj_clip_mix(p, p, p, 2 ** 40, 2 ** 20, 2 ** 10, 2 ** 10, None), b"vj_clip_mix", b"overflows")
    refused(lib.vj_clip_mix(None, p, p, 2, 3, 8, 8, None), b"vj_clip_mix", b"null pointer")
    refused(lib.vj_clip_mix(p, None, p, 2, 3, 8, 8, None), b"vj_clip_mix", b"null pointer")
    refused(lib.vj_clip_mix(p, p, None, 2, 3, 8, 8, None), b"vj_clip_mix", b"null pointer")
    refused(lib.vj_clip_mix(off, p, p, 2, 3, 8, 8, None), b"vj_clip_mix", b"16-byte aligned")
    assert lib.vj_clip_mix(None, None, None, 0, 3, 8, 8, None) == 0          # nothing to do: no launch
    assert lib.vj_clip_mix(None, None, None, 4, 3, 0, 8, None) == 0
    refused(lib.vj_soft_ce(p, 10, p, p, p, 0.1, -1, 10, p, p, p, None), b"vj_soft_ce", b"bad dims")
    refused(lib.vj_soft_ce(p, 10, p, p, p, 0.1, 2, 0, p, p, p, None), b"vj_soft_ce", b"bad dims")
    refused(lib.vj_soft_ce(p, 9, p, p, p, 0.1, 2, 10, p, p, p, None), b"vj_soft_ce", b"row stride")
    refused(lib.vj_soft_ce(p, 10, p, p, p, 1.0, 2, 10, p, p, p, None), b"vj_soft_ce", b"smoothing")
    refused(lib.vj_soft_ce(p, 10, p, p, p, -0.5, 2, 10, p, p, p, None), b"vj_soft_ce", b"smoothing")
    for k in (0, 2, 3, 4, 8, 9):        # logits, label_a, label_b, lam, loss, dlogits; probs (10) may be null
        args = [p, 10, p, p, p, 0.1, 2, 10, p, p, None, None]
        args[k] = None
        refused(lib.vj_soft_ce(*args), b"vj_soft_ce", b"null pointer")
    assert lib.vj_soft_ce(None, 10, None, None, None, 0.1, 0, 10, None, None, None, None) == 0
