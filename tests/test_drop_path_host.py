"""CPU: the host side of stochastic depth -- the fp32 reference against the oracle it restates, the per-block rate schedule, the
`optimization.finetune.drop_path` key, the argument validation of vj_drop_path_add / vj_drop_path_scale (refused before any HIP
call: there is no GPU here), the shape checks of set_drop_path_scales and the refusal of the C launch chains."""
import ctypes
import os
import sys
from functools import partial
from types import SimpleNamespace

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests import drop_path_ref_util as R  # noqa: E402
from tests.golden_util import MICRO, load_micro, micro_weights, step_inputs  # noqa: E402
from tests.step_util import oracle_cfg  # noqa: E402


def _vit(depth=2, **kw):
    from jepa_amd.src.models.vision_transformer import VisionTransformer
    return VisionTransformer(img_size=64, patch_size=16, num_frames=8, tubelet_size=2, embed_dim=64, depth=depth, num_heads=2,
                             mlp_ratio=4, qkv_bias=True, norm_layer=partial(torch.nn.LayerNorm, eps=1e-6), uniform_power=True, **kw)


def test_reference_with_unit_scales_is_the_oracle_bit_for_bit():
    from oracle import vjepa_oracle as O
    z = load_micro()
    w = micro_weights(z)[0]
    cfg = oracle_cfg(MICRO, 2)
    for s in (0, 1):
        clips = step_inputs(z, s)[0]
        ones = torch.ones(MICRO["depth"], 2, clips.shape[0])
        assert torch.equal(R.encoder_forward(w, clips, cfg, ones), O.encoder_forward(w, clips, cfg, masks=None))
    # and the scales do what they say: a sample whose branches are all dropped is the final norm of its embedded tokens
    clips = step_inputs(z, 0)[0]
    sc = torch.ones(MICRO["depth"], 2, clips.shape[0])
    sc[:, :, 0] = 0.0
    out = R.encoder_forward(w, clips, cfg, sc)
    D = MICRO["embed_dim"]
    x0 = O.patchify(clips, 2, 16) @ w["patch_embed.proj.weight"].reshape(D, -1).t() + w["patch_embed.proj.bias"] + w["pos_embed"]
    assert torch.equal(out[0], torch.nn.functional.layer_norm(x0, (D,), w["norm.weight"], w["norm.bias"], 1e-6)[0])
    assert torch.equal(out[1], O.encoder_forward(w, clips, cfg, masks=None)[1])


@pytest.mark.parametrize("depth", [1, 2, 12])
def test_rate_schedule(depth):
    m = _vit(depth=depth, drop_path_rate=0.3)
    ref = torch.linspace(0, 0.3, depth).tolist() if depth > 1 else [0.0]
    assert len(m.drop_path_rates) == depth and m.drop_path_rate == 0.3
    assert m.drop_path_rates == pytest.approx(ref, abs=1e-7)
    assert m.drop_path_rates[0] == 0.0 and (depth == 1 or m.drop_path_rates[-1] == 0.3)
    m.set_drop_path_rate(0.0)
    assert m.drop_path_rates == [0.0] * depth
    assert _vit(depth=depth).drop_path_rates == [0.0] * depth          # the default


def test_rate_out_of_range_raises_and_the_factories_take_it():
    from jepa_amd.src.models import vision_transformer as vit
    for bad in (-0.1, 1.0, 1.5):
        with pytest.raises(ValueError, match="drop_path_rate"):
            _vit(drop_path_rate=bad)
    with torch.device("meta"):
        m = vit.vit_tiny(img_size=64, patch_size=16, num_frames=8, tubelet_size=2, drop_path_rate=0.22)
    assert m.drop_path_rates == pytest.approx(torch.linspace(0, 0.22, 12).tolist(), abs=1e-7)
    with pytest.raises(ValueError, match="drop_path_rate"):
        vit.vit_tiny(img_size=64, patch_size=16, num_frames=8, tubelet_size=2, drop_path_rate=1.0)


def test_config_key():
    from jepa_amd.evals.video_classification_finetune.eval import parse_finetune
    opt = {'lr': 0.01}
    assert parse_finetune(opt).drop_path == 0.0
    assert parse_finetune(dict(opt, finetune={'drop_path': 0.2})).drop_path == 0.2
    assert parse_finetune(dict(opt, finetune={'drop_path': 0.1, 'layer_decay': 0.65})).layer_decay == 0.65
    with pytest.raises(ValueError, match="unknown keys"):
        parse_finetune(dict(opt, finetune={'drop_path_rate': 0.2}))


@pytest.mark.parametrize("name", ["vj_drop_path_add", "vj_drop_path_scale"])
def test_entry_points_refuse_bad_arguments_on_the_host(name):
    from jepa_amd.hip import lib as L
    lib = L.load_library()
    fn = getattr(lib, name)
    # three distinct, aligned, non-null addresses of host memory: refused calls never reach a launch, so nothing reads them
    bufs = [(ctypes.c_char * 64)() for _ in range(3)]
    a, b, s = (ctypes.c_void_p((ctypes.addressof(t) + 15) // 16 * 16) for t in bufs)

    def refused(match, *args):
        rc = fn(*args, None)
        assert rc < 0, (match, rc)
        msg = lib.vj_last_error()
        assert name.encode() in msg and match in msg, msg

    refused(b"multiple of 8", a, b, s, 2, 3, 12)
    refused(b"multiple of 8", a, b, s, 2, 3, 4)
    refused(b"bad dims", a, b, s, 2, 3, 0)
    refused(b"bad dims", a, b, s, -1, 3, 8)
    refused(b"bad dims", a, b, s, 2, -3, 8)
    refused(b"bad dims", a, b, s, 2, 3, -8)
    refused(b"null pointer", None, b, s, 2, 3, 8)
    refused(b"null pointer", a, None, s, 2, 3, 8)
    refused(b"null pointer", a, b, None, 2, 3, 8)
    refused(b"distinct", a, a, s, 2, 3, 8)
    refused(b"aligned", ctypes.c_void_p(a.value + 2), b, s, 2, 3, 8)
    refused(b"overflows", a, b, s, 1 << 62, 4, 8)
    # no rows: success without a launch (there is no device here to launch on), whatever the pointers
    assert fn(None, None, None, 0, 3, 8, None) == 0
    assert fn(a, b, s, 5, 0, 8, None) == 0


def test_ops_refuse_cpu_tensors():
    from jepa_amd.hip import ops
    x = torch.zeros(6, 8, dtype=torch.bfloat16)
    s = torch.ones(2)
    with pytest.raises(ValueError, match="GPU"):
        ops.drop_path_add(x, x.clone(), s, 2, 3)
    with pytest.raises(ValueError, match="GPU"):
        ops.drop_path_scale(x, s, 2, 3)


def test_set_drop_path_scales_shape_errors():
    m = _vit(depth=2, drop_path_rate=0.1)
    m.set_drop_path_scales(torch.ones(2, 2, 4))        # accepted; the batch is checked by the forward that takes them
    m.set_drop_path_scales(None)
    for bad in (torch.ones(3, 2, 4), torch.ones(2, 1, 4), torch.ones(2, 2), torch.ones(2, 2, 4, 1),
                torch.ones(2, 2, 4, dtype=torch.float64), torch.ones(2, 2, 4, dtype=torch.bfloat16)):
        with pytest.raises(ValueError, match="set_drop_path_scales"):
            m.set_drop_path_scales(bad)


def test_the_c_launch_chains_refuse_a_drop_list():
    from jepa_amd.engine import layers
    s = torch.ones(3)
    views = SimpleNamespace(blocks=[None, None], heads=2)
    segs = [layers.Seg(0, 3, 4)]
    drop = [None, (s, s)]
    with pytest.raises(ValueError, match="C launch chains"):
        layers._trunk_forward(None, views, segs, True, "enc_save", drop=drop)
    # the list itself: one entry per block, fp32 [B] scales
    with pytest.raises(ValueError, match="scale entries"):
        layers._check_drop([(s, s)], 2, 3, None)
    with pytest.raises(ValueError, match="one per clip"):
        layers._check_drop([None, (s, torch.ones(4))], 2, 3, None)
    with pytest.raises(ValueError, match="one per clip"):
        layers._check_drop([None, (s.double(), s)], 2, 3, None)
    layers._check_drop(drop, 2, 3, None)
    layers._check_drop(None, 2, 3, "enc_save")      # no drops: the Trainer's call
    layers._check_drop([], 2, 3, "enc_save")
