"""CPU: the host side of fine-tuning on still images -- vj_slice_sum's argument checks, ops.slice_sum on a recorder in place
of the library, what the image fine-tuning eval refuses before it creates a folder, the opt-in's default, and the still branch of
engine.layers.encoder_backward on stubbed wrappers."""
import inspect
import os
import sys
from functools import partial
from types import SimpleNamespace

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests.test_ops_host import Recorder, b, gpu  # noqa: E402


def test_slice_sum_rejects_bad_arguments_before_any_launch():
    from jepa_amd.hip.lib import load_library
    lib = load_library()
    rc = lib.vj_slice_sum(None, None, 2, 16, 4, 60, None)
    assert rc < 0 and b"vj_slice_sum" in lib.vj_last_error() and b"multiple of 8" in lib.vj_last_error()
    for dims in ((2, -1, 4, 64), (-2, 16, 4, 64), (2, 16, -4, 64), (2, 16, 4, 0)):
        rc = lib.vj_slice_sum(None, None, *dims, None)
        assert rc < 0 and b"bad dims" in lib.vj_last_error(), dims
    for dims in ((0, 16, 4, 64), (2, 0, 4, 64), (2, 16, 0, 64)):             # an empty problem launches nothing
        assert lib.vj_slice_sum(None, None, *dims, None) == 0, dims
    rc = lib.vj_slice_sum(None, None, 2, 16, 4, 64, None)
    assert rc < 0 and b"null pointer" in lib.vj_last_error()
    rc = lib.vj_slice_sum(2 ** 20, 2 ** 20, 2, 16, 4, 64, None)
    assert rc < 0 and b"must differ" in lib.vj_last_error()
    rc = lib.vj_slice_sum(2 ** 20, 2 ** 21 + 8, 2, 16, 4, 64, None)
    assert rc < 0 and b"16-byte aligned" in lib.vj_last_error()
    rc = lib.vj_slice_sum(2 ** 20, 2 ** 21, 2 ** 40, 2 ** 20, 4, 64, None)
    assert rc < 0 and b"overflows" in lib.vj_last_error()


@pytest.fixture
def rec(monkeypatch):
    from jepa_amd.hip import lib as L
    from jepa_amd.hip import ops
    r = Recorder()
    monkeypatch.setattr(ops, "load_library", lambda: r)
    monkeypatch.setattr(L, "load_library", lambda: r)
    monkeypatch.setattr(ops, "_device", lambda: 0)
    monkeypatch.setattr(ops, "_raw_stream", lambda dev: 0)
    return r


def test_wrapper_refuses_host_tensors_and_mismatched_shapes(rec):
    from jepa_amd.hip import ops
    with pytest.raises(ValueError, match="GPU"):
        ops.slice_sum(b(2 * 4 * 3, 8), 2, 3, 4)
    with pytest.raises(ValueError, match="GPU"):
        ops.slice_sum(gpu(b(2 * 4 * 3, 8)), 2, 3, 4, out=b(6, 8))
    assert rec.launches() == []
    with pytest.raises(ValueError, match="do not match B=2 S=3 Gt=5"):
        ops.slice_sum(gpu(b(2 * 4 * 3, 8)), 2, 3, 5)
    with pytest.raises(ValueError, match="do not match"):
        ops.slice_sum(gpu(b(2 * 4 * 3, 8)), 2, 3, 4, out=gpu(b(5, 8)))
    with pytest.raises(TypeError):
        ops.slice_sum(gpu(b(2 * 4 * 3, 8).float()), 2, 3, 4)
    with pytest.raises(ValueError, match="contiguous"):
        ops.slice_sum(gpu(b(2 * 4 * 3, 16))[:, :8], 2, 3, 4)
    assert rec.launches() == []
    dx, out = gpu(b(2 * 4 * 3, 8)), gpu(b(6, 8))
    assert ops.slice_sum(dx, 2, 3, 4, out=out) is out
    (name, args), = rec.calls
    assert name == "vj_slice_sum" and (args[0].value, args[1].value) == (dx.data_ptr(), out.data_ptr()) and args[2:6] == (2, 3, 4, 8)


# ---------------------------------------------------------------------------------------------------------------------- the eval
def _cfg(folder, **opt):
    return {
        'pretrain': {'model_name': 'vit_micro', 'checkpoint_key': 'target_encoder', 'patch_size': 16, 'folder': folder,
                     'checkpoint': 'micro-latest.pth.tar', 'write_tag': 'micro', 'tubelet_size': 2, 'frames_per_clip': 8,
                     'uniform_power': True},
        'data': {'dataset_name': 'synthetic', 'num_classes': 4, 'root_path': None, 'image_folder': None, 'resolution': 64,
                 'synthetic_length': 4},
        'optimization': dict({'batch_size': 2, 'num_epochs': 1, 'weight_decay': 0.01, 'start_lr': 0.002, 'lr': 0.01, 'final_lr': 0.0,
                              'warmup': 0.0, 'use_bfloat16': False}, **opt),
        'tag': 'ft',
    }


def test_main_refuses_the_image_encoder_and_a_probe_bank_before_creating_a_folder(tmp_path):
    from jepa_amd.evals.image_classification_finetune.eval import FOLDER_NAME, main
    assert FOLDER_NAME == 'image_classification_finetune/'
    cfg = _cfg(str(tmp_path))
    cfg['pretrain']['frames_per_clip'] = 1
    with pytest.raises(NotImplementedError, match="frames_per_clip == 1"):
        main(cfg)
    del cfg['pretrain']['frames_per_clip']            # the reference's default is 1
    with pytest.raises(NotImplementedError, match="frames_per_clip == 1"):
        main(cfg)
    with pytest.raises(ValueError, match="multihead_kwargs"):
        main(_cfg(str(tmp_path), multihead_kwargs=[{'lr': 0.01}, {'lr': 0.001}]))
    with pytest.raises(ValueError, match="unknown keys"):
        main(_cfg(str(tmp_path), finetune={'encoder_learning_rate': 1.0}))
    with pytest.raises(ValueError, match="mix: unknown keys"):
        main(_cfg(str(tmp_path), finetune={'mix': {'alpha': 1.0}}))
    assert not os.listdir(tmp_path)


def test_the_finetune_section_and_mechanics_are_the_video_evals():
    from jepa_amd.evals.image_classification_finetune import eval as IFT
    from jepa_amd.evals.video_classification_finetune import eval as VFT
    assert issubclass(IFT._ImageFineTune, VFT._FineTune)
    assert IFT._ImageFineTune.check is VFT._FineTune.check and IFT._ImageFineTune.attach is VFT._FineTune.attach
    assert IFT._ImageFineTune.folder_name != VFT._FineTune.folder_name
    for name in ("parse_finetune", "parse_mix", "EncoderFineTuner", "MixDraw"):
        assert name not in inspect.getsource(IFT).split('"""', 2)[2], name        # nothing of the mechanics is restated


def test_frozen_image_eval_keeps_its_defaults():
    from jepa_amd.evals.image_classification_frozen import eval as E
    sig = inspect.signature(E.run_one_epoch)
    for name, default in (("features_grad", False), ("after_update", None), ("mix", None)):
        p = sig.parameters[name]
        assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default is default
    assert inspect.signature(E.main).parameters["finetune"].default is None


def test_trainable_features_refuse_a_second_encoder_call(monkeypatch):
    from jepa_amd.evals.image_classification_frozen import eval as E
    calls = []
    enc = SimpleNamespace(patch_size=16, tubelet_size=2, num_frames=8, is_video=True, embed_dim=64, blocks=None)
    monkeypatch.setattr(E, "max_clips_per_call", lambda width, tokens: calls.append((width, tokens)) or 3)
    with pytest.raises(ValueError, match="max_clips_per_call = 3"):
        E.trainable_features(enc, torch.zeros(4, 3, 64, 64))
    assert calls == [(256, 4 * 16)]


# -------------------------------------------------------------------------------------------------------------------- the model
def _micro(**kw):
    from jepa_amd.src.models.vision_transformer import VisionTransformer
    args = dict(img_size=64, patch_size=16, num_frames=8, tubelet_size=2, embed_dim=64, depth=2, num_heads=2, mlp_ratio=4,
                qkv_bias=True, norm_layer=partial(torch.nn.LayerNorm, eps=1e-6), uniform_power=True)
    return VisionTransformer(**dict(args, **kw))


def test_opt_in_is_off_by_default_and_never_reaches_the_image_model():
    enc = _micro()
    assert enc.any_input_trains is False and "any_input_trains" not in enc.state_dict()
    for x in (torch.zeros(1, 3, 64, 64), torch.zeros(1, 3, 8, 96, 96)):
        with pytest.raises(NotImplementedError, match="frozen"):
            enc(x)
    assert enc.train_on_any_input() is enc and enc.any_input_trains is True
    assert enc.train_on_any_input(False).any_input_trains is False
    img = _micro(img_size=32, num_frames=1)
    img.train_on_any_input()
    with pytest.raises(NotImplementedError, match="frozen"):
        img(torch.zeros(1, 3, 32, 32))


# ------------------------------------------------------------------------------------------------------------------- the engine
def test_still_branch_of_encoder_backward(monkeypatch):
    """A saved still forward (fan-out (B, cells, gt)): exactly one slice_sum, on the trunk's input gradient, and the patch embedding's
    backward sees its B*cells rows; without the fan-out (clips, masked still images) no slice_sum and the gradient's own rows."""
    from jepa_amd.engine import layers
    B, cells, gt, D, kdim = 2, 16, 4, 64, 1536
    calls = []

    def slice_sum(dx, b_, s_, g_, out=None, stream=None):
        calls.append(("slice_sum", tuple(dx.shape), (b_, s_, g_)))
        return torch.zeros(b_ * s_, dx.shape[1], dtype=dx.dtype)

    def linear_backward(dy, x_in, lw, alpha, need_dx=True, beta=0.0, **kw):
        calls.append(("patch", tuple(dy.shape), tuple(x_in.shape), lw, need_dx, beta))

    monkeypatch.setattr(layers, "ops", SimpleNamespace(layernorm_bwd=lambda dout, *a, **kw: dout, slice_sum=slice_sum))
    monkeypatch.setattr(layers, "_tn_ok", lambda n, k: False)
    monkeypatch.setattr(layers, "_trunk_backward", lambda dx, *a, **kw: dx)
    monkeypatch.setattr(layers, "_linear_backward", linear_backward)
    monkeypatch.setattr(layers, "side_stream", lambda dev: SimpleNamespace(join=lambda: None))
    norm = SimpleNamespace(g=None, b=None, gg=None, gb=None)
    ew = SimpleNamespace(norm=norm, blocks=[SimpleNamespace(fc2=SimpleNamespace(gb=None))], patch="patch-embed")
    dout = torch.zeros(B * gt * cells, D, dtype=torch.bfloat16)
    tok = torch.zeros(B * cells, kdim, dtype=torch.bfloat16)
    saved = layers.EncoderSaved(tok=tok, blocks=[None], x=dout, mean=None, rstd=None, drop=None, fan=(B, cells, gt))
    layers.encoder_backward(dout, saved, ew, [layers.Seg(0, B, gt * cells)], alpha=1.0, beta=1.0)
    assert calls == [("slice_sum", (B * gt * cells, D), (B, cells, gt)),
                     ("patch", (B * cells, D), (B * cells, kdim), "patch-embed", False, 1.0)]
    del calls[:]
    tok = torch.zeros(B * gt * cells, kdim, dtype=torch.bfloat16)
    layers.encoder_backward(dout, saved._replace(tok=tok, fan=None), ew, [layers.Seg(0, B, gt * cells)], alpha=1.0)
    assert calls == [("patch", (B * gt * cells, D), (B * gt * cells, kdim), "patch-embed", False, 0.0)]
