"""A CPU trace of the per-kernel chain of jepa_amd.engine.layers: with the launch path of jepa_amd.hip.ops replaced by a recorder, the
encoder's and the predictor's forward and backward run end to end on zero tensors, with no library and no GPU, and leave the list of
launches they would have made -- every symbol with its integer and float arguments in order, a pointer as "*" (None when it is NULL,
which is how an optional operand such as layernorm_bwd's dxsum shows) and the problem table of the grouped weight-gradient launch
written out.  The trace says which kernels run in which order on which sizes; it does not say which buffer goes where.

`CASES` names every traced call; `run_case(monkeypatch, name)` returns its trace.  Everything is patched through the monkeypatch it is
given, nothing global.  Run as a script, this module writes tests/golden/layer_chain_trace.json from the tree it is run in:

    python tests/layer_trace_util.py
"""
import ctypes
import dataclasses
import json
import os
import sys
from functools import partial
from types import SimpleNamespace

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "layer_chain_trace.json")
DEFAULTS = {"wgrad_tn": 1, "wgrad_group": 1, "attn_softmax": 2}
CPU = torch.device("cpu")
B = 2


def _scalar(a):
    if a is None or isinstance(a, (bool, int, float, str, list)):
        return a
    if isinstance(a, ctypes.Array):         # a vj_seg_t array
        return [[getattr(e, n) for n, _ in e._fields_] for e in a]
    raise TypeError(f"launch argument {a!r} is neither a scalar nor a pointer")


def install(monkeypatch, options=None):
    """Put the recorder in place of ops' launch path and the stubs in place of what engine.layers asks the library and the streams;
    returns the list the launches are appended to."""
    from jepa_amd.engine import layers
    from jepa_amd.hip import ops
    calls = []
    opts = dict(DEFAULTS, **(options or {}))

    def launch(name, *args, stream=None, timer=None):
        args = list(args)
        if name == "vj_gemm_bf16_tn_grouped":       # (address of an int64 table of 8 entries per problem, problems, ...)
            args[0] = list((ctypes.c_int64 * (8 * args[1])).from_address(args[0]))
        calls.append([name] + [_scalar(a) for a in args])
        return 0

    def dev(t, dtype, name):
        if t.dtype != dtype:
            raise TypeError(f"{name}: expected {dtype}, got {t.dtype}")
        return t

    monkeypatch.setattr(ops, "_launch", launch)
    monkeypatch.setattr(ops, "_ptr", lambda t: None if t is None else "*")
    monkeypatch.setattr(ops, "_addr", lambda t, name: 0)
    monkeypatch.setattr(ops, "_dev", dev)
    monkeypatch.setattr(ops, "_device", lambda: 0)
    monkeypatch.setattr(ops, "_raw_stream", lambda d: 0)
    monkeypatch.setattr(ops, "_query", lambda name, *args: 64)
    monkeypatch.setattr(ops.Scratch, "_bufs", {})
    monkeypatch.setattr(layers, "get_option", opts.__getitem__)
    monkeypatch.setattr(layers, "side_stream", lambda device: SimpleNamespace(enabled=False, join=lambda: None))
    monkeypatch.setattr(layers, "USE_C_CHAIN", True)
    return calls


# ------------------------------------------------------------------------------------------------------------------- the models
def _views(module, views_fn, table, train):
    """The chain's views of a CPU module, as HipModule._hip_arena builds them on the GPU."""
    from jepa_amd.engine.weights import ParamArena
    weights = [(n, p) for n, p in module.named_parameters() if n != table]
    arena = ParamArena([weights], CPU, with_moments=False, bind_grads=False)
    if train:
        arena.make_transposed([n + ".weight" for n in module._hip_linear_names()])
    pos = getattr(module, table).data.to(torch.float32).reshape(module.num_patches, -1)
    return views_fn(arena, "", module, pos, train)


def encoder_views(depth=2, train=True, **kw):
    from jepa_amd.engine import weights
    from jepa_amd.src.models.vision_transformer import VisionTransformer
    args = dict(img_size=64, patch_size=16, num_frames=8, tubelet_size=2, embed_dim=64, depth=depth, num_heads=2, mlp_ratio=4,
                qkv_bias=True, norm_layer=partial(torch.nn.LayerNorm, eps=1e-6), uniform_power=True)
    return _views(VisionTransformer(**dict(args, **kw)), weights.encoder_views, "pos_embed", train)


def image_views():
    return encoder_views(train=False, img_size=32, num_frames=1)


def predictor_views():
    from jepa_amd.engine import weights
    from jepa_amd.src.models.predictor import VisionTransformerPredictor
    pred = VisionTransformerPredictor(img_size=64, patch_size=16, num_frames=8, tubelet_size=2, embed_dim=64, predictor_embed_dim=32,
                                      depth=2, num_heads=2, mlp_ratio=4, qkv_bias=True, norm_layer=partial(torch.nn.LayerNorm, eps=1e-6),
                                      uniform_power=True, use_mask_tokens=True, num_mask_tokens=2, zero_init_mask_tokens=True)
    return _views(pred, weights.predictor_views, "predictor_pos_embed", True)


def with_folds(ew):
    """ew with the LayerNorms of every block folded (engine.weights.FoldW), as the EMA target encoder carries them."""
    from jepa_amd.engine.weights import FoldW
    folds = []
    for bw in ew.blocks:
        (nq, d), nh = bw.qkv.w.shape, bw.fc1.w.shape[0]
        folds.append(FoldW(torch.zeros(nq, d, dtype=torch.bfloat16), torch.zeros(nq), torch.zeros(nq),
                           torch.zeros(nh, d, dtype=torch.bfloat16), torch.zeros(nh), torch.zeros(nh)))
    return dataclasses.replace(ew, folds=folds)


# ------------------------------------------------------------------------------------------------------------------- the inputs
def clip(size=64, frames=8, b=B):
    return torch.zeros(b, 3, frames, size, size)


def still(size=64, b=B):
    return torch.zeros(b, 3, size, size)


def masks(*lengths, b=B):
    return [torch.arange(k, dtype=torch.int64).repeat(b, 1) for k in lengths]


def scale(b=B):
    return torch.ones(b, dtype=torch.float32)


# -------------------------------------------------------------------------------------------------------------------- the cases
def _encoder(x, m=None, beta=0.0, depth=2, drop=None, pos=None):
    """Forward with save=True, then the backward of a zero gradient."""
    def run():
        from jepa_amd.engine import layers
        ew = encoder_views(depth=depth)
        yield
        out, segs, saved = layers.encoder_forward(ew, x(), m and m(), save=True, pos=pos and pos(), drop=drop and drop())
        layers.encoder_backward(torch.zeros_like(out), saved, ew, segs, alpha=1.0, beta=beta)
    return run


def _frozen(views, x, m=None, **kw):
    def run():
        from jepa_amd.engine import layers
        ew = views()
        yield
        layers.encoder_forward(ew, x(), m and m(), save=False, **kw)
    return run


def _predictor(beta):
    def run():
        from jepa_amd.engine import layers
        pw = predictor_views()
        yield
        enc_segs = layers.Seg.table(B, [5, 7])
        z = torch.zeros(B * 12, 64, dtype=torch.bfloat16)
        zhat, _, saved = layers.predictor_forward(pw, z, enc_segs, masks(5, 7), masks(3, 4), save=True)
        layers.predictor_backward(torch.zeros_like(zhat), saved, pw, enc_segs, alpha=1.0, beta=beta)
    return run


def _drops():
    s = scale
    return {
        "attention scale on the middle block": lambda: [None, (s(), None), None],
        "mlp scale on the middle block": lambda: [None, (None, s()), None],
        "mlp scale on the last block": lambda: [None, None, (None, s())],
        "both scales on every block": lambda: [(s(), s()) for _ in range(3)],
        "an entry that is None": lambda: [(s(), s()), None, (s(), s())],
    }


CASES = {       # name -> (generator function: set-up, yield, the traced calls; options)
    "encoder clip": (_encoder(clip), None),
    "encoder still": (_encoder(still), None),
    "encoder clip, two masks": (_encoder(clip, partial(masks, 5, 7)), None),
    "encoder still, two masks": (_encoder(still, partial(masks, 5, 7)), None),
    "encoder off-native clip": (_encoder(partial(clip, 96), pos=lambda: torch.zeros(4 * 6 * 6, 64)), None),
    "encoder clip, beta=1": (_encoder(clip, beta=1.0), None),
    "frozen clip, final_norm=False": (_frozen(encoder_views, clip, final_norm=False), None),
    "frozen clip, folded norms": (_frozen(lambda: with_folds(encoder_views()), clip), None),
    "frozen clip, folded norms, two masks": (_frozen(lambda: with_folds(encoder_views()), clip, partial(masks, 5, 7)), None),
    "image model, images": (_frozen(image_views, partial(still, 32)), None),
    "image model, one clip of frames": (_frozen(image_views, partial(clip, 32, 3)), None),
    "image model, two clips of frames": (_frozen(image_views, lambda: [clip(32, 3), clip(32, 2, b=1)]), None),
    "image model, images with a mask": (_frozen(image_views, partial(still, 32), partial(masks, 3)), None),
    "predictor, beta=0": (_predictor(0.0), None),
    "predictor, beta=1": (_predictor(1.0), None),
}
for _what, _drop in _drops().items():
    CASES[f"drop clip, {_what}"] = (_encoder(clip, depth=3, drop=_drop), None)
    CASES[f"drop still, {_what}"] = (_encoder(still, depth=3, drop=_drop), None)
for _opt in ("wgrad_tn", "wgrad_group", "attn_softmax"):
    CASES[f"encoder clip, {_opt}=0"] = (_encoder(clip), {_opt: 0})
    CASES[f"predictor, {_opt}=0"] = (_predictor(0.0), {_opt: 0})


def run_case(monkeypatch, name):
    """The trace of case `name`, as JSON gives it back (tuples are lists)."""
    run, options = CASES[name]
    calls = install(monkeypatch, options)
    steps = run()
    next(steps)             # set-up: building the arena launches its casts and transposes, which are not the chain's
    del calls[:]
    for _ in steps:
        pass
    return json.loads(json.dumps(calls))


def first_difference(got, want):
    """None when the traces agree, else (index, got entry or None, wanted entry or None) of the first place they do not."""
    for i in range(max(len(got), len(want))):
        g, w = (t[i] if i < len(t) else None for t in (got, want))
        if g != w:
            return i, g, w
    return None


if __name__ == "__main__":
    import pytest
    traces = {}
    for case in CASES:
        with pytest.MonkeyPatch.context() as mp:
            traces[case] = run_case(mp, case)
        print(f"{case}: {len(traces[case])} launches")
    with open(GOLDEN, "w") as fh:
        fh.write("{\n" + ",\n".join(f" {json.dumps(k)}: [\n  " + ",\n  ".join(json.dumps(c) for c in v) + "\n ]"
                                    for k, v in traces.items()) + "\n}\n")
    print("wrote", GOLDEN)
