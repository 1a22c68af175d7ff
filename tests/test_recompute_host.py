"""CPU: activation recomputation in the per-kernel chain (jepa_amd.engine.layers), as launch traces.  With the recorder of
tests.layer_trace_util in place of the launch path, a forward + backward under `recompute="block"` must leave the plain chain's
launches with exactly one insertion per block -- the launches of layers.block_forward(save=True) on that block with its drop-path
plan entry, directly before the block's backward and after every launch of the block above -- and under `recompute="mlp"` the single
fc1 GEMM that writes u and g.  Off (None or "none") is the plain trace, element for element.  The refusals are pinned with their
wording."""
import os
import sys
from functools import partial

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests import layer_trace_util as T  # noqa: E402

DEPTH = 3
INPUTS = {      # name -> (input, masks, drop list), each a callable or None
    "clip": (T.clip, None, None),
    "still": (T.still, None, None),
    "clip, two masks": (T.clip, partial(T.masks, 5, 7), None),
    "clip, both scales on every block": (T.clip, None, lambda: [(T.scale(), T.scale()) for _ in range(DEPTH)]),
}
# a vj_gemm_bf16_nt entry: [name, A, lda, B, ldb, out, ldo, M, N, K, bias, residual, ldr, aux_in, aux_out, ldaux, epilogue, ...]
GEMM_N, GEMM_K, GEMM_AUX_IN, GEMM_AUX_OUT, GEMM_EPI = 8, 9, 13, 14, 16


def _trace(monkeypatch, name, recompute):
    """(launches, launches of the forward, [(first, end) launch index of block i's backward, i = 0..DEPTH-1], the traces of
    block_forward alone on every block) of one forward + backward of input `name`."""
    from jepa_amd.engine import layers
    x, m, drop = INPUTS[name]
    calls = T.install(monkeypatch)
    ew = T.encoder_views(depth=DEPTH)
    spans = {}
    inner = layers.block_backward

    def block_backward(dx2, saved, bw, *a, **kw):
        first = len(calls)
        out = inner(dx2, saved, bw, *a, **kw)
        spans[[id(b) for b in ew.blocks].index(id(bw))] = (first, len(calls))
        return out

    monkeypatch.setattr(layers, "block_backward", block_backward)
    drops = drop and drop()
    del calls[:]
    out, segs, saved = layers.encoder_forward(ew, x(), m and m(), save=True, drop=drops, recompute=recompute)
    n_fwd = len(calls)
    layers.encoder_backward(torch.zeros_like(out), saved, ew, segs, alpha=1.0)
    trace = list(calls)
    alone = []
    for i, bw in enumerate(ew.blocks):
        del calls[:]
        layers.block_forward(torch.zeros_like(out), bw, segs, ew.heads, True, drop=layers._UNSCALED if drops is None else drops[i])
        alone.append(list(calls))
    return trace, n_fwd, [spans[i] for i in range(DEPTH)], alone


def _insertions(plain, got):
    """Both traces cut as (forward, backward); the backward of `got` as the plain backward with one insertion in front of every block's
    backward: returns [insertion of block i], having checked everything else."""
    (p, p_fwd, p_spans, _), (g, g_fwd, g_spans, _) = plain, got
    assert g[:g_fwd] == p[:p_fwd] and g_fwd == p_fwd, T.first_difference(g[:g_fwd], p[:p_fwd])
    ins, rest, at = [None] * DEPTH, g[g_fwd:p_spans[DEPTH - 1][0]], p_spans[DEPTH - 1][0]    # (the final norm's backward comes first)
    assert at == g_fwd + 1
    for i in range(DEPTH - 1, -1, -1):
        first, end = g_spans[i]
        assert first >= at
        ins[i] = g[at:first]                # everything between the end of block i+1's backward and the first launch of block i's
        assert end - first == p_spans[i][1] - p_spans[i][0]
        rest += g[first:end]
        at = end
    rest += g[at:]
    assert rest == p[p_fwd:], T.first_difference(rest, p[p_fwd:])
    return ins


@pytest.mark.parametrize("name", sorted(INPUTS))
def test_block_mode_inserts_each_blocks_forward_before_its_backward(monkeypatch, name):
    with pytest.MonkeyPatch.context() as mp:
        plain = _trace(mp, name, None)
    got = _trace(monkeypatch, name, "block")
    ins = _insertions(plain, got)
    for i in range(DEPTH):
        assert ins[i] == got[3][i], (i, T.first_difference(ins[i], got[3][i]))
        assert len(ins[i]) >= 7             # two LayerNorms, four GEMMs, attention once per segment
    assert len(got[0]) == len(plain[0]) + sum(len(a) for a in got[3])
    if "scales" in name:                    # the recomputed forward took the plan's entry: the scaled residual adds are in it
        assert [c[0] for c in ins[0]].count("vj_drop_path_add") == 2
    else:
        assert "vj_drop_path_add" not in [c[0] for c in ins[0]]


@pytest.mark.parametrize("name", sorted(INPUTS))
def test_mlp_mode_inserts_one_fc1_gemm_before_each_blocks_backward(monkeypatch, name):
    with pytest.MonkeyPatch.context() as mp:
        plain = _trace(mp, name, None)
    got = _trace(monkeypatch, name, "mlp")
    ins = _insertions(plain, got)
    for i in range(DEPTH):
        assert len(ins[i]) == 1, ins[i]
        c = ins[i][0]
        assert c[0] == "vj_gemm_bf16_nt"
        assert (c[GEMM_N], c[GEMM_K]) == (256, 64)                      # fc1: [M, D] x [4D, D]^T
        assert c[GEMM_AUX_OUT] == "*" and c[GEMM_AUX_IN] is None
        assert c[GEMM_EPI] == 1                                          # ops.EPI_GELU
        # it is the forward's own fc1 launch
        assert c in got[3][i]
    from jepa_amd.hip import ops
    assert ops.EPI_GELU == 1


@pytest.mark.parametrize("name", sorted(INPUTS))
@pytest.mark.parametrize("off", [None, "none"])
def test_off_is_the_plain_trace(monkeypatch, name, off):
    from jepa_amd.engine import layers
    x, m, drop = INPUTS[name]

    def run(**kw):
        with pytest.MonkeyPatch.context() as mp:
            calls = T.install(mp)
            ew = T.encoder_views(depth=DEPTH)
            del calls[:]
            out, segs, saved = layers.encoder_forward(ew, x(), m and m(), save=True, drop=drop and drop(), **kw)
            layers.encoder_backward(torch.zeros_like(out), saved, ew, segs, alpha=1.0)
            return list(calls), saved
    plain, _ = run()
    got, saved = run(recompute=off)
    assert T.first_difference(got, plain) is None and len(plain) > 0
    assert saved.recompute is None


def test_the_golden_cases_are_the_plain_traces(monkeypatch):
    """The same inputs through tests.layer_trace_util's own cases: recompute=None is what the golden file pins."""
    import json
    with open(T.GOLDEN) as fh:
        golden = json.load(fh)
    with pytest.MonkeyPatch.context() as mp:
        trace = _trace(mp, "clip, both scales on every block", None)[0]
    assert json.loads(json.dumps(trace)) == golden["drop clip, both scales on every block"]


def test_what_the_forward_keeps(monkeypatch):
    from jepa_amd.engine import layers
    T.install(monkeypatch)
    ew = T.encoder_views(depth=DEPTH)
    kept = {}
    for mode in (None, "mlp", "block"):
        _, _, saved = layers.encoder_forward(ew, T.clip(), None, save=True, recompute=mode)
        assert saved.recompute == mode
        kept[mode] = [{f for f in sv._fields if getattr(sv, f) is not None} for sv in saved.blocks]
    every = set(layers.BlockSaved._fields)
    assert kept[None] == [every] * DEPTH
    assert kept["mlp"] == [every - {"u", "g"}] * DEPTH
    assert kept["block"] == [{"x"}] * DEPTH


# -------------------------------------------------------------------------------------------------------------------- refusals
def _refused(monkeypatch, match, **kw):
    from jepa_amd.engine import layers
    for c_chain in (True, False):
        with pytest.MonkeyPatch.context() as mp:
            calls = T.install(mp)
            mp.setattr(layers, "USE_C_CHAIN", c_chain)
            ew = T.encoder_views()
            del calls[:]
            with pytest.raises(ValueError, match=match):
                layers.encoder_forward(ew, T.clip(), None, **kw)
            assert calls == [], calls


@pytest.mark.parametrize("mode", ["mlp", "block"])
def test_a_mode_with_a_workspace_is_refused(monkeypatch, mode):
    _refused(monkeypatch, r"activation recomputation runs on the per-kernel block chain only: the C launch chains \(ws_tag\)",
             save=True, ws_tag="enc_save", recompute=mode)


@pytest.mark.parametrize("mode", ["mlp", "block"])
def test_a_mode_without_a_record_is_refused(monkeypatch, mode):
    _refused(monkeypatch, rf"recompute='{mode}' with save=False: a forward that keeps nothing has nothing to recompute",
             save=False, recompute=mode)


@pytest.mark.parametrize("mode", ["full", True, 1, 0, False, "Block", ""])
def test_an_unknown_mode_is_refused(monkeypatch, mode):
    _refused(monkeypatch, r"activation recomputation is one of 'none', 'mlp', 'block'", save=True, recompute=mode)


def test_the_trunk_walker_refuses_what_encoder_forward_refuses(monkeypatch):
    """_trunk_forward is the predictor's walker too: a mode that reached it with a workspace or without save must not be dropped."""
    from jepa_amd.engine import layers
    calls = T.install(monkeypatch)
    ew = T.encoder_views()
    x = torch.zeros(T.B * 64, 64, dtype=torch.bfloat16)
    segs = [layers.Seg(0, T.B, 64)]
    del calls[:]
    with pytest.raises(ValueError, match=r"per-kernel block chain only"):
        layers._trunk_forward(x, ew, segs, True, "enc_save", recompute="block")
    with pytest.raises(ValueError, match=r"goes with save=True"):
        layers._trunk_forward(x, ew, segs, False, None, recompute="mlp")
    assert calls == []


def test_parse_finetune_takes_the_three_words():
    from jepa_amd.evals.video_classification_finetune.eval import parse_finetune
    assert parse_finetune({"lr": 1e-3}).recompute == "none"
    assert parse_finetune({"lr": 1e-3, "finetune": {"recompute": None}}).recompute == "none"
    for mode in ("none", "mlp", "block"):
        assert parse_finetune({"lr": 1e-3, "finetune": {"recompute": mode}}).recompute == mode
    for bad in ("full", True, 1):
        with pytest.raises(ValueError, match=r"optimization.finetune.recompute=.*one of 'none', 'mlp', 'block'"):
            parse_finetune({"lr": 1e-3, "finetune": {"recompute": bad}})


def test_set_activation_recompute_validates_and_stays_out_of_the_state_dict():
    from jepa_amd.src.models.vision_transformer import VisionTransformer
    vt = VisionTransformer(img_size=32, patch_size=16, num_frames=4, tubelet_size=2, embed_dim=32, depth=1, num_heads=2,
                           norm_layer=partial(torch.nn.LayerNorm, eps=1e-6))
    assert vt.activation_recompute is None
    keys = set(vt.state_dict())
    for mode, stored in (("mlp", "mlp"), ("block", "block"), ("none", None), (None, None)):
        assert vt.set_activation_recompute(mode) is vt and vt.activation_recompute == stored
    for bad in ("full", True, 1):
        vt.set_activation_recompute("block")
        with pytest.raises(ValueError, match=r"set_activation_recompute: mode=.*one of 'none', 'mlp', 'block'"):
            vt.set_activation_recompute(bad)
        assert vt.activation_recompute == "block"        # a refused value changes nothing
    assert set(vt.state_dict()) == keys
