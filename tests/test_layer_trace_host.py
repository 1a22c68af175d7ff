"""CPU: "same kernels, same order, same sizes" of the per-kernel chain (jepa_amd.engine.layers), as a test.  Every case of
tests.layer_trace_util runs the public entry points (encoder_forward / encoder_backward, predictor_forward / predictor_backward) on a
recorder in place of the launch path and must leave exactly the launches of tests/golden/layer_chain_trace.json: every symbol with its
integer and float arguments, in order.  The refusals those entry points make are pinned below with their wording, and each must come
before anything is launched."""
import json
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests import layer_trace_util as T  # noqa: E402


@pytest.fixture(scope="module")
def golden():
    with open(T.GOLDEN) as fh:
        return json.load(fh)


def test_the_fixture_holds_exactly_the_cases(golden):
    assert sorted(golden) == sorted(T.CASES)


@pytest.mark.parametrize("case", sorted(T.CASES))
def test_chain_launches_what_it_launched(monkeypatch, golden, case):
    got, want = T.run_case(monkeypatch, case), golden[case]
    diff = T.first_difference(got, want)
    if diff is not None:
        i, g, w = diff
        print(f"case {case!r}: {len(got)} launches, {len(want)} expected; first difference at index {i}\n  got      {g}\n  expected {w}")
    assert diff is None, f"{case}: launch {diff[0]} is {diff[1]}, expected {diff[2]}"


def test_the_traces_are_not_trivially_equal(golden):
    """The cases differ where the chain differs: a still image embeds fewer rows and sums its slices, a scaled MLP branch costs its
    LayerNorm backward the fused bias gradient, and the options change the weight-gradient route."""
    names = lambda case: [c[0] for c in golden[case]]                                           # noqa: E731
    assert "vj_slice_sum" in names("encoder still") and "vj_slice_sum" not in names("encoder clip")
    assert "vj_add_pos_bcast" in names("encoder still") and "vj_add_pos_bcast" not in names("encoder still, two masks")
    # dxsum of every LayerNorm backward, from the final norm down to block 0's norm1: the bias gradient it also writes, or NULL
    dxsum = lambda case: [c[10] for c in golden[case] if c[0] == "vj_layernorm_bwd_colsum"]     # noqa: E731
    assert dxsum("encoder clip") == ["*"] * 4 + [None]
    assert dxsum("drop clip, mlp scale on the last block") == [None] + ["*"] * 5 + [None]
    assert dxsum("drop clip, mlp scale on the middle block") == ["*", "*", None, "*", "*", "*", None]
    assert dxsum("drop clip, attention scale on the middle block") == ["*", "*", "*", None, "*", "*", None]
    assert dxsum("encoder clip, wgrad_tn=0") == [None] * 5
    assert "vj_gemm_bf16_tn_grouped" in names("encoder clip") and "vj_gemm_bf16_tn_grouped" not in names("encoder clip, wgrad_group=0")
    assert "vj_transpose_bf16" in names("encoder clip, wgrad_tn=0") and "vj_transpose_bf16" not in names("encoder clip")
    assert "vj_gemm_bf16_nt_lnfold" in names("frozen clip, folded norms")


# -------------------------------------------------------------------------------------------------------------------- refusals
def _refused(monkeypatch, match, views, x, masks=None, c_chain=True, **kw):
    from jepa_amd.engine import layers
    calls = T.install(monkeypatch)
    monkeypatch.setattr(layers, "USE_C_CHAIN", c_chain)
    ew = views()
    del calls[:]
    with pytest.raises(ValueError, match=match):
        layers.encoder_forward(ew, x, masks, **kw)
    assert calls == [], calls


def test_a_position_table_that_does_not_fit_is_refused(monkeypatch):
    _refused(monkeypatch, r"position table of 64 rows does not fit the input's token grid 4x6x6", T.encoder_views, T.clip(96), save=True)
    _refused(monkeypatch, r"position table of 64 rows does not fit the input's token grid 2x4x4", T.encoder_views, T.clip(64, 4), save=False)
    _refused(monkeypatch, r"position table of 64 rows does not fit images of 36 cells", T.encoder_views, T.still(96), save=True)
    _refused(monkeypatch, r"position table of 64 rows does not fit images of 0 cells", T.encoder_views, T.still(8), save=False)
    _refused(monkeypatch, r"position table of 4 rows does not fit images of 4x4 cells", T.image_views, T.still(64), save=False)
    _refused(monkeypatch, r"position table of 4 rows does not fit images of 4x4 cells", T.image_views, [T.clip(64, 3), T.clip(64, 2)],
             save=False)


def test_masks_with_frames_are_refused(monkeypatch):
    for x in (T.clip(32, 3), [T.clip(32, 3), T.clip(32, 2)], [T.still(32), T.still(32)]):
        _refused(monkeypatch, r"masks address one image's token grid; frames \[B,C,T,H,W\] take none", T.image_views, x, T.masks(3),
                 save=False)


def test_the_image_model_saves_nothing_and_drops_nothing(monkeypatch):
    _refused(monkeypatch, r"the image model is a frozen \(save=False\) path", T.image_views, T.still(32), save=True)
    drop = [(T.scale(), None), None]
    _refused(monkeypatch, r"stochastic depth goes with a video encoder's clips \[B,3,T,H,W\] or still images \[B,3,H,W\]", T.image_views,
             T.still(32), save=False, drop=drop)
    # (the drop list is looked at before save is)
    _refused(monkeypatch, r"stochastic depth goes with a video encoder's clips", T.image_views, T.still(32), save=True, drop=drop)


def test_a_drop_list_must_fit_the_blocks_and_the_batch(monkeypatch):
    s = T.scale()
    _refused(monkeypatch, r"stochastic depth: 3 scale entries for 2 blocks", T.encoder_views, T.clip(), save=True, drop=[None, (s, s), None])
    _refused(monkeypatch, r"stochastic depth: 1 scale entries for 2 blocks", T.encoder_views, T.still(), save=True, drop=[(s, None)])
    _refused(monkeypatch, r"a scale is torch.float64 \(2,\), expected float32 \(2,\): one per clip", T.encoder_views, T.clip(), save=True,
             drop=[None, (s.double(), s)])
    _refused(monkeypatch, r"a scale is torch.float32 \(3,\), expected float32 \(2,\): one per clip", T.encoder_views, T.still(), save=True,
             drop=[(None, torch.ones(3)), None])
    _refused(monkeypatch, r"a scale is torch.float32 \(2, 1\), expected float32 \(2,\): one per clip", T.encoder_views, T.clip(), save=True,
             drop=[(torch.ones(2, 1), None), None])
    # the list is looked at before the input's grid is
    _refused(monkeypatch, r"scale entries", T.encoder_views, T.clip(96), save=True, drop=[(s, s)])


def test_a_drop_list_with_a_workspace_is_refused(monkeypatch):
    from jepa_amd.engine import layers
    s = T.scale()
    for c_chain in (True, False):       # whichever chain the workspace's owner would take
        _refused(monkeypatch, r"stochastic depth runs on the per-kernel block chain only: the C launch chains \(ws_tag\)", T.encoder_views,
                 T.clip(), save=True, ws_tag="enc_save", drop=[None, (s, s)], c_chain=c_chain)
    # an empty list is no list: the chain of a clip without one
    calls = T.install(monkeypatch)
    ew = T.encoder_views()
    del calls[:]
    layers.encoder_forward(ew, T.clip(), None, save=True, drop=[])
    with open(T.GOLDEN) as fh:
        want = json.load(fh)["encoder clip"]
    assert calls == want[:len(calls)] and len(calls) > 0
