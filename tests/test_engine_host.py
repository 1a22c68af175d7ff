"""CPU: the host engine's shared pieces that need neither a GPU nor the library -- the segment-table builder against hand-written
tables, the one vj_seg_t array builder on Seg objects and on tuples, the stream log shared by engine.layers and engine.streams,
and the names that code outside the engine imports."""
import importlib

import pytest

# (B, lengths, the table written out by hand as (row0, B, S))
TABLES = [
    ("one mask", 4, [48], [(0, 4, 48)]),
    ("two masks of different lengths", 3, [40, 52], [(0, 3, 40), (120, 3, 52)]),
    ("a zero-length mask", 2, [5, 0, 7], [(0, 2, 5), (10, 2, 0), (10, 2, 7)]),
    ("B = 1", 1, [9, 4], [(0, 1, 9), (9, 1, 4)]),
]


@pytest.mark.parametrize("what,B,lengths,table", TABLES, ids=[t[0] for t in TABLES])
def test_segment_builder_against_hand_written_tables(what, B, lengths, table):
    from jepa_amd.engine.layers import Seg
    segs = Seg.table(B, lengths)
    assert segs == [Seg(*row) for row in table]
    assert [(s.row0, s.B, s.S, s.rows) for s in segs] == [(r, b, s, b * s) for r, b, s in table]


@pytest.mark.parametrize("what,B,lengths,table", TABLES, ids=[t[0] for t in TABLES])
def test_one_seg_array_builder_for_seg_objects_and_tuples(what, B, lengths, table):
    """ops._seg_array and chain.seg_array are one builder: byte-identical vj_seg_t arrays from Seg objects and from tuples."""
    import ctypes

    from jepa_amd.engine import chain
    from jepa_amd.engine.layers import Seg
    from jepa_amd.hip import ops
    from jepa_amd.hip.lib import VjSeg
    segs = Seg.table(B, lengths)
    want = b"".join(bytes(VjSeg(*row)) for row in table)
    assert len(want) == len(table) * ctypes.sizeof(VjSeg)
    for build in (ops._seg_array, chain.seg_array):
        assert bytes(build(segs)) == want
        assert bytes(build(table)) == want
        assert len(build(segs)) == len(table)


def test_the_predictor_pair_of_tables_comes_from_two_calls():
    """Whole sequences (context + target rows) and target rows of two masks, as predictor_forward lays them out."""
    from jepa_amd.engine.layers import Seg
    enc = Seg.table(2, [6, 4])
    tgt = Seg.table(2, [3, 5])
    whole = Seg.table(2, [e.S + t.S for e, t in zip(enc, tgt)])
    assert tgt == [Seg(0, 2, 3), Seg(6, 2, 5)]
    assert whole == [Seg(0, 2, 9), Seg(18, 2, 9)]


def test_stream_log_is_one_list():
    from jepa_amd.engine import layers, streams
    assert layers._INDEP_LOG is streams._INDEP_LOG
    for name in ("SideStream", "side_stream", "independent_stream", "streams_concurrent", "low_priority_stream"):
        assert getattr(layers, name) is getattr(streams, name), name


OPS_PUBLIC = """gather_rows scatter_rows copy_rows tubelet_pack add_pos image_pack clip_transform clip_erase add_pos_bcast slice_sum pos_interp3d
pos_interp2d_bicubic add_pos_frames layernorm_fwd layernorm_bwd gemm_nt ln_rowstats ln_fold_weights gemm_nt_lnfold gemm_wgrad
gemm_wgrad_tn_grouped gemm_wgrad_tn transpose_colsum pad64 transpose transpose_multi colsum attn_fwd attn_bwd attn_fwd_segs attn_bwd_segs
attn_bwd_colsum gemm_dgelu_colsum reduce_segments xattn_fwd xattn_bwd pool_softmax_fwd pool_softmax_bwd pred_assemble target_rows
latent_loss token_pstd reg_grad reg_finish adamw_ema step_advance adamw_ema_guarded grad_stats_multi ema_update cast_bf16 sqnorm""".split()

NAMES = {
    "jepa_amd.engine.layers": ["Seg", "encoder_forward", "encoder_backward", "predictor_forward", "predictor_backward", "block_forward",
                               "block_backward", "side_stream", "independent_stream", "streams_concurrent", "USE_C_CHAIN", "LN_EPS",
                               "_INDEP_LOG"],
    "jepa_amd.engine.chain": ["Workspace", "TrunkCtx", "blocks_forward", "blocks_backward", "seg_array", "block_array", "prof_enable",
                              "prof_collect"],
    "jepa_amd.hip.ops": OPS_PUBLIC + ["Scratch", "KERNEL_TIMERS", "GEMM_FLAGS", "WGRAD_WS_BYTES", "GROUP_WS_BYTES", "_seg_array", "pad64"],
}


@pytest.mark.parametrize("module", sorted(NAMES))
def test_names_outside_code_imports_are_where_they_were(module):
    mod = importlib.import_module(module)
    missing = [n for n in NAMES[module] if not hasattr(mod, n)]
    assert not missing, missing
    for n in OPS_PUBLIC if module.endswith("ops") else ():
        assert callable(getattr(mod, n)), n
