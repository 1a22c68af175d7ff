"""CPU checks of jepa_amd/hip/ops.py's one pointer helper and one launch path: the library is replaced by a recorder and the device
probes are patched, so every wrapper can be driven with host tensors and nothing can launch."""
import ctypes
import inspect
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from jepa_amd.hip import lib as L  # noqa: E402
from jepa_amd.hip import ops  # noqa: E402
from tests.test_engine_host import OPS_PUBLIC  # noqa: E402

QUERIES = {"vj_gemm_colsum_rows", "vj_attn_bwd_colsum_rows", "vj_grad_stats_chunks", "vj_last_error"}


class Recorder:
    """Stands in for the bound library: any vj_* attribute is a function that records (name, args) and returns rc[name] or 0."""

    def __init__(self, rc=None):
        self.calls, self.rc = [], dict(rc or {})

    def __getattr__(self, name):
        if not name.startswith("vj_"):
            raise AttributeError(name)

        def fn(*args):
            self.calls.append((name, args))
            return self.rc.get(name, 0)
        return fn

    def launches(self):
        return [n for n, _ in self.calls if not (n.endswith("_ws_bytes") or n in QUERIES)]


@pytest.fixture
def rec(monkeypatch):
    r = Recorder()
    monkeypatch.setattr(ops, "load_library", lambda: r)
    monkeypatch.setattr(L, "load_library", lambda: r)          # check() asks the library for its last error
    monkeypatch.setattr(ops, "_device", lambda: 0)
    monkeypatch.setattr(ops, "_raw_stream", lambda dev: 0)
    monkeypatch.setattr(ops.Scratch, "_bufs", {})
    return r


def b(*s):
    return torch.zeros(s, dtype=torch.bfloat16)


def f(*s):
    return torch.zeros(s, dtype=torch.float32)


def i64(*s):
    return torch.zeros(s, dtype=torch.int64)


def i32(*s):
    return torch.zeros(s, dtype=torch.int32)


def u8(*s):
    return torch.zeros(s, dtype=torch.uint8)


QKV, O, LSE, SEGS, ATT = (1, 48), (1, 16), (1, 1, 1), [(0, 1, 1)], (1, 16, 0.25)      # one token, one head of 16
ADAM = (1e-3, 0.05, 0.9, 0.999, 1e-8)

# one row per wrapper that hands tensors to a kernel: the smallest valid shapes, right dtypes, every tensor on the host
ROWS = {
    "gather_rows": lambda: ops.gather_rows(b(1, 2, 4), i64(1, 1)),
    "scatter_rows": lambda: ops.scatter_rows(b(1, 1, 4), i64(1, 1), 2),
    "copy_rows": lambda: ops.copy_rows(b(1, 2, 8), b(1, 2, 8), 1, 2, 0, 2, 0, 1, 8),
    "tubelet_pack": lambda: ops.tubelet_pack(f(1, 3, 2, 16, 16), 2, 16),
    "add_pos": lambda: ops.add_pos(b(1, 4), f(1, 4), 1, 1),
    "image_pack": lambda: ops.image_pack(f(1, 3, 16, 16), 2, 16),
    "clip_transform": lambda: ops.clip_transform(u8(48), i64(1, 4), i32(1, 1, 4), 4, (0, 0, 0), (1, 1, 1)),
    "clip_erase": lambda: ops.clip_erase(f(1, 3, 1, 4, 4), i32(1, 4), f(1), i64(1)),
    "clip_randaug": lambda: ops.clip_randaug(u8(48), i64(1, 4), 1, i32(1, 1), torch.zeros(1, 1, 6, dtype=torch.float64)),
    "add_pos_bcast": lambda: ops.add_pos_bcast(b(1, 4), f(1, 4), 1, 1, 1),
    "slice_sum": lambda: ops.slice_sum(b(1, 8), 1, 1, 1),
    "pos_interp3d": lambda: ops.pos_interp3d(f(1, 1, 1, 4), (1, 1, 1)),
    "pos_interp2d_bicubic": lambda: ops.pos_interp2d_bicubic(f(1, 1, 4), 1.0),
    "add_pos_frames": lambda: ops.add_pos_frames(b(1, 1, 4), f(1, 4), i64(1, 1), 1),
    "drop_path_add": lambda: ops.drop_path_add(b(1, 4), b(1, 4), f(1), 1, 1),
    "drop_path_scale": lambda: ops.drop_path_scale(b(1, 4), f(1), 1, 1),
    "clip_mix": lambda: ops.clip_mix(f(1, 1, 2, 2), f(1), i32(1, 4)),
    "soft_ce": lambda: ops.soft_ce(f(1, 2), i32(1), i32(1), f(1), 0.1),
    "layernorm_fwd": lambda: ops.layernorm_fwd(b(1, 4), f(4), f(4), 1e-6),
    "layernorm_bwd": lambda: ops.layernorm_bwd(b(1, 4), b(1, 4), f(4), f(1), f(1), f(4), f(4)),
    "gemm_nt": lambda: ops.gemm_nt(b(1, 8), b(1, 8)),
    "ln_rowstats": lambda: ops.ln_rowstats(b(1, 8), 1e-6),
    "ln_fold_weights": lambda: ops.ln_fold_weights(f(1, 8), f(1), f(8), f(8)),
    "gemm_nt_lnfold": lambda: ops.gemm_nt_lnfold(b(1, 8), b(1, 8), f(1), f(1, 2), f(1)),
    "gemm_wgrad": lambda: ops.gemm_wgrad(b(1, 64), b(1, 64), f(1, 1)),
    "gemm_wgrad_tn_grouped": lambda: ops.gemm_wgrad_tn_grouped([(b(1, 1), b(1, 1), f(1, 1))]),
    "gemm_wgrad_tn": lambda: ops.gemm_wgrad_tn(b(1, 1), b(1, 1), f(1, 1)),
    "transpose_colsum": lambda: ops.transpose_colsum(b(1, 1), f(1)),
    "transpose": lambda: ops.transpose(b(1, 1)),
    "transpose_multi": lambda: ops.transpose_multi(i64(6), i32(4), 1),
    "colsum": lambda: ops.colsum(b(1, 1), f(1)),
    "attn_fwd": lambda: ops.attn_fwd(b(*QKV), 1, 1, *ATT),
    "attn_bwd": lambda: ops.attn_bwd(b(*QKV), b(*O), b(*O), f(*LSE), 1, 1, *ATT),
    "attn_fwd_segs": lambda: ops.attn_fwd_segs(b(*QKV), SEGS, *ATT),
    "attn_bwd_segs": lambda: ops.attn_bwd_segs(b(*QKV), b(*O), b(*O), f(1), SEGS, *ATT, colsum=True),
    "attn_bwd_colsum": lambda: ops.attn_bwd_colsum(b(*QKV), b(*O), b(*O), f(*LSE), 1, 1, *ATT),
    "gemm_dgelu_colsum": lambda: ops.gemm_dgelu_colsum(b(1, 8), b(1, 8), b(1, 1)),
    "reduce_segments": lambda: ops.reduce_segments([(f(1, 1), f(1))]),
    "xattn_fwd": lambda: ops.xattn_fwd(b(1, 16), b(1, 32), 1, 1, 1, *ATT),
    "xattn_bwd": lambda: ops.xattn_bwd(b(1, 16), b(1, 32), b(1, 16), f(*LSE), 1, 1, *ATT),
    "pool_softmax_fwd": lambda: ops.pool_softmax_fwd(f(1, 1, 1)),
    "pool_softmax_bwd": lambda: ops.pool_softmax_bwd(b(1, 1, 1), f(1, 1, 1), f(1, 1)),
    "pred_assemble": lambda: ops.pred_assemble(b(1, 4), f(4), f(2, 4), i64(1, 1), i64(1, 1)),
    "target_rows": lambda: ops.target_rows(b(1, 4), f(4), f(4), i64(1, 1), 1, 1, 1e-6),
    "latent_loss": lambda: ops.latent_loss(b(4), f(4), f(1), dz=b(4)),
    "token_pstd": lambda: ops.token_pstd(b(1, 1, 4), f(1, 4), 1, 1, 4, False, stats=f(1, 4, 2)),
    "reg_grad": lambda: ops.reg_grad(b(1, 1, 4), f(1, 4), f(1, 4, 2), b(1, 1, 4), 1, 1, 4, 1, 1.0),
    "reg_finish": lambda: ops.reg_finish(f(1, 4), 1, f(1)),
    "adamw_ema": lambda: ops.adamw_ema(f(4), f(4), f(4), f(4), b(4), f(4), b(4), *ADAM, 1, 1.0, 0.998),
    "step_advance": lambda: ops.step_advance(f(4), f(1)),
    "adamw_ema_guarded": lambda: ops.adamw_ema_guarded(f(4), f(4), f(4), f(4), b(4), f(4), b(4), *ADAM, 1.0, 0.998, f(4), 0, 0.0, 1.0, f(1)),
    "grad_stats_multi": lambda: ops.grad_stats_multi(f(4), f(4), f(4), i64(1, 2), 1),
    "ema_update": lambda: ops.ema_update(f(4), f(4), b(4), 0.5),
    "cast_bf16": lambda: ops.cast_bf16(f(4), b(4)),
    "sqnorm": lambda: ops.sqnorm(f(4), f(2)),
}

# public functions that take no device tensor: they run on the host and launch nothing
HOST_ROWS = {
    "pad64": lambda: ops.pad64(65),
    "clip_randaug_ws_bytes": lambda: ops.clip_randaug_ws_bytes(48, 1, 1),
    "mix_tables": lambda: ops.mix_tables([1.0], [[0, 1, 0, 1]], 2, 2, "cpu"),
    "soft_ce_tables": lambda: ops.soft_ce_tables([0], [1], [0.5], 2, "cpu"),
}
NOT_WRAPPERS = {"grow_only", "seg_array", "check", "load_library"}


@pytest.mark.parametrize("name", sorted(ROWS))
def test_host_tensors_are_refused_before_anything_launches(rec, name):
    with pytest.raises(ValueError, match="GPU"):
        ROWS[name]()
    assert rec.launches() == [], rec.calls


@pytest.mark.parametrize("name", sorted(HOST_ROWS))
def test_host_side_functions_launch_nothing(rec, name):
    HOST_ROWS[name]()
    assert rec.launches() == [], rec.calls


def test_every_public_wrapper_has_a_row():
    """A wrapper added later without a row fails here: the rows cover OPS_PUBLIC and every other public function of ops.py."""
    public = {n for n, v in vars(ops).items() if inspect.isfunction(v) and not n.startswith("_")} - NOT_WRAPPERS
    rows = set(ROWS) | set(HOST_ROWS)
    assert not set(ROWS) & set(HOST_ROWS)
    assert set(OPS_PUBLIC) <= rows, sorted(set(OPS_PUBLIC) - rows)
    newer = {"drop_path_add", "drop_path_scale", "mix_tables", "clip_mix", "soft_ce_tables", "soft_ce", "clip_randaug",
             "clip_randaug_ws_bytes"}
    assert newer <= rows
    assert public == rows, sorted(public ^ rows)


# ------------------------------------------------------------------------------------------ _ptr and its sibling
class OnGpu(torch.Tensor):
    """A host tensor that says it is on the GPU: lets a test get past the device checks with the library stubbed."""
    is_cuda = True


def gpu(t):
    return t.as_subclass(OnGpu)


def test_ptr_and_addr():
    assert ops._ptr(None) is None                                   # ctypes passes None as NULL
    with pytest.raises(ValueError, match="GPU"):
        ops._ptr(f(2))
    with pytest.raises(ValueError, match="part: must live on the GPU"):
        ops._addr(f(2), "part")
    t = gpu(f(2))
    assert ops._ptr(t).value == t.data_ptr() == ops._addr(t, "t")
    assert isinstance(ops._ptr(t), ctypes.c_void_p)


def test_req_is_dev_plus_contiguity():
    t = gpu(f(2, 4))
    assert ops._dev(t, torch.float32, "t") is t and ops._req(t, torch.float32, "t") is t
    with pytest.raises(TypeError, match="t: expected torch.bfloat16"):
        ops._dev(t, torch.bfloat16, "t")
    with pytest.raises(ValueError, match="t: must live on the GPU"):
        ops._dev(f(2), torch.float32, "t")
    assert ops._dev(t.t(), torch.float32, "t") is not None          # the device part does not look at the layout
    with pytest.raises(ValueError, match="t: must be contiguous"):
        ops._req(t.t(), torch.float32, "t")


@pytest.fixture
def fake_scratch(monkeypatch):
    monkeypatch.setattr(ops.Scratch, "get", classmethod(lambda cls, nbytes, device, tag="default", stream=None: gpu(u8(8))))


@pytest.mark.parametrize("slot", range(3))
def test_grouped_wgrad_refuses_a_host_tensor_in_any_slot(rec, fake_scratch, slot):
    def problem():
        return [gpu(b(1, 1)), gpu(b(1, 1)), gpu(f(1, 1))]
    ops.gemm_wgrad_tn_grouped([tuple(problem()), tuple(problem())])
    assert rec.launches() == ["vj_gemm_bf16_tn_grouped"]
    bad = problem()
    bad[slot] = torch.Tensor(bad[slot])                                # the same tensor, on the host
    assert not bad[slot].is_cuda
    with pytest.raises(ValueError, match="GPU"):
        ops.gemm_wgrad_tn_grouped([tuple(problem()), tuple(bad)])
    assert rec.launches() == ["vj_gemm_bf16_tn_grouped"]


@pytest.mark.parametrize("slot", range(2))
def test_reduce_segments_refuses_a_host_tensor_in_any_slot(rec, slot):
    ops.reduce_segments([(gpu(f(2, 4)), gpu(f(4))), (gpu(f(2, 8))[:, :4], gpu(f(4)))])
    assert rec.launches() == ["vj_reduce_segments"]
    seg = rec.calls[-1][1][0][1]
    assert (seg.P, seg.N, seg.stride) == (2, 4, 8)
    bad = [gpu(f(2, 4)), gpu(f(4))]
    bad[slot] = torch.Tensor(bad[slot])
    with pytest.raises(ValueError, match="GPU"):
        ops.reduce_segments([(gpu(f(2, 4)), gpu(f(4))), tuple(bad)])
    assert rec.launches() == ["vj_reduce_segments"]


# ------------------------------------------------------------------------------------------ the launch path
def test_launch_appends_the_stream_and_names_the_symbol_it_called(rec):
    ops._launch("vj_anything", 1, 2.0)
    ops._launch("vj_anything", 3, stream=77)
    (n0, a0), (n1, a1) = rec.calls
    assert (n0, a0[:2], a0[2].value) == ("vj_anything", (1, 2.0), None)        # the patched current stream is 0 (NULL)
    assert (n1, a1[0], a1[1].value) == ("vj_anything", 3, 77)
    rec.rc["vj_anything"] = -1
    with pytest.raises(L.HipKernelError, match=r"^vj_anything failed \(rc=-1\)"):
        ops._launch("vj_anything")


def test_layernorm_bwd_failure_names_the_colsum_symbol(rec, fake_scratch):
    rec.rc["vj_layernorm_bwd_colsum"] = -1
    x = gpu(b(1, 4))
    with pytest.raises(L.HipKernelError, match=r"^vj_layernorm_bwd_colsum failed"):
        ops.layernorm_bwd(gpu(b(1, 4)), x, gpu(f(4)), gpu(f(1)), gpu(f(1)), gpu(f(4)), gpu(f(4)))
    assert rec.launches() == ["vj_layernorm_bwd_colsum"]


class _Event:
    log = []

    def __init__(self, enable_timing=False):
        assert enable_timing
        _Event.log.append(("new", self))

    def record(self):
        _Event.log.append(("record", self))


def test_timer_argument_costs_nothing_while_timers_are_off(rec, monkeypatch):
    monkeypatch.setattr(_Event, "log", [])
    monkeypatch.setattr(torch.cuda, "Event", _Event)
    monkeypatch.setattr(ops, "KERNEL_TIMERS", None)
    ops._launch("vj_k", 5, timer=("fam", 12.0))
    assert [n for n, _ in rec.calls] == ["vj_k"] and _Event.log == []


def test_timer_argument_puts_two_events_around_the_one_call(rec, monkeypatch):
    monkeypatch.setattr(_Event, "log", [])
    monkeypatch.setattr(torch.cuda, "Event", _Event)
    timers = {}
    monkeypatch.setattr(ops, "KERNEL_TIMERS", timers)
    real = rec.__getattr__("vj_k")
    rec.__dict__["vj_k"] = lambda *a: (_Event.log.append(("call", None)), real(*a))[1]
    ops._launch("vj_k", 5, timer=("fam", 12.0))
    ops._launch("vj_untimed", 5)
    assert [n for n, _ in rec.calls] == ["vj_k", "vj_untimed"]
    (e0, e1, work), = timers["fam"]
    assert work == 12.0 and list(timers) == ["fam"]
    assert _Event.log == [("new", e0), ("new", e1), ("record", e0), ("call", None), ("record", e1)]


# ------------------------------------------------------------------------------------------ single sites
def test_tensors_become_addresses_in_two_helpers_only():
    src = inspect.getsource(ops)
    inside = inspect.getsource(ops._ptr).count("data_ptr(") + inspect.getsource(ops._addr).count("data_ptr(")
    assert inside == 2 and src.count("data_ptr(") == inside


def test_the_library_is_fetched_in_the_launch_and_query_helpers_only():
    src = inspect.getsource(ops)
    inside = inspect.getsource(ops._launch).count("load_library(") + inspect.getsource(ops._query).count("load_library(")
    assert inside == 2 and src.count("load_library(") == inside
