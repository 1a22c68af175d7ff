"""GPU: the two grow-only buffer caches keep their own keys and growth policies over the body they share (hip.ops.grow_only) --
ops.Scratch: per (GPU, tag, stream), exactly max(nbytes, 1 MiB) bytes; engine.chain.Workspace: per (GPU, tag), nbytes * 1.3 + 256,
dropped by tag prefix."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
KIB, MIB = 1 << 10, 1 << 20


def test_scratch_grows_to_the_exact_size_per_stream():
    from jepa_amd.hip.ops import Scratch
    tag = "test_engine_buffers"
    try:
        a = Scratch.get(4 * KIB, DEV, tag)
        assert a.dtype == torch.uint8 and a.device == DEV and a.numel() == MIB            # 1 MiB at least
        assert Scratch.get(3 * KIB, DEV, tag) is a and Scratch.get(MIB, DEV, tag) is a    # a smaller request: the same buffer
        b = Scratch.get(2 * MIB, DEV, tag)
        assert b is not a and b.numel() == 2 * MIB                                        # a larger one: a new buffer, exactly that size
        assert Scratch.get(MIB + 1, DEV, tag) is b and Scratch.get(4 * KIB, DEV, tag) is b
        c = Scratch.get(2 * MIB + 3 * KIB, DEV, tag)
        assert c is not b and c.numel() == 2 * MIB + 3 * KIB
        # one buffer per stream: two launches of a kernel family may be in flight on two streams
        s1, s2 = torch.cuda.Stream(device=DEV).cuda_stream, torch.cuda.Stream(device=DEV).cuda_stream
        assert s1 != s2
        p, q = Scratch.get(8 * KIB, DEV, tag, stream=s1), Scratch.get(8 * KIB, DEV, tag, stream=s2)
        assert p is not q and p.data_ptr() != q.data_ptr() and p is not c and q is not c
        assert Scratch.get(8 * KIB, DEV, tag, stream=s1) is p and Scratch.get(8 * KIB, DEV, tag, stream=s2) is q
        assert Scratch.get(4 * KIB, DEV, tag) is c                                        # the current stream's is untouched
    finally:
        for key in [k for k in Scratch._bufs if k[1] == tag]:
            del Scratch._bufs[key]


def test_workspace_grows_with_headroom_and_is_keyed_by_gpu_index():
    from jepa_amd.engine.chain import Workspace
    pre = "test_engine_buffers:"
    try:
        n = 300 * KIB
        a = Workspace.get(pre + "a", n, DEV)
        assert a.dtype == torch.uint8 and a.device == DEV and a.numel() == int(n * 1.3) + 256
        assert Workspace.get(pre + "a", 8 * KIB, DEV) is a and Workspace.get(pre + "a", a.numel(), DEV) is a
        n2 = a.numel() + 1
        b = Workspace.get(pre + "a", n2, DEV)
        assert b is not a and b.numel() == int(n2 * 1.3) + 256
        # 'cuda' and 'cuda:0' are the same GPU (the current device is 0)
        assert torch.cuda.current_device() == 0
        assert Workspace.get(pre + "a", 8 * KIB, torch.device("cuda")) is b
        c = Workspace.get(pre + "c", 8 * KIB, torch.device("cuda"))
        assert Workspace.get(pre + "c", 8 * KIB, DEV) is c and c is not b
        # release(prefix) drops exactly the prefixed tags
        other = "test_engine_buffers_other:"
        d = Workspace.get(other + "a", 8 * KIB, DEV)
        before = set(Workspace._bufs)
        Workspace.release(pre)
        assert before - set(Workspace._bufs) == {(0, pre + "a"), (0, pre + "c")}
        assert Workspace.get(other + "a", 8 * KIB, DEV) is d
        Workspace.release(other)
        assert before - set(Workspace._bufs) == {(0, pre + "a"), (0, pre + "c"), (0, other + "a")}
    finally:
        Workspace.release("test_engine_buffers")
