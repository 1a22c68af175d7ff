"""HIP streams of the step beside the main one: the side stream (EMA-target forward, weight gradients), streams chosen to share a
hardware queue with none of the others (deferred update, gradient communication), and the probe that tells whether two streams
run concurrently."""
import ctypes
import os
import warnings

import torch

from ..hip.lib import check, load_library


def device_index(device=None):
    """The GPU a device names: None, 'cuda' and torch.device('cuda') all mean the current device, so 'cuda' and 'cuda:0' are one
    key for everything kept per GPU (streams, workspaces, pending-update events)."""
    idx = None if device is None else torch.device(device).index
    return torch.cuda.current_device() if idx is None else idx


class SideStream:
    """Second HIP stream of the step: the EMA-target forward in the forward phase, the weight-gradient GEMMs (and the
    reductions feeding the bias gradients) in the backward phase -- work that is off the main chain and fills the CUs its
    kernels leave idle.  `fork` makes the side stream wait for everything enqueued so far on the main stream; `join` makes
    the main stream wait for the side stream.  (A separate lowest-priority stream for the weight gradients was measured in
    round 3: no effect, +0.1 % in 7 of 8 interleaved rounds -- both phases are throughput-bound, not dispatch-order-bound.)"""

    def __init__(self, device):
        with torch.cuda.device(device):
            self.stream = independent_stream(device, [torch.cuda.current_stream(device)])
        self.enabled = os.environ.get("VJ_NO_OVERLAP", "0") != "1"   # serial mode for per-kernel profiling

    def fork(self, *tensors):
        self.stream.wait_stream(torch.cuda.current_stream())
        for t in tensors:          # allocator plumbing: these buffers are read on the side stream
            if t is not None:
                t.record_stream(self.stream)

    def join(self):
        torch.cuda.current_stream().wait_stream(self.stream)


def low_priority_stream(device):
    """A HIP stream of the LOWEST priority the device offers (torch.cuda.Stream only reaches the default and higher ones), wrapped
    for torch: the workgroups of the deferred fused update should take CUs only where the two forward streams leave them.
    Falls back to a plain stream when the runtime call is unavailable."""
    dev = torch.device(device)
    try:
        hip = ctypes.CDLL("libamdhip64.so")
        least, greatest = ctypes.c_int(0), ctypes.c_int(0)
        with torch.cuda.device(dev):
            if hip.hipDeviceGetStreamPriorityRange(ctypes.byref(least), ctypes.byref(greatest)) != 0:
                raise OSError("hipDeviceGetStreamPriorityRange")
            h = ctypes.c_void_p()
            if hip.hipStreamCreateWithPriority(ctypes.byref(h), 1, least.value) != 0 or not h.value:   # 1 = hipStreamNonBlocking
                raise OSError("hipStreamCreateWithPriority")
        return torch.cuda.ExternalStream(h.value, device=dev)
    except (OSError, AttributeError):
        return torch.cuda.Stream(device=dev)


_INDEP_LOG = []   # (candidate index, [concurrent with others[i]]) of every independent_stream() call: diagnostics / tests


def streams_concurrent(a, b, spin_us=300.0):
    """True when a kernel on stream `a` and one on stream `b` run at the same time (different hardware queues): two idle one-wave
    kernels of `spin_us` each (vj_probe_spin_stamped) leave their start / end stamps of the chip-wide 100 MHz timer in device memory;
    the streams are concurrent when the two intervals overlap by more than half a spin.  Judged on the DEVICE's clock (round 6; it was
    host wall-clock time around both, which eight ranks and their loader workers can stretch past any threshold).  Synchronises the
    two streams."""
    lib = load_library()
    ticks = int(spin_us * 100)
    dev = a.device if hasattr(a, "device") else torch.device("cuda", torch.cuda.current_device())
    stamps = torch.zeros(4, dtype=torch.int64, device=dev)
    torch.cuda.current_stream(dev).synchronize()      # the zero fill is complete before either probe writes
    best = 0
    for _ in range(2):                       # the first pass also pays one-time costs (code load, queue creation)
        check(lib.vj_probe_spin_stamped(ticks, stamps.data_ptr(), a.cuda_stream), "vj_probe_spin_stamped")
        check(lib.vj_probe_spin_stamped(ticks, stamps.data_ptr() + 16, b.cuda_stream), "vj_probe_spin_stamped")
        a.synchronize()
        b.synchronize()
        a0, a1, b0, b1 = stamps.tolist()
        best = max(best, min(a1, b1) - max(a0, b0))
    return best > ticks // 2


def independent_stream(device, others, make=None, tries=16):
    """A stream that shares a hardware queue with none of `others` (torch streams).  ROCclr maps streams onto GPU_MAX_HW_QUEUES
    hardware queues round-robin, and torch hands out its 32 pooled streams round-robin, so the n-th stream a process creates may
    land on the queue of the main or the side stream -- kernels of the two then serialise (measured: 72 -> 86 ms per step when the
    deferred update's stream aliased a forward stream, round 5; the same signature as the unexplained vj_comm_* slowdown of round 4).
    Candidates come from `make()` (default: torch.cuda.Stream) and are tested with streams_concurrent; the last one is returned
    with a warning if none is independent (GPU_MAX_HW_QUEUES too small)."""
    dev = torch.device(device)
    make = make or (lambda: torch.cuda.Stream(device=dev))
    cand = None
    for i in range(tries):
        cand = make()
        ok = [streams_concurrent(cand, o) for o in others]
        _INDEP_LOG.append((i, ok))
        if all(ok):
            return cand
    warnings.warn("jepa_amd: no stream independent of the existing ones was found (GPU_MAX_HW_QUEUES too small?); "
                  "streams will serialise on a shared hardware queue")
    return cand


_SIDE = {}


def side_stream(device):
    """One SideStream per GPU, keyed by device INDEX: the fork/join partners must be the same stream object."""
    idx = device_index(device)
    s = _SIDE.get(idx)
    if s is None:
        s = _SIDE[idx] = SideStream(torch.device("cuda", idx))
    return s
