"""Data-parallel gradient averaging for the V-JEPA step: bucketed all-reduce over RCCL (xGMI) on a side HIP
stream, overlapped with the hand-written backward.

The reference wraps encoder/predictor in DistributedDataParallel (app/vjepa/train.py:295-297), whose reducer
only sees encoder gradients become final during the LAST of four backward passes (MultiMaskWrapper re-enters the
backbone per mask).  Here both masks share one chain, so a transformer layer's weight gradients are final as
soon as that layer's backward has been enqueued: `layer_done` records an event on the compute stream and
launches the all-reduce of that layer's contiguous slice of the gradient arena on the communication stream.
Small tensors (biases, LayerNorm affine, mask tokens) are reduced in one tail bucket.  The SUM is turned into the
mean inside the fused AdamW kernel (gscale = 1/world), so no extra pass touches the gradients.

The same reducer serves a stand-alone encoder that is fine-tuned (engine.finetune.EncoderFineTuner): its arena is laid out by
layer, so it hands in an explicit bucket plan (finetune_bucket_plan) and the encoder's own backward drives the hooks.

With world_size == 1 every method is a no-op.  On CPU tensors (gloo, used by the tests) the same bucket walk
runs synchronously.

Collectives (VJ_DP_COLL): every bucket's all-reduce is issued ON the engine's own communication stream -- a stream that was tested
for sharing a hardware queue with none of the compute streams (engine/streams.py independent_stream):
  "sync"  (default) torch.distributed's process group (backend "nccl" IS RCCL on ROCm; the group the launcher created), called with
          async_op=False inside the stream's context: ProcessGroupNCCL then launches on that stream;
  "capi"  the library's own RCCL binding (`vj_comm_*`, include/vjepa_hip.h: what a host without torch.distributed calls); the 128-byte
          unique id travels over the existing process group once, at construction;
  "async" round 2-4's form, async_op=True: ProcessGroupNCCL launches on a pooled stream of ITS OWN.  When that stream shares a hardware
          queue with a compute stream its event waits stall that stream's kernels: 86.6 - 87.2 ms per step against 71.3 at one rank,
          3 of 3 processes (profiles/r05_dp1_coll_mode.md) -- the signature of the "unexplained" 17 % of the capi route in rounds 3 / 4,
          whose communication stream was simply never checked (profiles/r04_dp1_capi_trace.md, r05_queue_aliasing.md).  Kept as the A/B control.
"""
import torch
import torch.distributed as dist

from .streams import independent_stream, side_stream


def trainer_bucket_plan(sl, n_enc, n_pred, pred_layers_per_bucket=4):
    """The buckets of the pretraining step's arena (slots `sl` named enc.* / pred.*): one per encoder block (its four matrices) at
    hook ("enc", li), the patch embedding's weight at ("enc", -1), the predictor's blocks in groups of pred_layers_per_bucket at
    the hook of each group's lowest block, predictor_proj.weight at ("pred", n_pred)."""
    def span(prefix, names):
        offs = [sl[prefix + n] for n in names]
        return (min(s.off for s in offs), max(s.off + ((s.numel + 63) // 64) * 64 for s in offs))

    buckets = {}
    mats = ["attn.qkv.weight", "attn.proj.weight", "mlp.fc1.weight", "mlp.fc2.weight"]
    for li in range(n_enc):
        buckets[("enc", li)] = [span(f"enc.blocks.{li}.", mats)]
    buckets[("enc", -1)] = [span("enc.", ["patch_embed.proj.weight"])]
    group = []
    for li in range(n_pred - 1, -1, -1):
        group.append(span(f"pred.predictor_blocks.{li}.", mats))
        if len(group) == pred_layers_per_bucket or li == 0:
            buckets[("pred", li)] = [(min(g[0] for g in group), max(g[1] for g in group))]
            group = []
    buckets[("pred", n_pred)] = [span("pred.", ["predictor_proj.weight"])]
    return buckets


def finetune_bucket_plan(slots, group_ranges, total=None):
    """The bucket plan of a fine-tuned encoder's arena (engine.finetune.EncoderFineTuner), from what weights.layout() returned for
    optstate.layer_decay_groups(...): pure, no device, no process group.  -> {(kind, layer): [(lo, hi)]} for GradReducer(plan=...).

    The decayed range of layer id l -- one contiguous range per (layer id, no-decay) group -- holds the matrices only:
      ("enc", li)  the decayed range of layer li + 1: the four matrices of block li, final when the hook of block li fires (their
                   weight gradients are on the side stream by then, which is what the bucket's launch waits for);
      ("enc", -1)  the decayed range of layer 0, patch_embed.proj.weight, final at the hook after the patch embedding's backward.
    No no-decay range is in the plan, so all of them fall to the tail, which finish() reduces after the whole backward.  They could
    not ride with their block: the LayerNorm backward of a NEIGHBOURING block writes some of them -- block li's fc2.bias comes out of
    norm1's backward of block li + 1 (the final norm's for the last block) or, under a stochastic-depth scale, out of block li's own
    column sum (layers._fc2_gb_route), proj.bias out of norm2's backward or a column sum -- and every LayerNorm's affine gradients
    are written on the main stream, which the hook's event (recorded on the side stream) does not cover.  Uncovered ranges that
    touch go out as one collective: the last block's small tensors and the final norm's are neighbours, so the tail of a depth-L
    encoder is L + 1 collectives (a range per block below the last, and the patch embedding's bias)."""
    from .optstate import is_no_decay, layer_id
    by_range = [[] for _ in group_ranges]
    for s in slots.values():
        hit = [i for i, (lo, hi) in enumerate(group_ranges) if lo <= s.off < hi]
        if len(hit) != 1:
            raise ValueError(f"finetune_bucket_plan: {s.name} at {s.off} lies in {len(hit)} of the ranges {group_ranges}")
        by_range[hit[0]].append(s)
    blocks = [int(s.name.split(".")[1]) for s in slots.values() if s.name.startswith("blocks.")]
    depth = max(blocks) + 1 if blocks else 0
    plan = {}
    for (lo, hi), members in zip(group_ranges, by_range):
        if not members:
            raise ValueError(f"finetune_bucket_plan: the range {(lo, hi)} holds no tensor")
        kinds = {is_no_decay(s.name, s.param) for s in members}
        layers = {layer_id(s.name, depth) for s in members}
        if len(kinds) != 1 or len(layers) != 1:
            raise ValueError(f"finetune_bucket_plan: the range {(lo, hi)} mixes layers {sorted(layers)} or decayed and no-decay "
                             "tensors: not the layout of optstate.layer_decay_groups")
        lid = layers.pop()
        if kinds.pop() or lid > depth:     # no-decay tensors, and anything decayed beside the blocks and the patch embedding: the tail
            continue
        key = ("enc", lid - 1)
        if key in plan:
            raise ValueError(f"finetune_bucket_plan: two decayed ranges for layer {lid}")
        plan[key] = [(lo, hi)]
    if total is not None and group_ranges and (group_ranges[0][0] != 0 or group_ranges[-1][1] != total):
        raise ValueError(f"finetune_bucket_plan: the ranges {group_ranges[0]} ... {group_ranges[-1]} do not span [0, {total})")
    return plan


class GradReducer:
    def __init__(self, arena, vit, pred, world_size, overlap=True, pred_layers_per_bucket=4, plan=None):
        """Two ways in.  The Trainer's: `vit` and `pred`, whose `enc.` / `pred.` names in the arena give the buckets
        (trainer_bucket_plan).  Any other arena's: `plan`, a mapping (kind, layer) -> [(lo, hi), ...] over arena.G whose keys are the
        hooks layer_done() is called with (vit and pred are then unused and may be None).  Either way the tail, reduced by finish(),
        is whatever the buckets leave uncovered of [0, arena.total)."""
        self.arena = arena
        import os
        self.world = world_size
        # VJ_FORCE_DP=1 exercises the bucket / stream / event path with a 1-rank RCCL communicator (single-GPU boxes)
        self.enabled = world_size > 1 or (os.environ.get("VJ_FORCE_DP", "0") == "1" and dist.is_available()
                                          and dist.is_initialized())
        self.overlap = overlap
        # How a bucket's collective is issued (VJ_DP_COLL): "sync" (default) = async_op=False inside the communication stream's context --
        # torch.distributed (>= 2.7) then launches the collective ON that stream, the one stream this engine has checked against the
        # compute streams' hardware queues; "async" = async_op=True: ProcessGroupNCCL launches it on a pooled stream of ITS OWN, which
        # nobody has checked -- when that stream shares a hardware queue with the main stream, its waits on the weight-gradient
        # stream's events stall the main stream's kernels and the two-stream backward serialises (profiles/r05_queue_aliasing.md).
        self.coll_mode = os.environ.get("VJ_DP_COLL", "sync")
        if self.coll_mode not in ("sync", "async", "capi"):
            raise ValueError(f"VJ_DP_COLL={self.coll_mode!r}: expected sync, async or capi")
        self._capi = None      # (library, vj_comm_t handle) when VJ_DP_COLL=capi
        self.extra_streams = []   # further streams the communication stream must not share a queue with (the deferred update's)
        self.buckets = {}      # (kind, layer) -> list of (lo, hi) ranges of arena.G that become final at that hook
        self.tail = []
        self._pending = []
        self.comm_stream = None
        self.launched = []     # (lo, hi) in launch order -- inspected by tests
        self._exposed = []     # (event before, event after) the compute stream's wait on the collectives, per step
        self.exposed_samples = 0
        if not self.enabled:
            return
        if plan is not None:
            # an explicit plan (a tuner's arena, finetune_bucket_plan): the hooks and ranges are the caller's, in its order
            self.buckets = {key: [(int(lo), int(hi)) for lo, hi in ranges] for key, ranges in plan.items()}
        else:
            self.buckets = trainer_bucket_plan(arena.slots, len(vit.blocks), len(pred.predictor_blocks), pred_layers_per_bucket)
        # everything not covered above (small tensors + predictor_embed + mask tokens) goes in the tail
        covered = sorted(r for rs in self.buckets.values() for r in rs)
        pos, total = 0, arena.total
        for lo, hi in covered:
            if lo > pos:
                self.tail.append((pos, lo))
            pos = max(pos, hi)
        if pos < total:
            self.tail.append((pos, total))
        # VJ_DP_DIAG (one-rank diagnostics of the capi route, lab/trips/r05_trip19.sh): "extracomm" = create the C-ABI communicator but reduce
        # through torch.distributed; "skipcall" = capi without the ncclAllReduce call itself (events and stream joins only)
        self._diag = os.environ.get("VJ_DP_DIAG", "")
        self.coll_check = None   # outcome of verify_collective_stream() (bench.py prints it in the `dp` object)
        if self.coll_mode == "capi" and not (arena.G.is_cuda and overlap):
            # (round-5 advisor finding: this used to fall back to torch.distributed silently while bench.py reported the C ABI)
            raise ValueError("VJ_DP_COLL=capi needs the gradient arena on a GPU and overlap_comm=True: the C-ABI collectives are "
                             "issued on the engine's communication stream")
        if (self.coll_mode == "capi" or self._diag == "extracomm") and arena.G.is_cuda:
            self._init_capi(arena.G.device)
            if self.coll_mode != "capi":
                self._capi_unused, self._capi = self._capi, None

    def _init_capi(self, device):
        """RCCL communicator through the C ABI: rank 0 draws the unique id, the process group broadcasts it."""
        import ctypes
        from ..hip.lib import check, load_library
        lib = load_library()
        n = lib.vj_comm_unique_id_bytes()
        idt = torch.zeros(n, dtype=torch.uint8, device=device)
        if dist.get_rank() == 0:
            buf = (ctypes.c_ubyte * n)()
            check(lib.vj_comm_unique_id(buf), "vj_comm_unique_id")
            idt.copy_(torch.tensor(list(buf), dtype=torch.uint8))
        dist.broadcast(idt, 0)
        raw = bytes(idt.cpu().tolist())
        handle = ctypes.c_void_p()
        check(lib.vj_comm_init(ctypes.byref(handle), dist.get_rank(), dist.get_world_size(), raw), "vj_comm_init")
        self._capi = (lib, handle)
        import weakref
        weakref.finalize(self, lib.vj_comm_destroy, handle)   # the communicator lives as long as the reducer (also the diagnostic one)

    @property
    def route(self):
        """The route the buckets actually take: 'capi' (vj_comm_* on the engine's communication stream), 'sync' / 'async'
        (torch.distributed on that stream / on ProcessGroupNCCL's own), or 'blocking' (no overlap: CPU tensors, overlap_comm=False)."""
        if not (self.arena.G.is_cuda and self.overlap):
            return "blocking"
        return "capi" if self._capi is not None else self.coll_mode

    def prepare(self, producer_stream=None):
        """Pick the communication stream and check where the process group's collectives really land -- at construction time of the
        Trainer (every rank calls it: the check issues two tiny collectives), not inside the first backward."""
        if not (self.enabled and self.arena.G.is_cuda and self.overlap):
            return
        self._pick_comm_stream()
        import os
        # (only RCCL groups: a gloo group -- the two-ranks-on-one-GPU parity test -- reduces on the host, there is no stream to check)
        if (self.coll_mode == "sync" and self._capi is None and os.environ.get("VJ_DP_VERIFY", "1") != "0"
                and dist.get_backend() == "nccl"):
            self.coll_check = self.verify_collective_stream()
            # the ranks decide TOGETHER (building the C-ABI communicator is itself a collective): any rank that saw its collectives on
            # another stream moves every rank to the capi route
            flag = torch.tensor([1.0 if self.coll_check["verdict"] == "other-stream" else 0.0], device=self.arena.G.device)
            dist.all_reduce(flag, op=dist.ReduceOp.MAX)
            self.coll_check["any_rank_other_stream"] = bool(flag.item() > 0)
            if self.coll_check["any_rank_other_stream"]:
                import warnings
                warnings.warn("jepa_amd: torch.distributed launched a blocking collective on a stream of its own instead of the current "
                              f"(communication) stream ({self.coll_check}); switching the gradient buckets to the C-ABI route (vj_comm_*), "
                              "which takes the stream as an argument")
                try:
                    self._init_capi(self.arena.G.device)
                    self.coll_check["fallback"] = "capi"
                except Exception as ex:   # keep the working (if slower) route rather than lose the run
                    self._capi = None
                    self.coll_check["fallback"] = f"capi unavailable ({type(ex).__name__}): staying on torch.distributed"

    def _pick_comm_stream(self):
        if self.comm_stream is not None:
            return
        # a communication stream that shares a hardware queue with neither compute stream: on a shared queue the collectives
        # and the backward serialise (engine/streams.py independent_stream)
        dev = self.arena.G.device
        with torch.cuda.device(dev):
            others = [torch.cuda.current_stream(dev), side_stream(dev).stream] + [x for x in self.extra_streams if x is not None]
            self.comm_stream = independent_stream(dev, others)

    def verify_collective_stream(self):
        """`sync` mode rests on a torch behaviour: ProcessGroupNCCL launches an async_op=False collective on the CURRENT stream
        (torch >= 2.7).  Nothing in torch's API says which stream a collective used, so one small all-reduce + all-gather are traced
        with torch.profiler (roctracer) next to a marker kernel issued on the communication stream, and the stream ids of the device
        activities are compared.  -> {'verdict': 'comm-stream' | 'other-stream' | 'unobserved' | 'unavailable', ...}.
        'unobserved': the collectives produced no device activity (a one-rank in-place all-reduce is a no-op) -- nothing to disprove."""
        from ..hip.lib import check, load_library
        out = {"verdict": "unavailable", "marker_stream": None, "collective_streams": [], "activities": []}
        lib = load_library()
        dev = self.arena.G.device
        t = torch.ones(4096, dtype=torch.float32, device=dev)
        g = torch.empty(4096 * max(1, dist.get_world_size()), dtype=torch.float32, device=dev)
        with torch.cuda.stream(self.comm_stream):   # (builds the communicator OUTSIDE the traced region: connection set-up is not what is checked)
            dist.all_reduce(t, op=dist.ReduceOp.SUM)
        t.fill_(1.0)
        torch.cuda.synchronize(dev)
        # The two collectives below are issued on EVERY rank whatever happens to the tracer on this one: a rank that skipped them
        # would leave the others waiting.  Tracing is best effort around them.
        prof = None
        try:
            from torch.profiler import ProfilerActivity, profile
            prof = profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA])
            prof.__enter__()
        except Exception as ex:   # no tracer in this build / a tracer already attached (rocprofv3)
            out["error"] = f"{type(ex).__name__}: {ex}"[:200]
            prof = None
        try:
            check(lib.vj_probe_spin(1000, self.comm_stream.cuda_stream), "vj_probe_spin")   # 10 us marker on the comm stream
        except Exception as ex:
            out["error"] = f"{type(ex).__name__}: {ex}"[:200]
        with torch.cuda.stream(self.comm_stream):
            dist.all_reduce(t, op=dist.ReduceOp.SUM)
            dist.all_gather_into_tensor(g, t)
        torch.cuda.synchronize(dev)
        if prof is None:
            return out
        try:
            prof.__exit__(None, None, None)
            marker, colls = None, []
            for e in prof.events():
                if str(e.device_type).endswith("CPU"):
                    continue
                nm = e.name.lower()
                if "probe_spin" in nm:
                    marker = e.device_resource_id
                elif any(k in nm for k in ("nccl", "rccl", "allreduce", "allgather", "all_reduce", "all_gather", "memcpy", "copy")):
                    colls.append((e.name[:48], e.device_resource_id))
            out["marker_stream"] = marker
            out["activities"] = colls[:6]
            out["collective_streams"] = sorted({sid for _, sid in colls})
            if marker is None:
                out["verdict"] = "unavailable"
            elif not colls:
                out["verdict"] = "unobserved"
            else:
                out["verdict"] = "comm-stream" if all(sid == marker for _, sid in colls) else "other-stream"
        except Exception as ex:
            out["error"] = f"{type(ex).__name__}: {ex}"[:200]
        return out

    def begin(self, producer_stream=None):
        """producer_stream: the HIP stream on which the per-layer weight gradients are enqueued (the engine's side
        stream); bucket launches wait on IT, so the main (dgrad) stream never stalls on a collective."""
        if not self.enabled:
            return
        self.launched = []
        self._pending = []
        self._ev_next = 0           # ordering events are pooled: one per bucket position, re-recorded every step
        self._producer = producer_stream
        if self.arena.G.is_cuda and self.overlap and self.comm_stream is None:
            self._pick_comm_stream()   # (normally done by prepare() when the Trainer is built)

    def _reduce(self, lo, hi, producer=None):
        g = self.arena.G[lo:hi]
        self.launched.append((lo, hi))
        if g.is_cuda and self.overlap:
            # (a stream's wait on an event binds to the record that precedes the wait call, so re-recording the same event
            #  object in the next step cannot disturb a wait that is already enqueued)
            pool = self.__dict__.setdefault("_ev_pool", [])
            nxt = self.__dict__.get("_ev_next", 0)
            if nxt >= len(pool):
                pool.append(torch.cuda.Event())
            ev = pool[nxt]
            self._ev_next = nxt + 1
            ev.record(producer if producer is not None else torch.cuda.current_stream())
            self.comm_stream.wait_event(ev)
            if self._capi is not None:
                from ..hip.lib import check
                lib, handle = self._capi
                if self._diag != "skipcall":
                    check(lib.vj_comm_allreduce_bucket(handle, g.data_ptr(), g.numel(), self.comm_stream.cuda_stream), "vj_comm_allreduce_bucket")
                return
            with torch.cuda.stream(self.comm_stream):
                if self.coll_mode == "async":
                    self._pending.append(dist.all_reduce(g, op=dist.ReduceOp.SUM, async_op=True))
                else:
                    dist.all_reduce(g, op=dist.ReduceOp.SUM)   # on comm_stream itself; finish() joins the stream
        else:
            dist.all_reduce(g, op=dist.ReduceOp.SUM)

    def layer_done(self, kind, layer):
        if not self.enabled:
            return
        for lo, hi in self.buckets.get((kind, layer), ()):
            self._reduce(lo, hi, getattr(self, "_producer", None))

    def finish(self):
        """Reduce the tail bucket and make the compute stream wait for every outstanding bucket."""
        if not self.enabled:
            return
        for lo, hi in self.tail:
            self._reduce(lo, hi)
        if self.arena.G.is_cuda and self.overlap:
            cur = torch.cuda.current_stream()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(cur)
            for w in self._pending:
                w.wait()   # enqueues a wait of the current (compute) stream on the collective; no host block
            cur.wait_stream(self.comm_stream)
            e1.record(cur)   # e0 -> e1 on the compute stream = communication NOT hidden under the backward
            self._exposed = (self._exposed + [(e0, e1)])[-16:]
        self._pending = []

    def exposed_ms(self):
        """Mean time per step the compute stream sat waiting for the gradient collectives (synchronises)."""
        if not self._exposed:
            return None
        torch.cuda.synchronize()
        self.exposed_samples = len(self._exposed)
        return sum(a.elapsed_time(b) for a, b in self._exposed) / len(self._exposed)


def broadcast_parameters(arena, tarena=None, src=0):
    """One-time parameter sync from rank 0 (DDP's _sync_module_states, reference train.py:295-297)."""
    if not (dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1):
        return
    dist.broadcast(arena.P, src)
    if tarena is not None:
        dist.broadcast(tarena.P, src)
