"""Input edge of the step: pinned, double-buffered host-to-device staging of the next batch on a copy stream.

Reference: `load_clips()` (app/vjepa/train.py:391-408) issues `.to(device, non_blocking=True)` for every clip tensor
and every mask right before the step and the step then waits for them: 231 MB of fp32 pixels per step at ViT-L B=24
(PCIe Gen5 x16: >= 3.7 ms) sit on the critical path, 3.7 GB at the ViT-H B=384 recipe.  Here batch k+1 is copied while
step k computes:

    pf = DevicePrefetcher(fetch, device)          # fetch() -> (list of clip tensors [b,3,T,H,W], masks_enc, masks_pred)
    clips, masks_enc, masks_pred = pf.next()      # device tensors of batch k; batch k+1 is already in flight

Two device slots and two pinned host slots per stream of tensors; the copy stream waits until the step that consumed a
slot has been enqueued completely before overwriting it (event recorded on the compute stream at the following
`next()`), and the compute stream waits on the copy's event.  The only host-side wait is on the PINNED staging buffers:
before the host memcpy of batch k+depth into a slot's pinned buffer, the host waits for the event recorded after the
slot's previous H2D copy (batch k) -- normally long complete, so the wait is free, but without it a host that runs more
than `depth` steps ahead of the GPU (loss read every N steps, pageable loader tensors) would overwrite pixels a DMA has
not read yet.  The fp32 -> bf16 cast stays fused in `vj_tubelet_pack` (the copy moves the loader's fp32 pixels verbatim).

A clip entry may also be a `RawClipBatch` (app/vjepa/transforms.py: decoded uint8 frames of varying source size in one flat
buffer + descriptor and box tables).  Then the uint8 bytes and the two small tables are what crosses PCIe (3 bytes per SOURCE
pixel instead of 12 per output pixel: 0.38 x the fp32 clip for 240x320 sources at 224x224), and `vj_clip_transform` runs on the
copy stream, after the copies, into the slot's fp32 [B,3,T,S,S] buffer; `ready` is recorded after it, so `next()` hands out the same tensors as for fp32 batches.
The flat buffer changes size from batch to batch: its pinned and device staging buffers only ever grow.  A batch in the frozen
eval's normalise-first form goes through `vj_clip_transform_pre`, and a batch that carries RandomErasing boxes also ships its
noise and has `vj_clip_erase` write it, on the copy stream after the transform (no copy and no launch when no clip is erased).
A batch whose clips carry RandAugment plans ships the two plan tables too, and `vj_clip_randaug` rewrites the uploaded uint8 frames
in place on the copy stream BEFORE the transform, with a workspace kept in the slot (again nothing when no clip has an operation).
A batch in which some clip carries a resize (the validation transforms' `device_resize`: real frames of any size) has
`vj_clip_resample` bring every clip to its short-side size once, into a second frame buffer kept in the slot, and the transform
reads that buffer in place of the upload: the views of a clip are cut from the one resized copy (nothing when no clip is resized).

`EvalPrefetcher` is the same machinery for the batch structure of the frozen video eval (a list over segments of `RawClipBatch`,
labels, clip indices): it iterates like the loader it wraps and hands out what `run_one_epoch` takes.  `ImagePrefetcher` is its
sibling for the image evals: `(RawImageBatch, labels)` batches of decoded uint8 images, which `vj_image_resample` crops and resizes
on the copy stream as PIL would before `vj_clip_transform_pre` normalises them.  A batch whose images carry AutoAugment / RandAugment
plans (`data.auto_augment`) is mirrored on the uint8 side first (`vj_image_hflip`) and then augmented in place
(`vj_clip_randaug_fill`), as the reference's pipeline flips before its policy.
"""
import torch

from ..app.vjepa.transforms import RawClipBatch
from ..evals.image_classification_frozen.transforms import RawImageBatch, fill_colour
from ..hip import ops
from ..src.utils.tensors import repeat_interleave_batch


class DevicePrefetcher:
    def __init__(self, fetch, device, batch_size=None, num_clips=1, depth=2, timing=False):
        """fetch(): returns the next host batch `(clip_tensors, masks_enc, masks_pred)` (raises StopIteration when the
        data is exhausted -- the caller's `fetch` normally re-creates its loader instead).
        timing=True keeps, per batch, a pair of timing events in `edge_events`: the compute stream arriving at the input edge
        and the copy stream having finished the batch (tools/eval_bench.py reads the wait from them)."""
        self.fetch, self.device = fetch, torch.device(device)
        self.batch_size, self.num_clips, self.depth = batch_size, num_clips, depth
        self.copy_stream = torch.cuda.Stream(device=self.device)
        self._host = [dict() for _ in range(depth)]    # slot -> {key: pinned tensor}
        self._dev = [dict() for _ in range(depth)]     # slot -> {key: device tensor}
        self._free_ev = [None] * depth                 # compute-stream event: slot's previous contents are consumed
        self._h2d_done = [None] * depth                # copy-stream event: the slot's pinned buffers have been read
        self._slot = 0
        self._inflight = None                          # (slot, ready_event, staged batch)
        self._last_slot = None
        self.bytes_copied = 0
        self.timing, self.edge_events = timing, []

    @staticmethod
    def _fit(store, key, t, flat, **where):
        """The staging buffer of `store` that takes t: one of exactly t's shape, or (flat: a 1-D buffer whose length changes from
        batch to batch) the first t.numel() elements of one that grows (x1.25) and is never shrunk."""
        buf, n = store.get(key), t.numel()
        if flat:
            if buf is None or buf.numel() < n:
                buf = store[key] = torch.empty(max(n + n // 4, 1), dtype=t.dtype, **where)
            return buf[:n]
        if buf is None or buf.shape != t.shape or buf.dtype != t.dtype:
            buf = store[key] = torch.empty(t.shape, dtype=t.dtype, **where)
        return buf

    # -- one tensor through pinned staging into the slot's device buffer
    def _stage(self, slot, key, t, flat=False):
        t = t.contiguous()
        dev = self._fit(self._dev[slot], key, t, flat, device=self.device)
        src = t
        if not t.is_pinned():
            src = self._fit(self._host[slot], key, t, flat, pin_memory=True)
            src.copy_(t)        # pageable -> pinned (host memcpy; loaders with pin_memory=True skip this)
        dev.copy_(src, non_blocking=True)
        self.bytes_copied += t.numel() * t.element_size()
        return dev

    # -- uint8 frames + tables through staging, then the augmentation kernel into the slot's fp32 clip buffer
    def _stage_raw(self, slot, i, raw):
        raw.validate()                                 # on the host, before anything is copied
        frames = self._stage(slot, ("raw", i), raw.frames, flat=True)
        desc = self._stage(slot, ("desc", i), raw.desc)
        boxes = self._stage(slot, ("boxes", i), raw.boxes)
        if raw.augmented:
            # RandAugment comes first, on the uint8 frames, in place.  Only the layers in which some clip has an operation are
            # uploaded (each costs two launches); the workspace is the slot's and only ever grows.
            live = (raw.aug_ops != 0).any(0)
            aug_ops = self._stage(slot, ("aug_ops", i), raw.aug_ops[:, live].reshape(-1), flat=True).view(len(raw), -1)
            aug_args = self._stage(slot, ("aug_args", i), raw.aug_args[:, live].reshape(-1), flat=True).view(len(raw), -1, 6)
            need = ops.clip_randaug_ws_bytes(frames.numel(), len(raw), raw.num_frames)
            ws = self._dev[slot].get(("aug_ws", i))
            if ws is None or ws.numel() < need:
                ws = self._dev[slot][("aug_ws", i)] = torch.empty(need + need // 4, dtype=torch.uint8, device=self.device)
            ops.clip_randaug(frames, desc, raw.num_frames, aug_ops, aug_args, stream=self.copy_stream.cuda_stream, ws=ws)
        if raw.resized:
            # The validation transforms' short-side Resize: every clip once, whole frames, into a second frame buffer that the
            # transform reads in place of the upload (the views of a clip share the copy).  Buffer and workspace are the slot's
            # and only ever grow.
            B = len(raw) // raw.num_views
            rgeom, desc_out, nbytes, caps = raw.resample_plan()
            rgeom, desc_out = self._stage(slot, ("rgeom", i), rgeom), self._stage(slot, ("desc_out", i), desc_out)
            dev = self._dev[slot]
            resized = dev.get(("resized", i))
            if resized is None or resized.numel() < nbytes:
                resized = dev[("resized", i)] = torch.empty(nbytes + nbytes // 4, dtype=torch.uint8, device=self.device)
            need = ops.clip_resample.ws_bytes(B, raw.num_frames, caps)
            ws = dev.get(("resample_ws", i))
            if ws is None or ws.numel() < need:
                ws = dev[("resample_ws", i)] = torch.empty(need + need // 4, dtype=torch.uint8, device=self.device)
            ops.clip_resample(frames, desc[:B], rgeom, raw.num_frames, ops.BILINEAR, caps, resized, desc_out[:B],
                              stream=self.copy_stream.cuda_stream, ws=ws)
            frames, desc = resized, desc_out
        shape =(len(raw), 3, raw.num_frames, raw.crop_size, raw.crop_size)
        out = self._dev[slot].get(("clip", i))
        if out is None or tuple(out.shape) != shape or out.dtype != torch.float32:
            out = torch.empty(shape, dtype=torch.float32, device=self.device)
            self._dev[slot][("clip", i)] = out
        ops.clip_transform(frames, desc, boxes, raw.crop_size, raw.mean, raw.std, out=out, stream=self.copy_stream.cuda_stream,
                           pre=raw.pre)
        if raw.erased:
            noise = self._stage(slot, ("noise", i), raw.noise, flat=True)
            ebox = self._stage(slot, ("ebox", i), raw.ebox)
            noise_off = self._stage(slot, ("noise_off", i), raw.noise_off)
            ops.clip_erase(out, ebox, noise, noise_off, stream=self.copy_stream.cuda_stream)
        return out

    def _stage_batch(self, slot, batch):
        """What a host batch becomes on the device (called under the copy stream)."""
        clip_list, masks_enc, masks_pred = batch
        clips = [self._stage_raw(slot, i, u) if isinstance(u, RawClipBatch) else self._stage(slot, ("clip", i), u)
                 for i, u in enumerate(clip_list)]
        me = [self._stage(slot, ("me", i), m) for i, m in enumerate(masks_enc)]
        mp = [self._stage(slot, ("mp", i), m) for i, m in enumerate(masks_pred)]
        return clips, me, mp

    # -- the slot protocol: acquire a slot, stage under the copy stream, publish `ready` ...
    def _launch(self):
        batch = self.fetch()                           # StopIteration: nothing is in flight, no slot is taken
        slot = self._slot
        self._slot = (slot + 1) % self.depth
        if self._h2d_done[slot] is not None:
            self._h2d_done[slot].synchronize()         # the DMA engine is done with this slot's pinned staging buffers
        with torch.cuda.stream(self.copy_stream):
            if self._free_ev[slot] is not None:
                self.copy_stream.wait_event(self._free_ev[slot])
            staged = self._stage_batch(slot, batch)
            ready = torch.cuda.Event(enable_timing=self.timing)
            ready.record(self.copy_stream)
        self._h2d_done[slot] = ready
        self._inflight = (slot, ready, staged)

    # -- ... then retire the previous slot, wait for the batch, look ahead
    def _take(self, lookahead=True):
        cur = torch.cuda.current_stream()
        if self._last_slot is not None:   # everything that read the previous batch has been enqueued by now
            ev = torch.cuda.Event()
            ev.record(cur)
            self._free_ev[self._last_slot] = ev
        if self._inflight is None:
            self._launch()               # StopIteration of the source ends the data
        slot, ready, staged = self._inflight
        self._inflight = None
        if self.timing:
            arrive = torch.cuda.Event(enable_timing=True)
            arrive.record(cur)
            self.edge_events.append((arrive, ready))
        cur.wait_event(ready)
        self._last_slot = slot
        if lookahead:
            try:
                self._launch()           # batch k+1 overlaps step k
            except StopIteration:
                self._inflight = None
        return staged

    def next(self, lookahead=True):
        """Device tensors of the next batch (clips concatenated over num_clips, masks batch-repeated like
        train.py:398-406); starts copying the batch after it unless lookahead=False.  The train loop passes
        lookahead=False on the last iteration of an epoch: the reference re-creates its loader iterator at the first
        `next(loader)` of the next epoch, i.e. AFTER `sampler.set_epoch(epoch + 1)` (train.py:366-381) -- fetching across
        the boundary would permute epoch e+1 with epoch e's seed and draw one batch too many at the end of training."""
        clips, me, mp = self._take(lookahead)
        clips_d = clips[0] if len(clips) == 1 else torch.cat(clips, dim=0)
        if self.batch_size is not None:
            me = [repeat_interleave_batch(m, self.batch_size, repeat=self.num_clips) for m in me]
            mp = [repeat_interleave_batch(m, self.batch_size, repeat=self.num_clips) for m in mp]
        return clips_d, me, mp


class EvalPrefetcher(DevicePrefetcher):
    """The input edge of the frozen video eval.  `loader` yields `(segments, labels, clip_indices)` with `segments` a list over
    temporal segments of `RawClipBatch` (uint8 frames once per clip, V view-major box rows per clip:
    evals/video_classification_frozen/utils.py); iterating the prefetcher yields, per batch,

        ([[view 0, ..., view V-1] per segment] of fp32 [B,3,T,S,S] device tensors, labels, [clip indices per segment])

    all on the device -- what `run_one_epoch` and the probe bank's `_view_features` build themselves from fp32 loader batches with
    `.to(device)` (which is the identity on these).  The reference does those copies in front of the forward (eval.py:313-317);
    here batch k+1 is fetched, copied and transformed on the copy stream while batch k's frozen forward runs.  Slot reuse and the
    pinned-buffer wait are DevicePrefetcher's: this class supplies what is staged and what is handed out.  The tensors of a batch
    stay valid until the second `next` after it."""

    def __init__(self, loader, device, depth=2, timing=False):
        super().__init__(lambda: next(self._it), device, depth=depth, timing=timing)
        self.loader = loader
        self._it = None

    def __len__(self):
        return len(self.loader)

    @property
    def dataset(self):
        return self.loader.dataset

    def _stage_batch(self, slot, batch):
        segments, labels, clip_indices = batch
        clips = []
        for i, raw in enumerate(segments):
            if not isinstance(raw, RawClipBatch):
                raise TypeError(f"EvalPrefetcher: segment {i} is {type(raw).__name__}, expected the RawClipBatch that the eval's "
                                "transforms collate to (fp32 batches go to run_one_epoch as they are)")
            out, B = self._stage_raw(slot, i, raw), len(raw) // raw.num_views
            clips.append([out[v * B:(v + 1) * B] for v in range(raw.num_views)])
        lab = self._stage(slot, "labels", torch.as_tensor(labels))
        idx = [self._stage(slot, ("idx", i), torch.as_tensor(ci)) for i, ci in enumerate(clip_indices)]
        return clips, lab, idx

    def __iter__(self):
        self._it = iter(self.loader)
        self._inflight = None
        return self

    def __next__(self):
        return self._take()

    def next(self, lookahead=True):
        raise TypeError("EvalPrefetcher is iterated like the loader it wraps")


class ImagePrefetcher(EvalPrefetcher):
    """The input edge of the image evals.  `loader` yields `(RawImageBatch, labels)` (decoded uint8 images of mixed sizes in one
    flat buffer + descriptor and geometry tables: evals/image_classification_frozen/transforms.py); iterating the prefetcher yields
    `(fp32 [B,3,S,S] images, labels)` on the device -- what the image evals' run_one_epoch builds from fp32 loader batches with
    `.to(device)`, which is the identity on these.  On the copy stream, after the upload:
        vj_image_resample        PIL's resample of every crop box into the slot's uint8 [B,S,S,3] buffer
        vj_clip_transform_pre    that buffer as one-frame clips with identity boxes: (u / 255 - mean) / std and the flip
        vj_clip_erase            the RandomErasing noise, when a box was drawn
    and, for a batch in which some image carries a plan (RawImageBatch.augmented), between the first two
        vj_image_hflip           the flip, on the uint8 side: the policy sees the flipped crop (the flip column of the next but one
                                 kernel is then zero)
        vj_clip_randaug_fill     the plan on the [B,S,S,3] buffer as one-frame clips, fill colour round(255 * mean); only the layers
                                 in which some image has an operation; its workspace is kept in the slot and only grows
    so batch k+1 is fetched and transformed while batch k's forward runs, and fine-tuning's `mix` mixes in place in the slot's
    buffer.  The resample workspace is kept in the slot and only ever grows."""

    def _stage_images(self, slot, raw):
        raw.validate()                                 # on the host, before anything is copied
        B, S, stream = len(raw), raw.crop_size, self.copy_stream.cuda_stream
        frames = self._stage(slot, "raw", raw.frames, flat=True)
        desc = self._stage(slot, "desc", raw.desc)
        geom = self._stage(slot, "geom", raw.geom)
        dev = self._dev[slot]
        u8 = dev.get("u8")
        if u8 is None or tuple(u8.shape) != (B, S, S, 3):
            u8 = dev["u8"] = torch.empty((B, S, S, 3), dtype=torch.uint8, device=self.device)
        taps_x, taps_y, rows = raw.capacities()
        need = ops.ImageResample.ws_bytes(B, S, taps_x, taps_y, rows) if B else 0
        ws = dev.get("resample_ws")
        if ws is None or ws.numel() < need:
            ws = dev["resample_ws"] = torch.empty(max(need + need // 4, 16), dtype=torch.uint8, device=self.device)
        ops.ImageResample.run(frames, desc, geom, S, raw.filter, taps_x, taps_y, rows, out=u8, stream=stream, ws=ws)
        desc1, boxes1 = raw.resampled_tables()
        if raw.augmented:
            # the reference flips, then augments: mirror the uint8 crops now and hand the fp32 transform a zero flip column
            flips = desc1[:, 3].clone()
            desc_flip = self._stage(slot, "desc_flip", desc1)
            ops.image_hflip(u8, desc_flip, flips, stream=stream)
            desc1[:, 3] = 0
            live = (raw.aug_ops != 0).any(0)
            aug_ops = self._stage(slot, "aug_ops", raw.aug_ops[:, live].reshape(-1), flat=True).view(B, -1)
            aug_args = self._stage(slot, "aug_args", raw.aug_args[:, live].reshape(-1), flat=True).view(B, -1, 6)
            need = ops.clip_randaug_ws_bytes(u8.numel(), B, 1)
            aug_ws = dev.get("aug_ws")
            if aug_ws is None or aug_ws.numel() < need:
                aug_ws = dev["aug_ws"] = torch.empty(need + need // 4, dtype=torch.uint8, device=self.device)
            ops.clip_randaug(u8.view(-1), desc_flip, 1, aug_ops, aug_args, stream=stream, ws=aug_ws, fill=fill_colour(raw.mean))
        desc1, boxes1 = self._stage(slot, "desc1", desc1), self._stage(slot, "boxes1", boxes1)
        out = dev.get("images")
        if out is None or tuple(out.shape) != (B, 3, 1, S, S):
            out = dev["images"] = torch.empty((B, 3, 1, S, S), dtype=torch.float32, device=self.device)
        ops.clip_transform(u8.view(-1), desc1, boxes1, S, raw.mean, raw.std, out=out, stream=stream, pre=True)
        if raw.erased:
            noise = self._stage(slot, "noise", raw.noise, flat=True)
            ebox = self._stage(slot, "ebox", raw.ebox)
            noise_off = self._stage(slot, "noise_off", raw.noise_off)
            ops.clip_erase(out, ebox, noise, noise_off, stream=stream)
        return out.view(B, 3, S, S)

    def _stage_batch(self, slot, batch):
        raw, labels = batch
        if not isinstance(raw, RawImageBatch):
            raise TypeError(f"ImagePrefetcher: the batch holds {type(raw).__name__}, expected the RawImageBatch that the image "
                            "evals' transforms collate to (fp32 batches go to run_one_epoch as they are)")
        return self._stage_images(slot, raw), self._stage(slot, "labels", torch.as_tensor(labels))
