"""Trainable state of a stand-alone video encoder that is fine-tuned end to end, the way engine.step.Trainer owns the context
encoder's: flat fp32 master / gradient / Adam-moment arenas with bf16 and transposed-bf16 shadows, and the fused AdamW update
with layer-wise learning-rate decay.

    tuner = EncoderFineTuner(encoder, layer_decay=0.75)       # a VisionTransformer on the GPU, num_frames > 1
    loss = criterion(classifier(encoder(clips)), labels)      # encoder.forward is one autograd node (engine.hipmodule)
    loss.backward()                                           # the chain writes the gradients into the arena
    tuner.step(lr, wd, clip=None)                             # AdamW per (layer, no-decay) range + bf16 re-cast + W^T refresh

The encoder's parameters become views of the arena and their `.grad` views of the gradient arena, so `_ModuleFn.backward` hands
autograd nothing for them: what the backward chain wrote IS the gradient (every backward overwrites it; nothing accumulates).
No kernel of its own: vj_sqnorm_f32, vj_step_advance, vj_adamw_ema_guarded (tgt = NULL) and the single-launch transposed refresh.

Several ranks (world_size > 1 with torch.distributed initialised at that size; VJ_FORCE_DP=1 with a one-rank group takes the same path,
as it does for the Trainer): the encoder is not wrapped in DistributedDataParallel -- autograd never sees its gradients, so DDP's
hooks would never fire.  The tuner builds engine.dp.GradReducer over its arena from dp.finetune_bucket_plan, broadcasts the master
weights from rank 0, and hands the reducer to the encoder, whose backward launches a block's bucket as soon as the block is done
and the small tensors' tail at the end.  The arena then holds the SUM over the ranks; step() folds 1 / world into the factor the
fused update already takes for the GradScaler, so the norm, the clip and the non-finite guard act on the averaged gradient, and a
non-finite value on any rank -- which the sum carries to every rank -- skips the step everywhere without a collective of its own.
"""
import os

import torch
import torch.distributed as dist

from ..hip import ops
from . import optstate
from .dp import GradReducer, broadcast_parameters, finetune_bucket_plan
from .streams import device_index, side_stream
from .weights import ParamArena, bump_generation, wait_pending_update


class EncoderFineTuner:
    def __init__(self, encoder, layer_decay=0.75, betas=(0.9, 0.999), eps=1e-8, world_size=1):
        group = dist.get_world_size() if dist.is_available() and dist.is_initialized() else 0     # 0: no process group
        if world_size > 1 and group != world_size:
            raise NotImplementedError(f"EncoderFineTuner: world_size={world_size}: fine-tuning runs on one rank (the encoder's "
                                      "gradients are not reduced across ranks; that is engine.dp's job)")
        if not getattr(encoder, "is_video", False):
            raise NotImplementedError("EncoderFineTuner: video (num_frames > 1) VisionTransformer only: image encoders run on the "
                                      "frozen / no-grad path")
        named = list(encoder.named_parameters())
        device = named[0][1].device
        if device.type != "cuda":
            raise ValueError("EncoderFineTuner: move the encoder to the GPU first (.to('cuda')): jepa_amd has no CPU compute path")
        if "_hip_shared" in encoder.__dict__:
            raise ValueError("EncoderFineTuner: the encoder's parameters already live in another arena (a Trainer or a tuner)")
        wait_pending_update()
        self.encoder = encoder
        self.device = device = torch.device("cuda", device_index(device))
        self.betas, self.eps, self.layer_decay = tuple(betas), float(eps), float(layer_decay)
        depth = len(encoder.blocks)
        groups = optstate.layer_decay_groups(named, depth, layer_decay)
        self.arena = A = ParamArena([g for _, g in groups], device, with_moments=True, bind_grads=True)
        for n, p in named:
            if n not in A.slots:     # the sincos table: fp32 beside the arena, as the private arena of engine.hipmodule has it
                p.data = p.data.to(device=device, dtype=torch.float32).contiguous()
                A.frozen[n] = p.data
        A.make_transposed([n + ".weight" for n in encoder._hip_linear_names()])
        encoder.__dict__.pop("_hip_private", None)
        encoder._hip_attach(A, "")
        # optimizer-facing view, as torch.optim.AdamW built from the same groups would hold it
        self.param_groups = [dict(gd, params=[p for _, p in g], lr=0.0, weight_decay=gd.get("weight_decay", 0.0), _range=i)
                             for i, (gd, g) in enumerate(groups)]
        self._slot_of = {id(s.param): s for s in A.slots.values()}
        self._step_dev = torch.zeros(1, dtype=torch.float32, device=device)   # Adam step count t (advanced on the device)
        self._stat = torch.zeros(4, dtype=torch.float32, device=device)       # [sum g^2, non-finite count, 0, 0]
        self.world = int(world_size)
        self.reducer = None
        if world_size > 1 or (group == 1 and os.environ.get("VJ_FORCE_DP", "0") == "1"):
            self._attach_reducer()

    def _attach_reducer(self):
        """Every rank calls this at the same point: prepare() and the broadcast are collectives."""
        A = self.arena
        self.reducer = GradReducer(A, None, None, self.world, plan=finetune_bucket_plan(A.slots, A.group_ranges, A.total))
        side = side_stream(self.device)
        self.reducer.prepare(side.stream if side.enabled else None)
        broadcast_parameters(A)      # nothing else makes the ranks start equal: no DDP wraps the encoder
        self.sync_shadows()
        self.encoder.grad_reducer = self.reducer

    # ------------------------------------------------------------------------------------------------ update
    @property
    def opt_step(self):
        return int(self._step_dev.item())

    @opt_step.setter
    def opt_step(self, v):
        self._step_dev.fill_(float(v))

    def step(self, lr, wd, clip=None, grad_scale=1.0):
        """One AdamW step of every range at lr * lr_scale (weight decay wd, 0 for the no-decay ranges), the bf16 shadows in the
        same pass, then the transposed shadows.  clip: max global gradient norm (torch.nn.utils.clip_grad_norm_), None for none.
        grad_scale: the factor a GradScaler put on the loss of this backward; the gradients and their norm are divided by it inside
        the update, and so is the number of ranks whose gradients the arena sums.  A non-finite gradient anywhere, on any rank,
        skips the whole step (weights, moments and the step count stay), decided on the device."""
        A = self.arena
        inv = 1.0 / (float(grad_scale) * self.world)      # (several ranks: the arena holds the sum of their gradients)
        ops.sqnorm(A.G, self._stat[0:2])     # the ranges tile the arena and its padding stays zero: one pass gives the global norm
        ops.step_advance(self._stat, self._step_dev)
        b1, b2 = self.betas
        for g, (lo, hi) in zip(self.param_groups, A.group_ranges):
            decay = 0.0 if g.get("WD_exclude", False) else wd
            ops.adamw_ema_guarded(A.P[lo:hi], A.G[lo:hi], A.M1[lo:hi], A.M2[lo:hi], A.Pb[lo:hi], None, None, lr * g["lr_scale"],
                                  decay, b1, b2, self.eps, inv, 0.0, self._stat, 0, float(clip) if clip else 0.0, inv,
                                  self._step_dev)
            g["lr"] = lr * g["lr_scale"]
            if not g.get("WD_exclude", False):
                g["weight_decay"] = wd
        A.refresh_transposed()
        bump_generation()   # parameters changed behind torch's version counters: derived-weight caches must refresh

    def grad_stats(self):
        """(global gradient norm, number of non-finite gradient elements) of the last step -- one host sync."""
        sq, bad = self._stat[:2].tolist()
        # (of the gradients as the backward left them, times grad_scale where one was given; on several ranks of their mean, so
        #  that a log compares with a one-rank run's)
        return sq ** 0.5 / self.world, int(bad)

    def zero_grad(self, set_to_none=False):
        """Clears the gradient arena.  The parameters' `.grad` stay views of it (set_to_none is ignored: a `.grad` that is not the
        arena's would be added to instead of written).  Every backward overwrites the arena, so a training loop need not call it."""
        self.arena.G.zero_()

    def sync_shadows(self):
        """Call after writing parameters from outside (load_state_dict on the encoder): refresh the bf16 / transposed shadows."""
        self.arena.refresh_bf16()
        self.arena.refresh_transposed()
        bump_generation()

    # ------------------------------------------------------------------------------------------------ checkpoints
    def state_dict(self):
        """torch.optim.AdamW-compatible state (exp_avg / exp_avg_sq / step per parameter) of an optimizer built from the same
        groups (optstate.layer_decay_groups), each group with its layer_id and lr_scale."""
        return optstate.build_state_dict(self.param_groups, self._slot_of, self.arena.M1, self.arena.M2, self.opt_step,
                                         self.betas, self.eps)

    def load_state_dict(self, sd):
        step = optstate.load_state_dict(self.param_groups, self._slot_of, self.arena.M1, self.arena.M2, sd)
        if step is not None:
            self.opt_step = step
