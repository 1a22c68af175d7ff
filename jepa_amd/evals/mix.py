"""Mixup, cutmix and label smoothing of encoder fine-tuning: the host side.

The semantics are those of the ViT lineage's batch-mode mixup (restated, never copied; the V-JEPA reference has none of this):
sample i of a batch of B is mixed with sample B-1-i, every sample of a batch under the same draw.

    MixDraw.draw(B, S) -> plan          the draws of one batch (below) as the tables the kernels take
    ops.clip_mix(x, lam, box)           the pixels, in place (csrc/clip_mix.hip)
    SoftTargetCrossEntropy              the loss against  t_c = eps / C + (1 - eps) * (lam * [c == y_i] + (1 - lam) * [c == y_j])
                                        (csrc/soft_ce.hip), mean over the batch of  -sum_c t_c log_softmax(z)_c

Order of the draws of one batch, all from the MixDraw's OWN np.random.RandomState(seed) -- the transforms draw from the global
`random` / `np.random`, whose streams a MixDraw never moves:
  1. u = rand():  the batch is mixed iff u < prob (no draw at all when both alphas are 0: nothing can be mixed);
  2. a mixed batch with both alphas > 0:  rand() < switch_prob chooses cutmix (with one alpha > 0 the mode is fixed, no draw);
  3. lam = beta(alpha, alpha) with the chosen mode's alpha;
  4. cutmix only:  cy = randint(S), cx = randint(S);  r = sqrt(1 - lam), cut_h = cut_w = int(S * r), the box is
     y0, y1 = clip(cy -/+ cut_h // 2, 0, S) and the same in x, and lam becomes 1 - area / S^2.
An unmixed batch consumes draw 1 only.  Bit-parity with timm's random stream is NOT claimed: the recipe is the same, the stream is
this module's own.  The state of the generator is not part of the eval's checkpoint (like the drop-path generator's): a resumed run
draws another stream of plans than the uninterrupted one would have.
"""
from types import SimpleNamespace

import numpy as np
import torch

from ..hip import ops


class MixDraw:
    """The per-batch draws of mixup / cutmix, and the label smoothing that goes with them into the loss."""

    def __init__(self, mixup_alpha=0.8, cutmix_alpha=1.0, prob=1.0, switch_prob=0.5, label_smoothing=0.1, num_classes=None, seed=0):
        if mixup_alpha < 0 or cutmix_alpha < 0:
            raise ValueError(f"MixDraw: mixup_alpha={mixup_alpha}, cutmix_alpha={cutmix_alpha} must be >= 0")
        if not (0.0 <= prob <= 1.0 and 0.0 <= switch_prob <= 1.0):
            raise ValueError(f"MixDraw: prob={prob}, switch_prob={switch_prob} must lie in [0, 1]")
        if not 0.0 <= label_smoothing < 1.0:
            raise ValueError(f"MixDraw: label_smoothing={label_smoothing} must lie in [0, 1)")
        if num_classes is None or int(num_classes) < 1:
            raise ValueError(f"MixDraw: num_classes={num_classes}")
        self.mixup_alpha, self.cutmix_alpha = float(mixup_alpha), float(cutmix_alpha)
        self.prob, self.switch_prob = float(prob), float(switch_prob)
        self.label_smoothing = float(label_smoothing)
        self.num_classes = int(num_classes)
        self.seed = seed
        self.rng = np.random.RandomState(seed)

    def draw(self, B, S):
        """The plan of one batch of B clips of S x S pixels:
          mixed      bool: False = no sample changes (pixel_lam all 1, boxes empty; no clip_mix launch is needed)
          mode       'mixup', 'cutmix' or None
          lam        fp32 [B]: the weight of a sample's own label in its target (1 - area / S^2 for cutmix, exactly)
          box        int32 [B,4] = (y0, y1, x0, x1): the partner's pixels replace this region (empty unless cutmix)
          pixel_lam  fp32 [B]: the blend weight of the pixels outside the box (lam for mixup; 1 for cutmix, which only swaps)."""
        rng = self.rng
        lam, pixel_lam, box, mode = 1.0, 1.0, (0, 0, 0, 0), None
        if (self.mixup_alpha > 0 or self.cutmix_alpha > 0) and rng.rand() < self.prob:
            if self.mixup_alpha > 0 and self.cutmix_alpha > 0:
                mode = 'cutmix' if rng.rand() < self.switch_prob else 'mixup'
            else:
                mode = 'cutmix' if self.cutmix_alpha > 0 else 'mixup'
            alpha = self.cutmix_alpha if mode == 'cutmix' else self.mixup_alpha
            lam = float(rng.beta(alpha, alpha))
            if mode == 'cutmix':
                cy, cx = int(rng.randint(S)), int(rng.randint(S))
                cut = int(S * np.sqrt(1.0 - lam))
                y0, y1 = int(np.clip(cy - cut // 2, 0, S)), int(np.clip(cy + cut // 2, 0, S))
                x0, x1 = int(np.clip(cx - cut // 2, 0, S)), int(np.clip(cx + cut // 2, 0, S))
                box = (y0, y1, x0, x1)
                lam = 1.0 - (y1 - y0) * (x1 - x0) / float(S * S)
            else:
                pixel_lam = lam
        return SimpleNamespace(mixed=mode is not None, mode=mode,
                               lam=np.full((B,), lam, dtype=np.float32),
                               pixel_lam=np.full((B,), pixel_lam, dtype=np.float32),
                               box=np.tile(np.asarray(box, dtype=np.int32), (B, 1)))


def mix_batch(mix, clips, labels, device):
    """One training batch under a MixDraw: draws its plan, mixes every view of every segment in place with the same tables (the
    segments of a clip share its label, so they share its partner, weight and box) and returns the loss's tables
    (label_a, label_b, lam) on the device.  clips: the epoch's [[view, ...] per segment] of fp32 [B,3,T,S,S] device tensors;
    labels: the batch's labels (validated on the host: a device tensor is read back once).  An unmixed plan launches nothing."""
    B, S = clips[0][0].shape[0], clips[0][0].shape[-1]
    plan = mix.draw(B, S)
    if plan.mixed:
        lam_d, box_d = ops.mix_tables(plan.pixel_lam, plan.box, S, S, device)
        for segment in clips:
            for view in segment:
                ops.clip_mix(view, lam_d, box_d)
    host = torch.as_tensor(labels).cpu()
    return ops.soft_ce_tables(host, host.flip(0), plan.lam, mix.num_classes, device)


class SoftTargetCrossEntropy(torch.autograd.Function):
    """mean over the rows of ops.soft_ce: forward(logits fp32 [R,C], label_a, label_b, lam (the device tables of
    ops.soft_ce_tables), smoothing, probs=False) -> (loss, the soft-max [R,C] or None).  Backward: the saved softmax - target times
    grad_out / R, one torch multiply; the soft-max output carries no gradient, and there is no double backward."""

    @staticmethod
    def forward(ctx, logits, label_a, label_b, lam, smoothing, probs=False):
        loss_rows, dlogits, p = ops.soft_ce(logits, label_a, label_b, lam, smoothing, probs=probs)
        ctx.save_for_backward(dlogits)
        if p is not None:
            ctx.mark_non_differentiable(p)
        return loss_rows.mean(), p

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_loss, grad_probs=None):
        dlogits, = ctx.saved_tensors
        return dlogits * (grad_loss / dlogits.shape[0]), None, None, None, None, None
