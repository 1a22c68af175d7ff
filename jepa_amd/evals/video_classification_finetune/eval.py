"""Fine-tuning of a pretrained video encoder end to end through the attentive probe:

    from jepa_amd.evals.video_classification_finetune.eval import main
    main(args_eval_dict_from_yaml, resume_preempt=False)

The reference releases no such loop; this one is the frozen video eval (..video_classification_frozen.eval) with the encoder
left trainable.  It takes that eval's dictionary -- the same keys, `data.dataset_type: synthetic` / `synthetic_frames`,
`data.rand_augment` -- and one more section:

    optimization:
      finetune:
        encoder_lr: 0.0001            # peak learning rate of the encoder's last layer (default: optimization.lr)
        layer_decay: 0.75             # layer l of depth L trains at encoder_lr * layer_decay ** (L + 1 - l)
        encoder_weight_decay: 0.05    # constant; biases and 1-D tensors get 0
        clip_grad: null               # max global norm of the encoder's gradient
        drop_path: 0.0                # stochastic depth: block i of L drops each branch per clip at rate drop_path * i / (L - 1)
        recompute: none               # none | mlp | block: recompute block activations in the backward instead of keeping them
        mix:                          # absent (the default): off.  Present: the sub-keys left out take these values
          mixup_alpha: 0.8            # lam ~ Beta(alpha, alpha): x_i <- lam x_i + (1 - lam) x_(B-1-i); 0: no mixup
          cutmix_alpha: 1.0           # a box of area (1 - lam) S^2 of x_(B-1-i) replaces that of x_i; 0: no cutmix
          prob: 1.0                   # a batch is mixed with this probability
          switch_prob: 0.5            # a mixed batch is cutmix with this probability (when both alphas are > 0)
          label_smoothing: 0.1        # eps of the target eps / C + (1 - eps) (lam onehot(y_i) + (1 - lam) onehot(y_(B-1-i)))
          seed: 0                     # of the draws' own np.random.RandomState

A training iteration: the clips go through ClipAggregation with gradients enabled (one encoder call), the AttentiveClassifier,
the cross-entropy and backward(); the probe's optimizer steps exactly as in the frozen eval; then engine.finetune.EncoderFineTuner
steps the encoder at the probe's warm-up / cosine learning rate scaled by encoder_lr / lr.  Validation runs the encoder under
no_grad.  With `drop_path` > 0 the encoder, which stays in training mode, applies stochastic depth to the training iterations'
forward (VisionTransformer.set_drop_path_rate: one draw per clip, branch and block from the default CUDA generator, on the device);
the no_grad validation forward drops nothing.  The generator's state is not part of the checkpoint: a resumed run draws another
stream of drops than the uninterrupted one would have.  With a `mix` section (..mix: the draws and their order) every training batch
is mixed with its flipped self on the device, in place in the loader's buffers (vj_clip_mix: one plan per batch, the same tables for
every segment of a clip), and the loss is the soft-target cross-entropy with label smoothing (vj_soft_ce) per view; the semantics
are the ViT lineage's batch-mode mixup / cutmix, the random stream is this package's own (no bit-parity with timm's is claimed) and,
like the drop-path generator, not part of the checkpoint.  The training top-1 is counted against each clip's own label, a lower
bound under mixing; validation is untouched.  A section with both alphas and the smoothing at 0 counts as absent, and without the
key an iteration issues the launches it issued before.  The data, the probe, its update and schedules, the CSV log and the checkpoint are the frozen eval's (under
`<pretrain folder>/video_classification_finetune/`); the checkpoint adds `encoder` (a state dict in the reference's names, which
the frozen eval's load_pretrained(checkpoint_key='encoder') reads) and `encoder_opt` (Adam moments and step count in
torch.optim.AdamW's format).

`recompute` (VisionTransformer.set_activation_recompute) trades time for memory and nothing else: `block` keeps each block's input
alone and runs the block's forward again directly before its backward (about one more forward per iteration), `mlp` keeps all but the
two [M, 4D] tensors of the MLP and refills them with one fc1 GEMM per block.  Losses, gradients and weights are the same bits in every
mode, validation (no_grad) is untouched, and the checkpoint does not hold the mode: a run resumed with another one continues
bit-identically.  profiles/finetune_recompute.md has the measured time and memory.

Several ranks (launched as the frozen evals are: one process per GPU with one visible device each, RANK / WORLD_SIZE from the
launcher): the loaders shard as the frozen eval's do, the probe is wrapped in DistributedDataParallel as there, and the encoder's
gradients are averaged by the project's own bucketed reducer (engine.dp.GradReducer, driven by the encoder's backward: a block's
matrices go out as soon as the block is done, the small tensors after the backward) with the 1 / world folded into the encoder's
fused update, which therefore clips and guards the averaged gradient; a non-finite gradient on one rank skips the encoder's step
on all.  The tuner broadcasts rank 0's encoder at construction.  Rank r seeds a drop-path generator of its own with the global
seed + r and its MixDraw with `mix.seed` + r (rank_seeds), so the ranks drop different branches and each mixes its own local
batch; rank 0's seeds are the one-rank run's.  Every rank builds the checkpoint's entries, rank 0 writes them, every rank restores
them; the format is unchanged and a run may resume on another world size.  Only one-GPU hosts have been available: the path is
tested with two ranks on one device and timed at one forced rank (profiles/finetune_dp.md); scaling, the overlap under real
traffic and the cost of the small tensors' collectives are unmeasured.

Limits, all raising: video encoders at their native clip size (image encoders are frozen-path features, and so are still
images and off-native sizes unless the module opted in -- VisionTransformer.train_on_any_input, which this eval leaves off and
..image_classification_finetune.eval switches on); the lone probe (`optimization.multihead_kwargs` is the frozen evals'); every clip of a batch in one encoder call;
0 <= drop_path < 1; `recompute` one of none, mlp, block (the words: true, 1 and anything else raise); `mix`: alphas >= 0, probabilities in [0, 1], 0 <= label_smoothing < 1, unknown sub-keys raise.
"""
from types import SimpleNamespace

import torch

from ...engine.finetune import EncoderFineTuner
from ...engine.layers import recompute_mode
from ...src.utils.logging import get_logger
from ..mix import MixDraw
from ..video_classification_frozen import eval as frozen_eval

logger = get_logger(__name__)

FOLDER_NAME = 'video_classification_finetune/'


MIX_DEFAULTS = {'mixup_alpha': 0.8, 'cutmix_alpha': 1.0, 'prob': 1.0, 'switch_prob': 0.5, 'label_smoothing': 0.1, 'seed': 0}


def parse_mix(section):
    """The `optimization.finetune.mix` section -> the keywords of MixDraw (without num_classes), or None when the key is absent
    or switches nothing on (both alphas and the smoothing 0).  A present section takes the recipe's values for the sub-keys it
    leaves out."""
    if section is None:
        return None
    if not isinstance(section, dict):
        raise ValueError(f"optimization.finetune.mix: expected a mapping of {sorted(MIX_DEFAULTS)}, got {section!r}")
    unknown = sorted(set(section) - set(MIX_DEFAULTS))
    if unknown:
        raise ValueError(f"optimization.finetune.mix: unknown keys {unknown}")
    mix = {**MIX_DEFAULTS, **section}
    for k in ('mixup_alpha', 'cutmix_alpha', 'prob', 'switch_prob', 'label_smoothing'):
        if isinstance(mix[k], bool) or not isinstance(mix[k], (int, float)) or mix[k] != mix[k]:
            raise ValueError(f"optimization.finetune.mix.{k}: expected a number, got {mix[k]!r}")
    for k in ('mixup_alpha', 'cutmix_alpha'):
        if mix[k] < 0 or mix[k] == float('inf'):
            raise ValueError(f"optimization.finetune.mix.{k}={mix[k]} must be >= 0 and finite")
    for k in ('prob', 'switch_prob'):
        if not 0.0 <= mix[k] <= 1.0:
            raise ValueError(f"optimization.finetune.mix.{k}={mix[k]} must lie in [0, 1]")
    if not 0.0 <= mix['label_smoothing'] < 1.0:
        raise ValueError(f"optimization.finetune.mix.label_smoothing={mix['label_smoothing']} must lie in [0, 1)")
    if isinstance(mix['seed'], bool) or not isinstance(mix['seed'], int) or not 0 <= mix['seed'] < 2 ** 32:
        raise ValueError(f"optimization.finetune.mix.seed={mix['seed']!r} must be an integer in [0, 2^32)")
    if mix['mixup_alpha'] == 0 and mix['cutmix_alpha'] == 0 and mix['label_smoothing'] == 0:
        return None
    return mix


def parse_finetune(args_opt):
    """The `optimization.finetune` section with its defaults."""
    ft = args_opt.get('finetune', None) or {}
    unknown = sorted(set(ft) - {'encoder_lr', 'layer_decay', 'encoder_weight_decay', 'clip_grad', 'drop_path', 'mix', 'recompute'})
    if unknown:
        raise ValueError(f"optimization.finetune: unknown keys {unknown}")
    encoder_lr = ft.get('encoder_lr', None)
    return SimpleNamespace(encoder_lr=args_opt.get('lr') if encoder_lr is None else encoder_lr,
                           layer_decay=ft.get('layer_decay', 0.75),
                           encoder_weight_decay=ft.get('encoder_weight_decay', 0.05),
                           clip_grad=ft.get('clip_grad', None),
                           drop_path=ft.get('drop_path', 0.0),
                           mix=parse_mix(ft.get('mix', None)),
                           recompute=recompute_mode(ft.get('recompute', 'none'), "optimization.finetune.recompute") or 'none')


def rank_seeds(rank, world_size, mix_seed=0, global_seed=None):
    """(seed of the encoder's drop-path generator, seed of the MixDraw) of one rank.  Every rank seeds torch's default generator
    with the evals' global seed at import, so on several ranks the default generator would drop the same branches everywhere and a
    shared `mix.seed` would mix every local batch alike: each rank takes the global seed + rank and mix.seed + rank instead.  Rank
    0's are the one-rank seeds -- at world_size 1 the pair is returned for that comparison only: one rank installs no generator and
    draws from the default one, as it always has."""
    if not 0 <= rank < max(1, world_size):
        raise ValueError(f"rank_seeds: rank {rank} of {world_size}")
    base = frozen_eval._GLOBAL_SEED if global_seed is None else global_seed
    return base + rank, (mix_seed + rank) % 2 ** 32


class _FineTune:
    """What frozen_eval.main takes to leave the encoder trainable.  The image fine-tuning eval (..image_classification_finetune.eval)
    derives from it: `folder_name` and `encoder_of` are what differs."""

    folder_name = FOLDER_NAME

    def encoder_of(self, module):
        """The VisionTransformer inside what the frozen eval calls: here the ClipAggregation's model."""
        return module.model

    def check(self, cfg):
        if cfg.multihead is not None:
            raise ValueError("optimization.multihead_kwargs: a bank of probes belongs to the frozen evals (features of a FROZEN "
                             "encoder); fine-tuning trains the encoder through the lone probe")
        if cfg.frames_per_clip == 1:
            raise NotImplementedError("pretrain.frames_per_clip == 1: image encoders run on the frozen / no-grad path only")
        self.ft = parse_finetune(cfg.args_opt)

    def attach(self, cfg, run, aggregation):
        ft, encoder = self.ft, self.encoder_of(aggregation)
        encoder.set_drop_path_rate(ft.drop_path)
        encoder.set_activation_recompute(ft.recompute)
        aggregation.train()     # training iterations drop in training mode only; validation runs under no_grad and drops nothing
        tuner = EncoderFineTuner(encoder, layer_decay=ft.layer_decay, world_size=run.world_size)
        mix_args = ft.mix
        if run.world_size > 1:
            drop_seed, mix_seed = rank_seeds(run.rank, run.world_size, 0 if ft.mix is None else ft.mix['seed'])
            encoder.drop_path_generator = torch.Generator(device=run.device).manual_seed(drop_seed)
            if ft.mix is not None:
                mix_args = dict(ft.mix, seed=mix_seed)
            logger.info(f'rank {run.rank} of {run.world_size}: the encoder\'s gradients are averaged over the ranks '
                        f'({len(tuner.reducer.buckets)} buckets under the backward, {len(tuner.reducer.tail)} collectives after it); '
                        f'drop-path seed {drop_seed}, mix seed {mix_seed}; each rank mixes its own local batch')
        lr_ratio = ft.encoder_lr / cfg.lr

        def after_update(optimizer, grad_scale):
            # the probe's schedule has set this iteration's learning rate; the encoder follows its shape
            tuner.step(optimizer.param_groups[0]['lr'] * lr_ratio, ft.encoder_weight_decay, clip=ft.clip_grad, grad_scale=grad_scale)

        def extra_state():
            return {'encoder': {k: v.detach().cpu().clone() for k, v in encoder.state_dict().items()},
                    'encoder_opt': tuner.state_dict()}

        def restore_extra(checkpoint):
            msg = encoder.load_state_dict(checkpoint['encoder'])
            tuner.sync_shadows()
            tuner.load_state_dict(checkpoint['encoder_opt'])
            logger.info(f'loaded fine-tuned encoder and its optimizer state with msg: {msg}')

        logger.info(f'fine-tuning the encoder: lr {ft.encoder_lr} x {ft.layer_decay} ** (layers below the last), weight decay '
                    f'{ft.encoder_weight_decay}, clip {ft.clip_grad}, {len(tuner.param_groups)} parameter ranges, stochastic depth '
                    f'{ft.drop_path} (per block: {", ".join("%.3f" % r for r in encoder.drop_path_rates)}), activation recomputation '
                    f'{ft.recompute}')
        self.tuner = tuner
        epoch = dict(features_grad=True, after_update=after_update)
        if ft.mix is not None:
            epoch['mix'] = self.mix = MixDraw(num_classes=cfg.num_classes, **mix_args)
            logger.info('mixing the training batches with their flipped selves: ' + ', '.join(f'{k} {v}' for k, v in mix_args.items())
                        + ' (soft-target cross-entropy; the training top-1 is counted against the clips\' own labels)')
        return epoch, extra_state, restore_extra


def main(args_eval, resume_preempt=False):
    return frozen_eval.main(args_eval, resume_preempt, finetune=_FineTune())
