"""Fine-tuning of a pretrained video encoder on still images, end to end through the attentive probe:

    from jepa_amd.evals.image_classification_finetune.eval import main
    main(args_eval_dict_from_yaml, resume_preempt=False)

The reference releases no such loop; this one is the frozen image eval (..image_classification_frozen.eval) with the encoder left
trainable, the way ..video_classification_finetune.eval sits on the frozen video eval.  It takes the frozen image eval's dictionary
and the video fine-tuning eval's `optimization.finetune` section, key for key (encoder_lr, layer_decay, encoder_weight_decay,
clip_grad, drop_path, recompute, mix and its sub-keys: that module's docstring has the semantics; parse_finetune, parse_mix and the mechanics
of the encoder's step and checkpoint are its definitions, not copies).

A training iteration: the [B,C,H,W] batch goes through the video encoder with gradients enabled, in one call
(VisionTransformer.train_on_any_input, which this eval switches on for its encoder).  The repeated clip is never materialised, in
either direction: the forward embeds the gh*gw distinct tubelets of each image and fans them out over the temporal slices
(vj_image_pack, vj_add_pos_bcast), the backward sums the gradient over the slices (vj_slice_sum) and takes the patch embedding's
weight and bias gradients from B*gh*gw rows.  `data.resolution` may differ from the checkpoint's: the interpolated position table is
a constant of the backward.  Then the AttentiveClassifier, the cross-entropy, backward(), the probe's update and the encoder's
(engine.finetune.EncoderFineTuner at the probe's schedule scaled by encoder_lr / lr).  With `drop_path` > 0 the drops are drawn
per image; with a `mix` section every training batch is mixed with its flipped self in place (vj_clip_mix on the images as
one-frame clips) and the loss is the soft-target cross-entropy (vj_soft_ce).  Validation runs the frozen eval's no_grad forward.
The CSV log and the checkpoint are the frozen image eval's, under `<pretrain folder>/image_classification_finetune/`; the
checkpoint adds `encoder` (a state dict in the reference's names, which the frozen evals' load_pretrained reads with
`checkpoint_key: encoder`) and `encoder_opt` (Adam moments and step count in torch.optim.AdamW's format), as the video one does.

`data.auto_augment` (null, 'original' or a `rand-...` string such as 'rand-m9-mstd0.5-inc1', the usual image fine-tuning recipe) is
the frozen image eval's key, read by its parser (`parse_auto_augment`, re-exported here); `mix` still mixes the finished fp32 buffer.

Several ranks run as the video fine-tuning eval's do (its docstring: the sharded loader, the DistributedDataParallel probe, the
encoder's gradients averaged by engine.dp.GradReducer under the backward, per-rank drop-path and mix seeds, rank 0 writing the
checkpoint), tested with two ranks on one device; nothing about scaling is measured.

Limits, all raising: `pretrain.frames_per_clip` == 1 (the 2-D image encoder runs on the frozen / no-grad path only); the
lone probe (`optimization.multihead_kwargs` is the frozen evals'); every image of a batch in one encoder call (max_clips_per_call);
with `mix`, an image width that is a multiple of 4 (vj_clip_mix moves four pixels at a time) and square images; and those of the
`finetune` section itself.
"""
from ..image_classification_frozen import eval as frozen_eval
from ..image_classification_frozen.eval import parse_auto_augment  # noqa: F401  (one parser for both image evals)
from ..video_classification_finetune.eval import _FineTune

FOLDER_NAME = 'image_classification_finetune/'


class _ImageFineTune(_FineTune):
    """_FineTune for the frozen image eval, which calls the VisionTransformer itself on [B,C,H,W] batches."""

    folder_name = FOLDER_NAME

    def encoder_of(self, module):
        module.train_on_any_input(True)
        return module


def main(args_eval, resume_preempt=False):
    return frozen_eval.main(args_eval, resume_preempt, finetune=_ImageFineTune())
