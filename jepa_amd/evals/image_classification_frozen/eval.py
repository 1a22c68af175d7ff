"""Frozen image-classification eval with the reference's entry point and YAML schema
(evals/image_classification_frozen/eval.py:63-503), the eval of the nine `*_in1k`, `*_inat` and `*_places` configs:

    from jepa_amd.evals.image_classification_frozen.eval import main
    main(args_eval_dict_from_yaml, resume_preempt=False)

Same config keys, probe (AttentiveClassifier on all tokens of the frozen encoder), optimizer groups, schedules, loss and accuracy
arithmetic, CSV columns, checkpoint dictionary and folder / file names.  Differences from the reference:
  - with `pretrain.frames_per_clip` > 1 (every shipped image config) the encoder is the VIDEO ViT and takes the [B,C,H,W] batch
    itself: the reference's forward pre-hook that repeats every image `frames_per_clip` times (eval.py:451-457) is not registered
    and the repeated clip is never materialised (vj_image_pack / vj_add_pos_bcast, bit-identical to feeding the repeated clip).
    `data.resolution` may differ from the checkpoint's: the position table is interpolated (vj_pos_interp3d) when the model is
    called at another size than it was built for, and load_pretrained keeps the model's own table when the shapes differ.
  - with `pretrain.frames_per_clip` == 1 (the reference's default) the encoder is the 2-D image ViT, fed the [B,C,H,W] batch as the
    reference feeds it (no pre-hook is registered there, eval.py:451); its table is interpolated bicubically at other square sizes
    (vj_pos_interp2d_bicubic).
  - bf16 compute, `use_bfloat16`, `use_silu` and the DistributedDataParallel wrapping are handled exactly as in the video eval
    (..video_classification_frozen.eval, whose load_pretrained, init_model and init_opt are this file's too; what the two evals
    share beyond those is in ..frozen).
  - `data.dataset_name` is `synthetic` (seeded labelled fp32 images, src/datasets/data_manager.py: SyntheticImageClassification),
    `synthetic_images` (seeded labelled uint8 images of mixed sizes) or `image_folder` (<root_path>/<image_folder>/{train,val}/
    <class>/<file>, read with PIL; src/datasets/image_datasets.py).  The last two go through the reference's image transforms
    (eval.py:379-423: random-resized crop bicubic, flip, RandomErasing 0.25 to train; Resize bilinear + CenterCrop to validate) as
    draws on the host (.transforms) and pixel work on the device: uint8 bytes are uploaded, vj_image_resample does PIL's antialiased
    resample byte for byte, vj_clip_transform_pre and vj_clip_erase the rest, on a copy stream one batch ahead of the forward
    (engine.input.ImagePrefetcher).  The reference's own dataset classes (ImageNet, iNat21, Places205, `subset_file`) are not part
    of this package, and stream parity with timm / torchvision draws is not claimed.  Extension keys `data.synthetic_length` (items
    per split, default 8 batches), `data.num_workers` (default 0) and `data.auto_augment` (default null: off).
  - the reference's training transform also asks timm for `auto_augment='original'` (eval.py:392-403).  Here that is
    `data.auto_augment: original` (or a `rand-...` string, timm's RandAugment form): the training transform then draws the policy's
    plan for the flipped S x S crop and the device carries it out on the uint8 side (vj_image_hflip, vj_clip_randaug_fill with the
    fill colour round(255 * mean)), byte for byte what PIL gives for that plan.  The policy table was not checked against a timm
    install.  The key needs uint8 images: with `dataset_name: synthetic` it raises.  Without the key the eval issues the launches
    and produces the bits it always did.
  - one encoder call never holds more images than keep fc1's output below 2^31 elements, counted from the tokens the actual input
    makes (frozen_features).
  - `main` returns a small record of the run (per-epoch accuracies, per-iteration training loss and learning rate).
  - `main(finetune=...)` and run_one_epoch's `features_grad`, `after_update` and `mix` are what ..image_classification_finetune.eval
    brings to train the encoder with the probe; without them this eval runs what it always ran.
"""
import os
import pprint

import numpy as np
import torch

from ...engine.input import ImagePrefetcher
from ...src.datasets.data_manager import SyntheticImageClassification
from ...src.datasets.image_datasets import ImageFolder, SyntheticImages
from ...src.models.attentive_pooler import AttentiveClassifier
from ...src.utils.logging import get_logger
from ..frozen import classifier_state_dict, load_checkpoint  # noqa: F401  (the reference's names in this file)
from ..frozen import distributed as _distributed
from ..frozen import (chunked_call, freeze, max_clips_per_call, parse_config, run_probe_epoch, setup_run, synthetic_dataloader,
                      train_single_probe, widest_activation)
from ..mix import SoftTargetCrossEntropy, mix_batch
from ..multihead import run as run_multihead
from ..video_classification_frozen.eval import init_model, init_opt, load_pretrained  # noqa: F401
from ...app.vjepa.randaugment import auto_augment_draw
from .transforms import make_transforms

logger = get_logger(__name__)

_GLOBAL_SEED = 0
np.random.seed(_GLOBAL_SEED)
torch.manual_seed(_GLOBAL_SEED)

pp = pprint.PrettyPrinter(indent=4)

UINT8_DATASETS = ('synthetic_images', 'image_folder')   # decoded uint8 images through the transform, staged by ImagePrefetcher
_auto_augment_logged = False


def parse_auto_augment(args_data):
    """`data.auto_augment` of both image evals (extension; absent / null: off, 'original', or a `rand-...` string), validated by the
    one parser (app/vjepa/randaugment.auto_augment_draw) and against the dataset: finished fp32 images cannot be augmented."""
    value = (args_data or {}).get('auto_augment', None)
    auto_augment_draw(value)                      # raises ValueError naming what is accepted
    kind = str((args_data or {}).get('dataset_name')).lower()
    if value is not None and kind not in UINT8_DATASETS:
        raise ValueError(f"data.auto_augment needs uint8 images (dataset_name: {' or '.join(UINT8_DATASETS)}); {kind!r} yields "
                         "finished fp32 images")
    return value


def main(args_eval, resume_preempt=False, finetune=None):
    """finetune (extension): None (the frozen eval), or what ..image_classification_finetune.eval brings to train the encoder with
    the probe on this eval's data, probe, schedules and checkpoints: `folder_name`; check(cfg), called before anything is set up;
    attach(cfg, run, encoder) -> (epoch keywords of the training run_one_epoch, extra_state, restore_extra of
    frozen.train_single_probe), called on the encoder instead of freezing it."""
    cfg = parse_config(args_eval, resume_preempt)
    multihead = cfg.multihead
    if finetune is not None:
        finetune.check(cfg)

    # -- DATA
    args_data = args_eval.get('data')
    dataset_name = args_data.get('dataset_name')
    num_classes = cfg.num_classes = args_data.get('num_classes')
    root_path = args_data.get('root_path', None)
    image_folder = args_data.get('image_folder', None)
    resolution = args_data.get('resolution', 224)
    synthetic_length = args_data.get('synthetic_length', None)
    num_workers = args_data.get('num_workers', 0)
    auto_augment = parse_auto_augment(args_data)

    run = setup_run(cfg, 'image_classification_frozen/' if finetune is None else finetune.folder_name, csv=multihead is None)
    device = run.device

    # -- pretrained encoder (frozen): the video ViT, or the image ViT with frames_per_clip == 1; both are fed [B,C,H,W] directly
    encoder = init_model(crop_size=resolution, device=device, pretrained=cfg.pretrained_path, model_name=cfg.model_name,
                         patch_size=cfg.patch_size, frames_per_clip=cfg.frames_per_clip, tubelet_size=cfg.tubelet_size,
                         uniform_power=cfg.uniform_power, checkpoint_key=cfg.checkpoint_key, use_SiLU=cfg.use_SiLU,
                         tight_SiLU=cfg.tight_SiLU, use_sdpa=cfg.use_sdpa)
    tune, extra = {}, {}
    if finetune is None:
        freeze(encoder)
    else:
        tune, extra['extra_state'], extra['restore_extra'] = finetune.attach(cfg, run, encoder)

    # -- init classifier
    if multihead is None:
        classifier = AttentiveClassifier(embed_dim=encoder.embed_dim, num_heads=encoder.num_heads, depth=1,
                                         num_classes=num_classes).to(device)

    common = dict(dataset_name=dataset_name, root_path=root_path, resolution=resolution, image_folder=image_folder,
                  batch_size=cfg.batch_size, world_size=run.world_size, rank=run.rank, num_classes=num_classes,
                  synthetic_length=synthetic_length, num_workers=num_workers)
    train_loader = make_dataloader(training=True, auto_augment=auto_augment, **common)
    val_loader = make_dataloader(training=False, **common)
    if str(dataset_name).lower() in UINT8_DATASETS:
        # uint8 images cross PCIe; resample, normalisation, flip and erasing run on the device, one batch ahead of the forward
        train_loader, val_loader = ImagePrefetcher(train_loader, device), ImagePrefetcher(val_loader, device)
    ipe = len(train_loader)
    logger.info(f'Dataloader created... iterations per epoch: {ipe}')

    if multihead is not None:
        return run_multihead(hps=multihead, init_opt=init_opt, features=_image_features, encoder=encoder,
                             train_loader=train_loader, val_loader=val_loader, num_classes=num_classes,
                             num_epochs=cfg.num_epochs, use_bfloat16=cfg.use_bfloat16, folder=run.folder, tag=cfg.tag,
                             rank=run.rank, world_size=run.world_size, batch_size=cfg.batch_size,
                             resume_checkpoint=cfg.resume_checkpoint, distributed=_distributed(), device=device)

    # -- optimizer and scheduler
    opt = init_opt(classifier=classifier, wd=cfg.wd, start_lr=cfg.start_lr, ref_lr=cfg.lr, final_lr=cfg.final_lr,
                   iterations_per_epoch=ipe, warmup=cfg.warmup, num_epochs=cfg.num_epochs, use_bfloat16=cfg.use_bfloat16)

    def train_epoch(**probe):
        return run_one_epoch(device=device, training=True, encoder=encoder, data_loader=train_loader,
                             use_bfloat16=cfg.use_bfloat16, **probe, **tune)

    def val_epoch(**probe):
        return run_one_epoch(device=device, training=False, encoder=encoder, data_loader=val_loader,
                             use_bfloat16=cfg.use_bfloat16, **probe)

    return train_single_probe(cfg, run, classifier, opt, ipe, train_epoch, val_epoch, **extra)


def frozen_features(encoder, imgs):
    """encoder(imgs) in calls small enough that the widest activation of one call (token rows x fc1's width) stays below 2^31
    elements.  The rows are counted from the tokens THIS input makes -- the model's num_patches describes its native size only --
    and the calls' outputs are joined by the bit-exact row copy."""
    cap = images_per_call(encoder, imgs)
    return encoder(imgs) if cap is None else chunked_call(encoder, imgs, cap)


def images_per_call(encoder, imgs):
    """The images of `imgs` one encoder call may hold (frozen_features), None for an encoder that does not describe its grid."""
    if not (hasattr(encoder, 'patch_size') and hasattr(encoder, 'tubelet_size') and hasattr(encoder, 'num_frames')):
        return None
    frames = encoder.num_frames if imgs.dim() == 4 else imgs.shape[2]
    depth = frames // encoder.tubelet_size if getattr(encoder, 'is_video', True) else 1     # the image model has no tubelets
    tokens = depth * (imgs.shape[-2] // encoder.patch_size) * (imgs.shape[-1] // encoder.patch_size)
    return max_clips_per_call(widest_activation(encoder), max(tokens, 1))


def trainable_features(encoder, imgs):
    """encoder(imgs) with a backward recorded: ONE encoder call for the batch (a second call would overwrite the gradient slots the
    first one's backward writes)."""
    cap = images_per_call(encoder, imgs)
    if cap is not None and imgs.shape[0] > cap:
        raise ValueError(f"{imgs.shape[0]} images with gradients enabled need one encoder call, and one call takes at most "
                         f"max_clips_per_call = {cap} images of this size (fc1's output stays below 2^31 elements); use a smaller batch")
    return encoder(imgs)


def _image_features(encoder, data, device):
    """One batch for the probe bank: the frozen features as a one-view list of [B, N, D], and the labels."""
    return [frozen_features(encoder, data[0].to(device, non_blocking=True))], data[1].to(device)


def run_one_epoch(device, training, encoder, classifier, scaler, optimizer, scheduler, wd_scheduler, data_loader, use_bfloat16,
                  *, history=None, features_grad=False, after_update=None, mix=None):
    """The reference's epoch (eval.py:262-317), same parameters in the same order.  history (keyword-only, optional list):
    (learning rate, loss) of each training iteration.  features_grad / after_update (keyword-only, off by default): the
    fine-tuning eval's encoder gradients and encoder step, see frozen.run_probe_epoch; the batch then goes through one encoder call
    (trainable_features).  mix (keyword-only, a ..mix.MixDraw or None): training iterations mix the batch with its flipped self in
    place (mixup / cutmix: vj_clip_mix on the images viewed as one-frame clips, three planes per image) and take the soft-target
    cross-entropy with label smoothing (vj_soft_ce) instead of the hard one; the training top-1 is still counted against each
    image's own label.  Validation ignores `mix`."""
    criterion = torch.nn.CrossEntropyLoss()
    mix = mix if training else None
    encode = trainable_features if training and features_grad else frozen_features

    def features(data):
        imgs, labels = data[0].to(device, non_blocking=True), data[1].to(device)
        if mix is not None:
            if imgs.shape[-1] % 4:
                raise ValueError(f"mix: images of width {imgs.shape[-1]}: vj_clip_mix moves four pixels at a time, the width must be "
                                 "a multiple of 4")
            tables = mix_batch(mix, [[imgs.unsqueeze(2)]], data[1], device)     # (labels, labels.flip(0), lam), validated on the host
            return encode(encoder, imgs), (labels, tables)
        return encode(encoder, imgs), labels

    def loss_and_top1(outputs, labels):
        # the prediction is the arg-max of the logits
        outputs = classifier(outputs)
        if mix is not None:
            labels, tables = labels
            loss, _ = SoftTargetCrossEntropy.apply(outputs, *tables, mix.label_smoothing, False)
        else:
            loss = criterion(outputs, labels)
        with torch.no_grad():
            return loss, 100. * outputs.max(dim=1).indices.eq(labels).sum() / len(labels)

    return run_probe_epoch(training, classifier, scaler, optimizer, scheduler, wd_scheduler, data_loader, use_bfloat16, features,
                           loss_and_top1, history=history, features_grad=features_grad, after_update=after_update)


def make_dataloader(dataset_name, root_path, image_folder, batch_size, world_size, rank, resolution=224, training=False,
                    subset_file=None, num_classes=None, synthetic_length=None, num_workers=0, seed=None, auto_augment=None):
    """The reference's loader factory (eval.py:379-423) for
        `dataset_name: synthetic`          finished fp32 images (SyntheticImageClassification);
        `dataset_name: synthetic_images`   seeded uint8 images of mixed sizes through the eval's transform (SyntheticImages);
        `dataset_name: image_folder`       <root_path>/<image_folder>/{train,val}/<class>/<file>, read with PIL, through the transform.
    The last two yield `(RawImageBatch, labels)` for engine.input.ImagePrefetcher: the reference's transforms (random-resized crop
    bicubic, flip, RandomErasing 0.25 to train; Resize bilinear + CenterCrop to validate) are drawn on the host and carried out on
    the device (.transforms).  The reference's own dataset names raise, as data_manager.init_data does.  auto_augment (extension,
    `data.auto_augment`): the training transform of the uint8 datasets also draws timm's policy plan per image."""
    kind = str(dataset_name).lower()
    if kind not in ('synthetic',) + UINT8_DATASETS:
        raise NotImplementedError(
            f"dataset_name={dataset_name!r}: the reference's ImageNet, iNat21 and Places205 dataset classes (their index files and "
            "subset_file) are not part of this package; a directory of <split>/<class>/<file> images runs with "
            "data.dataset_name: image_folder, seeded data with synthetic_images or synthetic, or pass your own loader to "
            "run_one_epoch")
    auto_augment = parse_auto_augment(dict(dataset_name=kind, auto_augment=auto_augment)) if training else None
    if kind in UINT8_DATASETS and training:
        global _auto_augment_logged
        if auto_augment is not None:
            logger.info(f"probe training: timm's auto_augment={auto_augment!r} (the reference asks for 'original', eval.py:392-403) is "
                        "applied on the device (data.auto_augment), between the flip and the normalisation")
        elif not _auto_augment_logged:
            _auto_augment_logged = True
            logger.info("probe training: the reference's auto_augment='original' policy (eval.py:392-403) is NOT applied; the random "
                        "resized crop, flip and RandomErasing (re_prob 0.25) are (data.auto_augment: original applies it on the "
                        "device)")
    if kind == 'image_folder':
        if subset_file is not None:
            raise NotImplementedError("image_folder: the reference's subset_file is not implemented")
        if root_path is None or image_folder is None:
            raise ValueError("make_dataloader(dataset_name='image_folder') needs root_path and image_folder")
        transform = make_transforms(training=training, resolution=resolution, auto_augment=auto_augment)
        dataset = ImageFolder(os.path.join(root_path, image_folder, 'train' if training else 'val'), transform=transform)
        sampler = torch.utils.data.distributed.DistributedSampler(dataset, num_replicas=world_size, rank=rank, shuffle=training)
        return torch.utils.data.DataLoader(dataset, sampler=sampler, batch_size=batch_size, drop_last=False, num_workers=num_workers,
                                           pin_memory=True, persistent_workers=False)
    if num_classes is None:
        raise ValueError(f"make_dataloader(dataset_name={kind!r}) needs num_classes")
    if kind == 'synthetic_images':
        transform = make_transforms(training=training, resolution=resolution, auto_augment=auto_augment)

        def make_dataset(length, seed):
            return SyntheticImages(length, num_classes, resolution, transform, seed=seed)
    else:
        def make_dataset(length, seed):
            return SyntheticImageClassification(length, num_classes, resolution, seed=seed)

    return synthetic_dataloader(make_dataset, batch_size, world_size, rank, training, num_workers, synthetic_length, seed)
