"""Frozen video-classification eval with the reference's entry point and YAML schema
(evals/video_classification_frozen/eval.py:67-561):

    from jepa_amd.evals.video_classification_frozen.eval import main
    main(args_eval_dict_from_yaml, resume_preempt=False)

Same config keys, probe (AttentiveClassifier on ClipAggregation features), optimizer groups, schedules, loss and accuracy
arithmetic, CSV columns, checkpoint dictionary and folder / file names.  Differences from the reference:
  - the frozen encoder and the probe compute in bf16 with fp32 accumulation and statistics on the HIP kernels of this package;
    the reference's fp16 autocast (eval.py:323) would do nothing to these modules and is not entered.  `use_bfloat16` still
    selects the GradScaler path of the update, as in the reference.
  - there are no real video datasets: `data.dataset_type` must be `synthetic` (seeded labelled fp32 views,
    src/datasets/data_manager.py: SyntheticVideoClassification) or `synthetic_frames` (seeded labelled uint8 frames of mixed source
    sizes, SyntheticFramesClassification, through the eval's own transforms: .utils make_transforms with the reference's
    reprob 0.25 for training and its centre-crop / multi-view forms for validation); extension keys `data.synthetic_length` (items
    per split, default 8 batches) and `data.num_workers` (default 0).  Real videos come as frames: `data.dataset_type: frame_folder`
    reads `dataset_train` / `dataset_val` as the reference's index csv over folders of frame images or .npy frame arrays
    (src/datasets/frame_folder.py: the reference's clip sampling, no video decoder) through the same transforms and input edge;
    its validation frames may have any size (see below).  `VideoDataset` and the other reference names still raise.
  - uint8 frames are what crosses to the device: the transforms only draw, the views are made by vj_clip_transform_pre and
    vj_clip_erase on a copy stream, and batch k+1 uploads while batch k's frozen forward runs (engine.input.EvalPrefetcher).
    `auto_augment` stays false where the reference's probe training sets it true; its RandAugment is opt-in instead: with the
    extension key `data.rand_augment: true` (default false; `synthetic_frames` only) the training transform draws the reference's
    plan per clip and vj_clip_randaug applies it to the uint8 frames on the device, byte for byte what PIL gives.  The short-side
    resize of the validation transforms is done on the device for `frame_folder` (vj_clip_resample: PIL's antialiased bilinear
    Image.resize, not the cv2.INTER_LINEAR the reference's decord frames get); the synthetic frames have that short side.
  - the classifier is wrapped in DistributedDataParallel only when a process group with more than one rank is active; its
    checkpoint keys carry the `module.` prefix either way, so checkpoints move between this package and the reference.
  - with `pretrain.frames_per_clip` == 1 the encoder is the 2-D image ViT under FrameAggregation, which (as in the reference) only
    has the concatenated form: `optimization.attend_across_segments` must be true.
  - `main` returns a small record of the run (per-epoch accuracies, per-iteration training loss and learning rate).
  - `optimization.multihead_kwargs` (optional list of dictionaries overriding lr / start_lr / final_lr / weight_decay / warmup)
    trains one probe per entry on the same frozen forward pass (..multihead); without the key nothing changes.
"""
import pprint
from functools import partial

import numpy as np
import torch
import torch.nn.functional as F

from ...app.vjepa.randaugment import RandAugmentDraw
from ...engine.input import EvalPrefetcher
from ...src.datasets.data_manager import SyntheticFramesClassification, SyntheticVideoClassification, init_data
from ...src.models import vision_transformer as vit
from ...src.models.attentive_pooler import AttentiveClassifier
from ...src.utils.logging import get_logger
from ...src.utils.schedulers import CosineWDSchedule, WarmupCosineSchedule
from ..frozen import classifier_state_dict, load_checkpoint  # noqa: F401  (the reference's names in this file)
from ..frozen import distributed as _distributed
from ..frozen import freeze, parse_config, run_probe_epoch, setup_run, synthetic_dataloader, train_single_probe
from ..mix import SoftTargetCrossEntropy, mix_batch
from ..multihead import run as run_multihead
from .utils import ClipAggregation, FrameAggregation, make_transforms

logger = get_logger(__name__)

_GLOBAL_SEED = 0
np.random.seed(_GLOBAL_SEED)
torch.manual_seed(_GLOBAL_SEED)

pp = pprint.PrettyPrinter(indent=4)

_randaugment_logged = False


def main(args_eval, resume_preempt=False, finetune=None):
    """finetune (extension): None (the frozen eval), or what ..video_classification_finetune.eval brings to train the encoder
    with the probe on this eval's data, probe, schedules and checkpoints: `folder_name`; check(cfg), called before anything is
    set up; attach(cfg, run, encoder) -> (epoch keywords of the training run_one_epoch, extra_state, restore_extra of
    frozen.train_single_probe), called on the ClipAggregation instead of freezing it."""
    cfg = parse_config(args_eval, resume_preempt)
    multihead = cfg.multihead
    if finetune is not None:
        finetune.check(cfg)
    args_pretrain, args_opt = cfg.args_pretrain, cfg.args_opt

    # -- DATA
    args_data = args_eval.get('data')
    train_data_path = [args_data.get('dataset_train')]
    val_data_path = [args_data.get('dataset_val')]
    dataset_type = args_data.get('dataset_type', 'VideoDataset')
    num_classes = cfg.num_classes = args_data.get('num_classes')
    eval_num_segments = args_data.get('num_segments', 1)
    eval_frames_per_clip = args_data.get('frames_per_clip', 16)
    eval_frame_step = args_pretrain.get('frame_step', 4)
    eval_duration = args_pretrain.get('clip_duration', None)
    eval_num_views_per_segment = args_data.get('num_views_per_segment', 1)
    synthetic_length = args_data.get('synthetic_length', None)
    num_workers = args_data.get('num_workers', 0)
    rand_augment = bool(args_data.get('rand_augment', False))

    # -- OPTIMIZATION (the video eval's own keys)
    resolution = args_opt.get('resolution', 224)
    attend_across_segments = args_opt.get('attend_across_segments', False)

    if cfg.frames_per_clip == 1 and not attend_across_segments:
        raise ValueError("pretrain.frames_per_clip == 1 needs optimization.attend_across_segments: true: the reference's frame "
                         "aggregation only has the concatenated form (one [B, S*T*N, D] tensor per view), and the epoch loop of "
                         "attend_across_segments: false would iterate over the batch dimension of those tensors")

    run = setup_run(cfg, 'video_classification_frozen/' if finetune is None else finetune.folder_name, csv=multihead is None)
    device = run.device

    # -- pretrained encoder (frozen)
    encoder = init_model(crop_size=resolution, device=device, pretrained=cfg.pretrained_path, model_name=cfg.model_name,
                         patch_size=cfg.patch_size, tubelet_size=cfg.tubelet_size, frames_per_clip=cfg.frames_per_clip,
                         uniform_power=cfg.uniform_power, checkpoint_key=cfg.checkpoint_key, use_SiLU=cfg.use_SiLU,
                         tight_SiLU=cfg.tight_SiLU, use_sdpa=cfg.use_sdpa)
    if cfg.frames_per_clip == 1:
        encoder = FrameAggregation(encoder).to(device)
    else:
        encoder = ClipAggregation(encoder, tubelet_size=cfg.tubelet_size,
                                  attend_across_segments=attend_across_segments).to(device)
    tune, extra = {}, {}
    if finetune is None:
        freeze(encoder)
    else:
        tune, extra['extra_state'], extra['restore_extra'] = finetune.attach(cfg, run, encoder)

    # -- init classifier
    if multihead is None:
        classifier = AttentiveClassifier(embed_dim=encoder.embed_dim, num_heads=encoder.num_heads, depth=1,
                                         num_classes=num_classes).to(device)

    common = dict(dataset_type=dataset_type, resolution=resolution, frames_per_clip=eval_frames_per_clip,
                  frame_step=eval_frame_step, eval_duration=eval_duration, allow_segment_overlap=True,
                  batch_size=cfg.batch_size, world_size=run.world_size, rank=run.rank, num_classes=num_classes,
                  synthetic_length=synthetic_length, num_workers=num_workers)
    train_loader = make_dataloader(root_path=train_data_path, num_segments=eval_num_segments if attend_across_segments else 1,
                                   num_views_per_segment=1, training=True, rand_augment=rand_augment, **common)
    val_loader = make_dataloader(root_path=val_data_path, num_segments=eval_num_segments,
                                 num_views_per_segment=eval_num_views_per_segment, training=False, **common)
    if str(dataset_type).lower() in ('synthetic_frames', 'frame_folder'):
        # uint8 frames: the views are made on the device, and the upload of batch k+1 runs under batch k's frozen forward
        train_loader, val_loader = EvalPrefetcher(train_loader, device), EvalPrefetcher(val_loader, device)
    ipe = len(train_loader)
    logger.info(f'Dataloader created... iterations per epoch: {ipe}')

    if multihead is not None:
        return run_multihead(hps=multihead, init_opt=init_opt, features=partial(_view_features, attend_across_segments),
                             encoder=encoder, train_loader=train_loader, val_loader=val_loader, num_classes=num_classes,
                             num_epochs=cfg.num_epochs, use_bfloat16=cfg.use_bfloat16, folder=run.folder, tag=cfg.tag,
                             rank=run.rank, world_size=run.world_size, batch_size=cfg.batch_size,
                             resume_checkpoint=cfg.resume_checkpoint, distributed=_distributed(), device=device)

    # -- optimizer and scheduler
    opt = init_opt(classifier=classifier, wd=cfg.wd, start_lr=cfg.start_lr, ref_lr=cfg.lr, final_lr=cfg.final_lr,
                   iterations_per_epoch=ipe, warmup=cfg.warmup, num_epochs=cfg.num_epochs, use_bfloat16=cfg.use_bfloat16)
    epoch = dict(device=device, encoder=encoder, use_bfloat16=cfg.use_bfloat16, attend_across_segments=attend_across_segments)

    def train_epoch(**probe):
        return run_one_epoch(training=True, num_temporal_views=eval_num_segments if attend_across_segments else 1,
                             num_spatial_views=1, data_loader=train_loader, **epoch, **probe, **tune)

    def val_epoch(**probe):
        return run_one_epoch(training=False, num_temporal_views=eval_num_segments,
                             num_spatial_views=eval_num_views_per_segment, data_loader=val_loader, **epoch, **probe)

    return train_single_probe(cfg, run, classifier, opt, ipe, train_epoch, val_epoch, **extra)


def _view_features(attend_across_segments, encoder, data, device):
    """One batch for the probe bank: the frozen features of every view as a flat list of [B, N, D] tensors, and the labels."""
    clips = [[dij.to(device, non_blocking=True) for dij in di] for di in data[0]]
    clip_indices = [d.to(device, non_blocking=True) for d in data[2]]
    outputs = encoder(clips, clip_indices)
    return (outputs if attend_across_segments else [ost for os_ in outputs for ost in os_]), data[1].to(device)


def run_one_epoch(device, training, encoder, classifier, scaler, optimizer, scheduler, wd_scheduler, data_loader, use_bfloat16,
                  num_spatial_views, num_temporal_views, attend_across_segments, *, history=None, features_grad=False,
                  after_update=None, mix=None):
    """The reference's epoch (eval.py:298-380), same parameters in the same order.  history (keyword-only, optional list):
    (learning rate, loss) of each training iteration.  features_grad / after_update (keyword-only, off by default): the
    fine-tuning eval's encoder gradients and encoder step, see frozen.run_probe_epoch.  mix (keyword-only, a ..mix.MixDraw or
    None): training iterations mix the batch with its flipped self in place (mixup / cutmix, vj_clip_mix on every view with the
    batch's one plan; the tensors are the loader's device buffers or this function's own copies) and take the soft-target
    cross-entropy with label smoothing (vj_soft_ce) instead of the hard one.  The training top-1 is still counted against each
    clip's own label: under mixing it is a lower bound of what the model knows, since a mixed clip's partner label may be the
    right answer.  Validation ignores `mix`."""
    criterion = torch.nn.CrossEntropyLoss()
    mix = mix if training else None

    def features(data):
        # Load data and put on GPU
        clips = [[dij.to(device, non_blocking=True) for dij in di] for di in data[0]]
        clip_indices = [d.to(device, non_blocking=True) for d in data[2]]
        labels = data[1].to(device)
        if mix is not None:
            tables = mix_batch(mix, clips, data[1], device)     # (labels, labels.flip(0), lam), validated on the host
            return encoder(clips, clip_indices), (labels, tables)
        return encoder(clips, clip_indices), labels

    def soft_loss_and_top1(outputs, labels, tables):
        # the same arithmetic as below with the soft-target loss, whose kernel also gives the soft-max of each view
        views = outputs if attend_across_segments else [ost for ov in outputs for ost in ov]
        results = [SoftTargetCrossEntropy.apply(classifier(o), *tables, mix.label_smoothing, True) for o in views]
        loss = sum([ls for ls, _ in results]) / len(results)
        with torch.no_grad():
            probs = sum([p for _, p in results]) / len(results)
            return loss, 100. * probs.max(dim=1).indices.eq(labels).sum() / len(labels)

    def loss_and_top1(outputs, labels):
        if mix is not None:
            return soft_loss_and_top1(outputs, *labels)
        # the prediction is the arg-max of the soft-max averaged over every view
        if attend_across_segments:
            outputs = [classifier(o) for o in outputs]
            loss = sum([criterion(o, labels) for o in outputs]) / len(outputs)
            with torch.no_grad():
                probs = sum([F.softmax(o, dim=1) for o in outputs]) / len(outputs)
        else:
            outputs = [[classifier(ost) for ost in ov] for ov in outputs]
            loss = sum([sum([criterion(ost, labels) for ost in ov]) for ov in outputs]) / len(outputs) / len(outputs[0])
            with torch.no_grad():
                probs = sum([sum([F.softmax(ost, dim=1) for ost in ov]) for ov in outputs]) / len(outputs) / len(outputs[0])
        with torch.no_grad():
            return loss, 100. * probs.max(dim=1).indices.eq(labels).sum() / len(labels)

    return run_probe_epoch(training, classifier, scaler, optimizer, scheduler, wd_scheduler, data_loader, use_bfloat16, features,
                           loss_and_top1, history=history, features_grad=features_grad, after_update=after_update)


def load_pretrained(encoder, pretrained, checkpoint_key='target_encoder'):
    logger.info(f'Loading pretrained model from {pretrained}')
    checkpoint = torch.load(pretrained, map_location='cpu')
    try:
        pretrained_dict = checkpoint[checkpoint_key]
    except Exception:
        pretrained_dict = checkpoint['encoder']

    pretrained_dict = {k.replace('module.', ''): v for k, v in pretrained_dict.items()}
    pretrained_dict = {k.replace('backbone.', ''): v for k, v in pretrained_dict.items()}
    for k, v in encoder.state_dict().items():
        if k not in pretrained_dict:
            logger.info(f'key "{k}" could not be found in loaded state dict')
        elif pretrained_dict[k].shape != v.shape:
            logger.info(f'key "{k}" is of different shape in model and loaded state dict')
            pretrained_dict[k] = v
    msg = encoder.load_state_dict(pretrained_dict, strict=False)
    logger.info(f'loaded pretrained model with msg: {msg}')
    logger.info(f'loaded pretrained encoder from epoch: {checkpoint.get("epoch")}\n path: {pretrained}')
    del checkpoint
    return encoder


def make_dataloader(root_path, batch_size, world_size, rank, dataset_type='VideoDataset', resolution=224, frames_per_clip=16,
                    frame_step=4, num_segments=8, eval_duration=None, num_views_per_segment=1, allow_segment_overlap=True,
                    training=False, num_workers=12, subset_file=None, num_classes=None, synthetic_length=None, seed=None,
                    rand_augment=False):
    """The reference's loader factory (eval.py:442-488) for `dataset_type: synthetic` (finished fp32 views) and
    `synthetic_frames` (uint8 frames through the eval's transforms, with the reference's arguments: eval.py:460-469 -- batches of
    RawClipBatch, one per segment, for engine.input.EvalPrefetcher); every real dataset type raises, as data_manager.init_data
    does.  rand_augment (extension, `data.rand_augment`): the training transform of `synthetic_frames` also draws the reference's
    RandAugment plan per clip ('rand-m7-n4-mstd0.5-inc1', utils.py:233-237), which the prefetcher carries out on the device."""
    kind = str(dataset_type).lower()
    if kind == 'frame_folder':
        return _frame_folder_dataloader(root_path, batch_size, world_size, rank, resolution, frames_per_clip, frame_step,
                                        num_segments, eval_duration, num_views_per_segment, allow_segment_overlap, training,
                                        num_workers, subset_file, rand_augment)
    if kind not in ('synthetic', 'synthetic_frames'):
        raise NotImplementedError(
            f"dataset_type={dataset_type!r}: the reference's decord/torchvision video pipeline is not part of this package; "
            "use data.dataset_type: synthetic or synthetic_frames, or pass your own loader to run_one_epoch")
    if num_classes is None:
        raise ValueError(f"make_dataloader(dataset_type={kind!r}) needs num_classes")
    if rand_augment and kind != 'synthetic_frames':
        raise ValueError(f"data.rand_augment needs uint8 frames (dataset_type: synthetic_frames); {kind!r} yields finished fp32 views")
    if kind == 'synthetic_frames':
        global _randaugment_logged
        if training and rand_augment:
            logger.info("probe training: the reference's RandAugment (auto_augment=True, eval.py:465: rand-m7-n4-mstd0.5-inc1, "
                        "bicubic) is applied on the device (data.rand_augment), before the random resized crop and RandomErasing")
        elif training and not _randaugment_logged:
            _randaugment_logged = True
            logger.info("probe training: the reference's RandAugment (auto_augment=True, eval.py:465) is NOT applied -- it runs "
                        "through PIL on the CPU; the random resized crop and RandomErasing (reprob 0.25) are "
                        "(data.rand_augment: true applies it on the device)")
        transform = make_transforms(training=training, num_views_per_clip=num_views_per_segment, random_horizontal_flip=False,
                                    random_resize_aspect_ratio=(0.75, 4/3), random_resize_scale=(0.08, 1.0), reprob=0.25,
                                    auto_augment=False, motion_shift=False, crop_size=resolution)
        if training and rand_augment:
            transform.rand_augment = RandAugmentDraw('rand-m7-n4-mstd0.5-inc1')
        short = None if training else (resolution if num_views_per_segment > 1 else int(resolution * 256 / 224))

        def make_dataset(length, seed):
            return SyntheticFramesClassification(length, num_classes, frames_per_clip, resolution, transform,
                                                 num_segments=num_segments, short_side=short, frame_step=frame_step, seed=seed)
    else:
        def make_dataset(length, seed):
            return SyntheticVideoClassification(length, num_classes, frames_per_clip, resolution, num_segments=num_segments,
                                                num_views_per_segment=num_views_per_segment, frame_step=frame_step, seed=seed)
    return synthetic_dataloader(make_dataset, batch_size, world_size, rank, training, num_workers, synthetic_length, seed)


def _frame_folder_dataloader(root_path, batch_size, world_size, rank, resolution, frames_per_clip, frame_step, num_segments,
                             eval_duration, num_views_per_segment, allow_segment_overlap, training, num_workers, subset_file,
                             rand_augment):
    """`dataset_type: frame_folder`: real videos as folders of frames (src/datasets/frame_folder.py) through the eval's transforms
    and init_data with the reference's arguments (eval.py:460-487).  The validation transforms resize frames of any size to the
    reference's short side on the device (`device_resize`); the training transform takes any size as it is."""
    if subset_file is not None:
        raise NotImplementedError("dataset_type: frame_folder does not read a subset_file; write the subset as its own csv")
    transform = make_transforms(training=training, num_views_per_clip=num_views_per_segment, random_horizontal_flip=False,
                                random_resize_aspect_ratio=(0.75, 4/3), random_resize_scale=(0.08, 1.0), reprob=0.25,
                                auto_augment=False, motion_shift=False, crop_size=resolution)
    if training and rand_augment:
        transform.rand_augment = RandAugmentDraw('rand-m7-n4-mstd0.5-inc1')
    if not training:
        transform.device_resize = True
    data_loader, _ = init_data(data='frame_folder', root_path=root_path, transform=transform, batch_size=batch_size,
                               world_size=world_size, rank=rank, clip_len=frames_per_clip, frame_sample_rate=frame_step,
                               duration=eval_duration, num_clips=num_segments, allow_clip_overlap=allow_segment_overlap,
                               num_workers=num_workers, copy_data=False, drop_last=False, subset_file=subset_file)
    return data_loader


def init_model(device, pretrained, model_name, patch_size=16, crop_size=224, frames_per_clip=16, tubelet_size=2, use_sdpa=False,
               use_SiLU=False, tight_SiLU=True, uniform_power=False, checkpoint_key='target_encoder'):
    """vit.<model_name> with the pretrained weights (pretrained=None keeps the random initialisation)."""
    if use_SiLU:
        raise NotImplementedError("use_silu: the SiLU MLP variant is not implemented by the encoder kernels")
    encoder = vit.__dict__[model_name](img_size=crop_size, patch_size=patch_size, num_frames=frames_per_clip,
                                       tubelet_size=tubelet_size, uniform_power=uniform_power, use_sdpa=use_sdpa)
    encoder.to(device)
    if pretrained is not None:
        encoder = load_pretrained(encoder=encoder, pretrained=pretrained, checkpoint_key=checkpoint_key)
    return encoder


def init_opt(classifier, iterations_per_epoch, start_lr, ref_lr, warmup, num_epochs, wd=1e-6, final_wd=1e-6, final_lr=0.0,
             use_bfloat16=False):
    param_groups = [
        {
            'params': (p for n, p in classifier.named_parameters() if ('bias' not in n) and (len(p.shape) != 1))
        }, {
            'params': (p for n, p in classifier.named_parameters() if ('bias' in n) or (len(p.shape) == 1)),
            'WD_exclude': True,
            'weight_decay': 0
        }
    ]
    logger.info('Using AdamW')
    optimizer = torch.optim.AdamW(param_groups)
    scheduler = WarmupCosineSchedule(optimizer, warmup_steps=int(warmup * iterations_per_epoch), start_lr=start_lr,
                                     ref_lr=ref_lr, final_lr=final_lr, T_max=int(num_epochs * iterations_per_epoch))
    wd_scheduler = CosineWDSchedule(optimizer, ref_wd=wd, final_wd=final_wd, T_max=int(num_epochs * iterations_per_epoch))
    scaler = torch.amp.GradScaler('cuda') if use_bfloat16 else None
    return optimizer, scaler, scheduler, wd_scheduler
