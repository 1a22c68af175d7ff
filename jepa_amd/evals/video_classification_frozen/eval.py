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
    per split, default 8 batches) and `data.num_workers` (default 0).
  - uint8 frames are what crosses to the device: the transforms only draw, the views are made by vj_clip_transform_pre and
    vj_clip_erase on a copy stream, and batch k+1 uploads while batch k's frozen forward runs (engine.input.EvalPrefetcher).
    `auto_augment` stays false where the reference's probe training sets it true; its RandAugment is opt-in instead: with the
    extension key `data.rand_augment: true` (default false; `synthetic_frames` only) the training transform draws the reference's
    plan per clip and vj_clip_randaug applies it to the uint8 frames on the device, byte for byte what PIL gives.  The short-side
    resize of the validation transforms is the loader's job (the synthetic frames have that short side).
  - the classifier is wrapped in DistributedDataParallel only when a process group with more than one rank is active; its
    checkpoint keys carry the `module.` prefix either way, so checkpoints move between this package and the reference.
  - with `pretrain.frames_per_clip` == 1 the encoder is the 2-D image ViT under FrameAggregation, which (as in the reference) only
    has the concatenated form: `optimization.attend_across_segments` must be true.
  - `main` returns a small record of the run (per-epoch accuracies, per-iteration training loss and learning rate).
  - `optimization.multihead_kwargs` (optional list of dictionaries overriding lr / start_lr / final_lr / weight_decay / warmup)
    trains one probe per entry on the same frozen forward pass (..multihead); without the key nothing changes.
"""
import os
import pprint
from functools import partial

import numpy as np
import torch
import torch.nn.functional as F
from torch.nn.parallel import DistributedDataParallel

from ...app.vjepa.randaugment import RandAugmentDraw
from ...engine.input import EvalPrefetcher
from ...src.datasets.data_manager import SyntheticFramesClassification, SyntheticVideoClassification
from ...src.models import vision_transformer as vit
from ...src.models.attentive_pooler import AttentiveClassifier
from ...src.utils.distributed import AllReduce, init_distributed
from ...src.utils.logging import AverageMeter, CSVLogger, get_logger
from ...src.utils.schedulers import CosineWDSchedule, WarmupCosineSchedule
from ..multihead import parse_multihead_kwargs
from ..multihead import run as run_multihead
from .utils import ClipAggregation, FrameAggregation, make_transforms

logger = get_logger(__name__)

_GLOBAL_SEED = 0
np.random.seed(_GLOBAL_SEED)
torch.manual_seed(_GLOBAL_SEED)

pp = pprint.PrettyPrinter(indent=4)

_randaugment_logged = False


def _distributed():
    import torch.distributed as dist
    return dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1


def main(args_eval, resume_preempt=False):
    # -- PRETRAIN
    args_pretrain = args_eval.get('pretrain')
    checkpoint_key = args_pretrain.get('checkpoint_key', 'target_encoder')
    model_name = args_pretrain.get('model_name', None)
    patch_size = args_pretrain.get('patch_size', None)
    pretrain_folder = args_pretrain.get('folder', None)
    ckp_fname = args_pretrain.get('checkpoint', None)
    tag = args_pretrain.get('write_tag', None)
    use_sdpa = args_pretrain.get('use_sdpa', True)
    use_SiLU = args_pretrain.get('use_silu', False)
    tight_SiLU = args_pretrain.get('tight_silu', True)
    uniform_power = args_pretrain.get('uniform_power', False)
    pretrained_path = os.path.join(pretrain_folder, ckp_fname)
    tubelet_size = args_pretrain.get('tubelet_size', 2)
    pretrain_frames_per_clip = args_pretrain.get('frames_per_clip', 1)

    # -- DATA
    args_data = args_eval.get('data')
    train_data_path = [args_data.get('dataset_train')]
    val_data_path = [args_data.get('dataset_val')]
    dataset_type = args_data.get('dataset_type', 'VideoDataset')
    num_classes = args_data.get('num_classes')
    eval_num_segments = args_data.get('num_segments', 1)
    eval_frames_per_clip = args_data.get('frames_per_clip', 16)
    eval_frame_step = args_pretrain.get('frame_step', 4)
    eval_duration = args_pretrain.get('clip_duration', None)
    eval_num_views_per_segment = args_data.get('num_views_per_segment', 1)
    synthetic_length = args_data.get('synthetic_length', None)
    num_workers = args_data.get('num_workers', 0)
    rand_augment = bool(args_data.get('rand_augment', False))

    # -- OPTIMIZATION
    args_opt = args_eval.get('optimization')
    resolution = args_opt.get('resolution', 224)
    batch_size = args_opt.get('batch_size')
    attend_across_segments = args_opt.get('attend_across_segments', False)
    num_epochs = args_opt.get('num_epochs')
    wd = args_opt.get('weight_decay')
    start_lr = args_opt.get('start_lr')
    lr = args_opt.get('lr')
    final_lr = args_opt.get('final_lr')
    warmup = args_opt.get('warmup')
    use_bfloat16 = args_opt.get('use_bfloat16')
    multihead = parse_multihead_kwargs(args_opt)   # None: the single probe below; a list: one bank of probes (..multihead)

    # -- EXPERIMENT-ID/TAG (optional)
    resume_checkpoint = args_eval.get('resume_checkpoint', False) or resume_preempt
    eval_tag = args_eval.get('tag', None)

    if pretrain_frames_per_clip == 1 and not attend_across_segments:
        raise ValueError("pretrain.frames_per_clip == 1 needs optimization.attend_across_segments: true: the reference's frame "
                         "aggregation only has the concatenated form (one [B, S*T*N, D] tensor per view), and the epoch loop of "
                         "attend_across_segments: false would iterate over the batch dimension of those tensors")

    if not torch.cuda.is_available():
        raise RuntimeError("the frozen eval computes on the GPU through libvjepa_hip.so (there is no CPU path)")
    device = torch.device('cuda:0')
    torch.cuda.set_device(device)

    world_size, rank = init_distributed()
    logger.info(f'Initialized (rank/world-size) {rank}/{world_size}')

    # -- log/checkpointing paths
    folder = os.path.join(pretrain_folder, 'video_classification_frozen/')
    if eval_tag is not None:
        folder = os.path.join(folder, eval_tag)
    os.makedirs(folder, exist_ok=True)
    log_file = os.path.join(folder, f'{tag}_r{rank}.csv')
    latest_path = os.path.join(folder, f'{tag}-latest.pth.tar')

    if rank == 0 and multihead is None:
        csv_logger = CSVLogger(log_file, ('%d', 'epoch'), ('%.5f', 'loss'), ('%.5f', 'acc'))

    # -- pretrained encoder (frozen)
    encoder = init_model(crop_size=resolution, device=device, pretrained=pretrained_path, model_name=model_name,
                         patch_size=patch_size, tubelet_size=tubelet_size, frames_per_clip=pretrain_frames_per_clip,
                         uniform_power=uniform_power, checkpoint_key=checkpoint_key, use_SiLU=use_SiLU, tight_SiLU=tight_SiLU,
                         use_sdpa=use_sdpa)
    if pretrain_frames_per_clip == 1:
        encoder = FrameAggregation(encoder).to(device)
    else:
        encoder = ClipAggregation(encoder, tubelet_size=tubelet_size, attend_across_segments=attend_across_segments).to(device)
    encoder.eval()
    for p in encoder.parameters():
        p.requires_grad = False

    # -- init classifier
    if multihead is None:
        classifier = AttentiveClassifier(embed_dim=encoder.embed_dim, num_heads=encoder.num_heads, depth=1,
                                         num_classes=num_classes).to(device)

    common = dict(dataset_type=dataset_type, resolution=resolution, frames_per_clip=eval_frames_per_clip,
                  frame_step=eval_frame_step, eval_duration=eval_duration, allow_segment_overlap=True, batch_size=batch_size,
                  world_size=world_size, rank=rank, num_classes=num_classes, synthetic_length=synthetic_length,
                  num_workers=num_workers)
    train_loader = make_dataloader(root_path=train_data_path, num_segments=eval_num_segments if attend_across_segments else 1,
                                   num_views_per_segment=1, training=True, rand_augment=rand_augment, **common)
    val_loader = make_dataloader(root_path=val_data_path, num_segments=eval_num_segments,
                                 num_views_per_segment=eval_num_views_per_segment, training=False, **common)
    if str(dataset_type).lower() == 'synthetic_frames':
        # uint8 frames: the views are made on the device, and the upload of batch k+1 runs under batch k's frozen forward
        train_loader, val_loader = EvalPrefetcher(train_loader, device), EvalPrefetcher(val_loader, device)
    ipe = len(train_loader)
    logger.info(f'Dataloader created... iterations per epoch: {ipe}')

    if multihead is not None:
        return run_multihead(hps=multihead, init_opt=init_opt, features=partial(_view_features, attend_across_segments),
                             encoder=encoder, train_loader=train_loader, val_loader=val_loader, num_classes=num_classes,
                             num_epochs=num_epochs, use_bfloat16=use_bfloat16, folder=folder, tag=tag, rank=rank,
                             world_size=world_size, batch_size=batch_size, resume_checkpoint=resume_checkpoint,
                             distributed=_distributed(), device=device)

    # -- optimizer and scheduler
    optimizer, scaler, scheduler, wd_scheduler = init_opt(classifier=classifier, wd=wd, start_lr=start_lr, ref_lr=lr,
                                                          final_lr=final_lr, iterations_per_epoch=ipe, warmup=warmup,
                                                          num_epochs=num_epochs, use_bfloat16=use_bfloat16)
    if _distributed():
        classifier = DistributedDataParallel(classifier, static_graph=True)

    # -- load training checkpoint
    start_epoch = 0
    if resume_checkpoint:
        classifier, optimizer, scaler, start_epoch = load_checkpoint(device=device, r_path=latest_path, classifier=classifier,
                                                                     opt=optimizer, scaler=scaler)
        for _ in range(start_epoch * ipe):
            scheduler.step()
            wd_scheduler.step()

    def save_checkpoint(epoch):
        save_dict = {
            'classifier': classifier_state_dict(classifier),
            'opt': optimizer.state_dict(),
            'scaler': None if scaler is None else scaler.state_dict(),
            'epoch': epoch,
            'batch_size': batch_size,
            'world_size': world_size,
            'lr': lr
        }
        if rank == 0:
            torch.save(save_dict, latest_path)

    record = dict(start_epoch=start_epoch, train_acc=[], val_acc=[], train_history=[])
    for epoch in range(start_epoch, num_epochs):
        logger.info('Epoch %d' % (epoch + 1))
        train_acc = run_one_epoch(device=device, training=True,
                                  num_temporal_views=eval_num_segments if attend_across_segments else 1,
                                  attend_across_segments=attend_across_segments, num_spatial_views=1, encoder=encoder,
                                  classifier=classifier, scaler=scaler, optimizer=optimizer, scheduler=scheduler,
                                  wd_scheduler=wd_scheduler, data_loader=train_loader, use_bfloat16=use_bfloat16,
                                  history=record['train_history'])
        val_acc = run_one_epoch(device=device, training=False, num_temporal_views=eval_num_segments,
                                attend_across_segments=attend_across_segments, num_spatial_views=eval_num_views_per_segment,
                                encoder=encoder, classifier=classifier, scaler=scaler, optimizer=optimizer, scheduler=scheduler,
                                wd_scheduler=wd_scheduler, data_loader=val_loader, use_bfloat16=use_bfloat16)
        logger.info('[%5d] train: %.3f%% test: %.3f%%' % (epoch + 1, train_acc, val_acc))
        if rank == 0:
            csv_logger.log(epoch + 1, train_acc, val_acc)
        save_checkpoint(epoch + 1)
        record['train_acc'].append(train_acc)
        record['val_acc'].append(val_acc)
    return record


def _view_features(attend_across_segments, encoder, data, device):
    """One batch for the probe bank: the frozen features of every view as a flat list of [B, N, D] tensors, and the labels."""
    clips = [[dij.to(device, non_blocking=True) for dij in di] for di in data[0]]
    clip_indices = [d.to(device, non_blocking=True) for d in data[2]]
    outputs = encoder(clips, clip_indices)
    return (outputs if attend_across_segments else [ost for os_ in outputs for ost in os_]), data[1].to(device)


def run_one_epoch(device, training, encoder, classifier, scaler, optimizer, scheduler, wd_scheduler, data_loader, use_bfloat16,
                  num_spatial_views, num_temporal_views, attend_across_segments, *, history=None):
    """The reference's epoch (eval.py:298-380), same parameters in the same order.  history (keyword-only, optional list):
    (learning rate, loss) of each training iteration."""
    classifier.train(mode=training)
    criterion = torch.nn.CrossEntropyLoss()
    top1_meter = AverageMeter()
    for itr, data in enumerate(data_loader):

        if training:
            scheduler.step()
            wd_scheduler.step()

        # Load data and put on GPU
        clips = [[dij.to(device, non_blocking=True) for dij in di] for di in data[0]]
        clip_indices = [d.to(device, non_blocking=True) for d in data[2]]
        labels = data[1].to(device)
        batch_size = len(labels)

        # Forward and prediction
        with torch.no_grad():
            outputs = encoder(clips, clip_indices)
            if not training:
                if attend_across_segments:
                    outputs = [classifier(o) for o in outputs]
                else:
                    outputs = [[classifier(ost) for ost in os] for os in outputs]
        if training:
            if attend_across_segments:
                outputs = [classifier(o) for o in outputs]
            else:
                outputs = [[classifier(ost) for ost in os] for os in outputs]

        # Compute loss
        if attend_across_segments:
            loss = sum([criterion(o, labels) for o in outputs]) / len(outputs)
        else:
            loss = sum([sum([criterion(ost, labels) for ost in os]) for os in outputs]) / len(outputs) / len(outputs[0])
        with torch.no_grad():
            if attend_across_segments:
                outputs = sum([F.softmax(o, dim=1) for o in outputs]) / len(outputs)
            else:
                outputs = sum([sum([F.softmax(ost, dim=1) for ost in os]) for os in outputs]) / len(outputs) / len(outputs[0])
            top1_acc = 100. * outputs.max(dim=1).indices.eq(labels).sum() / batch_size
            top1_acc = float(AllReduce.apply(top1_acc))
            top1_meter.update(top1_acc)

        if training:
            if use_bfloat16:
                scaler.scale(loss).backward()
                scaler.unscale_(optimizer)
                torch.nn.utils.clip_grad_norm_(classifier.parameters(), 1.0)
                scaler.step(optimizer)
                scaler.update()
            else:
                loss.backward()
                torch.nn.utils.clip_grad_norm_(classifier.parameters(), 1.0)
                optimizer.step()
            optimizer.zero_grad()
            if history is not None:
                history.append((optimizer.param_groups[0]['lr'], float(loss.detach())))

        if itr % 20 == 0:
            logger.info('[%5d] %.3f%% (loss: %.3f) [mem: %.2e]'
                        % (itr, top1_meter.avg, float(loss.detach()), torch.cuda.max_memory_allocated() / 1024.**2))

    return top1_meter.avg


def classifier_state_dict(classifier):
    """The classifier's state dict with the `module.` prefix the reference's DDP-wrapped classifier writes."""
    sd = classifier.state_dict()
    if isinstance(classifier, DistributedDataParallel):
        return sd
    return {'module.' + k: v for k, v in sd.items()}


def load_checkpoint(device, r_path, classifier, opt, scaler):
    try:
        checkpoint = torch.load(r_path, map_location=torch.device('cpu'))
        epoch = checkpoint['epoch']

        # -- loading classifier (`module.`-prefixed keys, as the reference writes them)
        pretrained_dict = checkpoint['classifier']
        if not isinstance(classifier, DistributedDataParallel):
            pretrained_dict = {(k[len('module.'):] if k.startswith('module.') else k): v for k, v in pretrained_dict.items()}
        msg = classifier.load_state_dict(pretrained_dict)
        logger.info(f'loaded pretrained classifier from epoch {epoch} with msg: {msg}')

        # -- loading optimizer
        opt.load_state_dict(checkpoint['opt'])
        if scaler is not None:
            scaler.load_state_dict(checkpoint['scaler'])
        logger.info(f'loaded optimizers from epoch {epoch}')
        logger.info(f'read-path: {r_path}')
        del checkpoint

    except Exception as e:
        logger.info(f'Encountered exception when loading checkpoint {e}')
        epoch = 0

    return classifier, opt, scaler, epoch


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
    if kind not in ('synthetic', 'synthetic_frames'):
        raise NotImplementedError(
            f"dataset_type={dataset_type!r}: the reference's decord/torchvision video pipeline is not part of this package; "
            "use data.dataset_type: synthetic or synthetic_frames, or pass your own loader to run_one_epoch")
    if num_classes is None:
        raise ValueError(f"make_dataloader(dataset_type={kind!r}) needs num_classes")
    if rand_augment and kind != 'synthetic_frames':
        raise ValueError(f"data.rand_augment needs uint8 frames (dataset_type: synthetic_frames); {kind!r} yields finished fp32 views")
    length = synthetic_length if synthetic_length is not None else 8 * batch_size * world_size
    seed = (0 if training else 1) if seed is None else seed
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
        dataset = SyntheticFramesClassification(length, num_classes, frames_per_clip, resolution, transform,
                                                num_segments=num_segments, short_side=short, frame_step=frame_step, seed=seed)
    else:
        dataset = SyntheticVideoClassification(length, num_classes, frames_per_clip, resolution, num_segments=num_segments,
                                               num_views_per_segment=num_views_per_segment, frame_step=frame_step, seed=seed)
    sampler = torch.utils.data.distributed.DistributedSampler(dataset, num_replicas=world_size, rank=rank, shuffle=training)
    return torch.utils.data.DataLoader(dataset, sampler=sampler, batch_size=batch_size, drop_last=False,
                                       num_workers=num_workers, pin_memory=True, persistent_workers=False)


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
