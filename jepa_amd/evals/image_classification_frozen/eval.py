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
    (..video_classification_frozen.eval, whose load_checkpoint, load_pretrained, init_model and init_opt are these files' too).
  - there are no real image datasets: `data.dataset_name` must be `synthetic` (seeded labelled images,
    src/datasets/data_manager.py: SyntheticImageClassification); extension keys `data.synthetic_length` (items per split, default 8
    batches) and `data.num_workers` (default 0).
  - one encoder call never holds more images than keep fc1's output below 2^31 elements, counted from the tokens the actual input
    makes (frozen_features).
  - `main` returns a small record of the run (per-epoch accuracies, per-iteration training loss and learning rate).
"""
import os
import pprint

import numpy as np
import torch
from torch.nn.parallel import DistributedDataParallel

from ...hip import ops
from ...src.datasets.data_manager import SyntheticImageClassification
from ...src.models.attentive_pooler import AttentiveClassifier
from ...src.utils.distributed import AllReduce, init_distributed
from ...src.utils.logging import AverageMeter, CSVLogger, get_logger
from ..multihead import parse_multihead_kwargs
from ..multihead import run as run_multihead
from ..video_classification_frozen.eval import (_distributed, classifier_state_dict, init_model, init_opt,  # noqa: F401
                                                load_checkpoint, load_pretrained)
from ..video_classification_frozen.utils import _widest, max_clips_per_call

logger = get_logger(__name__)

_GLOBAL_SEED = 0
np.random.seed(_GLOBAL_SEED)
torch.manual_seed(_GLOBAL_SEED)

pp = pprint.PrettyPrinter(indent=4)


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
    frames_per_clip = args_pretrain.get('frames_per_clip', 1)

    # -- DATA
    args_data = args_eval.get('data')
    dataset_name = args_data.get('dataset_name')
    num_classes = args_data.get('num_classes')
    root_path = args_data.get('root_path', None)
    image_folder = args_data.get('image_folder', None)
    resolution = args_data.get('resolution', 224)
    synthetic_length = args_data.get('synthetic_length', None)
    num_workers = args_data.get('num_workers', 0)

    # -- OPTIMIZATION
    args_opt = args_eval.get('optimization')
    batch_size = args_opt.get('batch_size')
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

    if not torch.cuda.is_available():
        raise RuntimeError("the frozen eval computes on the GPU through libvjepa_hip.so (there is no CPU path)")
    device = torch.device('cuda:0')
    torch.cuda.set_device(device)

    world_size, rank = init_distributed()
    logger.info(f'Initialized (rank/world-size) {rank}/{world_size}')

    # -- log/checkpointing paths
    folder = os.path.join(pretrain_folder, 'image_classification_frozen/')
    if eval_tag is not None:
        folder = os.path.join(folder, eval_tag)
    os.makedirs(folder, exist_ok=True)
    log_file = os.path.join(folder, f'{tag}_r{rank}.csv')
    latest_path = os.path.join(folder, f'{tag}-latest.pth.tar')

    if rank == 0 and multihead is None:
        csv_logger = CSVLogger(log_file, ('%d', 'epoch'), ('%.5f', 'loss'), ('%.5f', 'acc'))

    # -- pretrained encoder (frozen): the video ViT, or the image ViT with frames_per_clip == 1; both are fed [B,C,H,W] directly
    encoder = init_model(crop_size=resolution, device=device, pretrained=pretrained_path, model_name=model_name,
                         patch_size=patch_size, frames_per_clip=frames_per_clip, tubelet_size=tubelet_size,
                         uniform_power=uniform_power, checkpoint_key=checkpoint_key, use_SiLU=use_SiLU, tight_SiLU=tight_SiLU,
                         use_sdpa=use_sdpa)
    encoder.eval()
    for p in encoder.parameters():
        p.requires_grad = False

    # -- init classifier
    if multihead is None:
        classifier = AttentiveClassifier(embed_dim=encoder.embed_dim, num_heads=encoder.num_heads, depth=1,
                                         num_classes=num_classes).to(device)

    common = dict(dataset_name=dataset_name, root_path=root_path, resolution=resolution, image_folder=image_folder,
                  batch_size=batch_size, world_size=world_size, rank=rank, num_classes=num_classes,
                  synthetic_length=synthetic_length, num_workers=num_workers)
    train_loader = make_dataloader(training=True, **common)
    val_loader = make_dataloader(training=False, **common)
    ipe = len(train_loader)
    logger.info(f'Dataloader created... iterations per epoch: {ipe}')

    if multihead is not None:
        return run_multihead(hps=multihead, init_opt=init_opt, features=_image_features, encoder=encoder,
                             train_loader=train_loader, val_loader=val_loader, num_classes=num_classes, num_epochs=num_epochs,
                             use_bfloat16=use_bfloat16, folder=folder, tag=tag, rank=rank, world_size=world_size,
                             batch_size=batch_size, resume_checkpoint=resume_checkpoint, distributed=_distributed(), device=device)

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
        train_acc = run_one_epoch(device=device, training=True, encoder=encoder, classifier=classifier, scaler=scaler,
                                  optimizer=optimizer, scheduler=scheduler, wd_scheduler=wd_scheduler, data_loader=train_loader,
                                  use_bfloat16=use_bfloat16, history=record['train_history'])
        val_acc = run_one_epoch(device=device, training=False, encoder=encoder, classifier=classifier, scaler=scaler,
                                optimizer=optimizer, scheduler=scheduler, wd_scheduler=wd_scheduler, data_loader=val_loader,
                                use_bfloat16=use_bfloat16)
        logger.info('[%5d] train: %.3f%% test: %.3f%%' % (epoch + 1, train_acc, val_acc))
        if rank == 0:
            csv_logger.log(epoch + 1, train_acc, val_acc)
        save_checkpoint(epoch + 1)
        record['train_acc'].append(train_acc)
        record['val_acc'].append(val_acc)
    return record


def frozen_features(encoder, imgs):
    """encoder(imgs) in calls small enough that the widest activation of one call (token rows x fc1's width) stays below 2^31
    elements.  The rows are counted from the tokens THIS input makes -- the model's num_patches describes its native size only --
    and the calls' outputs are joined by the bit-exact row copy."""
    if not (hasattr(encoder, 'patch_size') and hasattr(encoder, 'tubelet_size') and hasattr(encoder, 'num_frames')):
        return encoder(imgs)
    B = imgs.shape[0]
    frames = encoder.num_frames if imgs.dim() == 4 else imgs.shape[2]
    depth = frames // encoder.tubelet_size if getattr(encoder, 'is_video', True) else 1     # the image model has no tubelets
    tokens = depth * (imgs.shape[-2] // encoder.patch_size) * (imgs.shape[-1] // encoder.patch_size)
    cap = max_clips_per_call(_widest(encoder), max(tokens, 1))
    if B <= cap:
        return encoder(imgs)
    out = None
    for c0 in range(0, B, cap):
        f = encoder(imgs[c0:c0 + cap])
        if out is None:
            out = torch.empty((B,) + tuple(f.shape[1:]), dtype=f.dtype, device=f.device)
        N, D = f.shape[1], f.shape[2]
        ops.copy_rows(f, out, 1, f.shape[0] * N, 0, B * N, c0 * N, f.shape[0] * N, D)
    return out


def _image_features(encoder, data, device):
    """One batch for the probe bank: the frozen features as a one-view list of [B, N, D], and the labels."""
    return [frozen_features(encoder, data[0].to(device, non_blocking=True))], data[1].to(device)


def run_one_epoch(device, training, encoder, classifier, scaler, optimizer, scheduler, wd_scheduler, data_loader, use_bfloat16,
                  *, history=None):
    """The reference's epoch (eval.py:262-317), same parameters in the same order.  history (keyword-only, optional list):
    (learning rate, loss) of each training iteration."""
    classifier.train(mode=training)
    criterion = torch.nn.CrossEntropyLoss()
    top1_meter = AverageMeter()
    for itr, data in enumerate(data_loader):

        if training:
            scheduler.step()
            wd_scheduler.step()

        imgs, labels = data[0].to(device, non_blocking=True), data[1].to(device)
        with torch.no_grad():
            outputs = frozen_features(encoder, imgs)
            if not training:
                outputs = classifier(outputs)
        if training:
            outputs = classifier(outputs)

        loss = criterion(outputs, labels)
        with torch.no_grad():
            top1_acc = 100. * outputs.max(dim=1).indices.eq(labels).sum() / len(imgs)
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


def make_dataloader(dataset_name, root_path, image_folder, batch_size, world_size, rank, resolution=224, training=False,
                    subset_file=None, num_classes=None, synthetic_length=None, num_workers=0, seed=None):
    """The reference's loader factory (eval.py:379-423) for `dataset_name: synthetic`; the real datasets raise, as
    data_manager.init_data does."""
    if str(dataset_name).lower() != 'synthetic':
        raise NotImplementedError(
            f"dataset_name={dataset_name!r}: the reference's timm / torchvision image pipeline (ImageNet, iNat21, Places205) is not "
            "part of this package; use data.dataset_name: synthetic, or pass your own loader to run_one_epoch")
    if num_classes is None:
        raise ValueError("make_dataloader(dataset_name='synthetic') needs num_classes")
    length = synthetic_length if synthetic_length is not None else 8 * batch_size * world_size
    dataset = SyntheticImageClassification(length, num_classes, resolution, seed=(0 if training else 1) if seed is None else seed)
    sampler = torch.utils.data.distributed.DistributedSampler(dataset, num_replicas=world_size, rank=rank, shuffle=training)
    return torch.utils.data.DataLoader(dataset, sampler=sampler, batch_size=batch_size, drop_last=False,
                                       num_workers=num_workers, pin_memory=True, persistent_workers=False)
