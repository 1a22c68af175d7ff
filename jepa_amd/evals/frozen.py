"""What the frozen video- and image-classification evals (.video_classification_frozen.eval, .image_classification_frozen.eval)
and the probe bank (.multihead) share: one definition each of

  - the PRETRAIN / OPTIMIZATION / EXPERIMENT keys of the YAML schema and their defaults (parse_config, parse_multihead_kwargs);
  - the device check, process group, folder and file names of a run (setup_run);
  - the update of one probe (probe_update), the epoch of a single probe (run_probe_epoch) and its training run -- resume, epochs,
    CSV, checkpoint, record (train_single_probe);
  - the `module.` prefix convention of the classifier checkpoints (add_module_prefix, strip_module_prefix, classifier_state_dict)
    and the "load what is there, else start at epoch 0" frame of resuming (resume, load_checkpoint);
  - encoder calls in pieces that keep fc1's output below 2^31 elements (max_clips_per_call, widest_activation, chunked_call);
  - the loader of a synthetic split (synthetic_dataloader).

Each eval keeps what is its own: its DATA block, its encoder wrapper, its features and its prediction arithmetic.
"""
import os
from types import SimpleNamespace

import torch
from torch.nn.parallel import DistributedDataParallel

from ..hip import ops
from ..src.utils.distributed import AllReduce, init_distributed
from ..src.utils.logging import AverageMeter, CSVLogger, get_logger

logger = get_logger(__name__)

HP_KEYS = ('lr', 'start_lr', 'final_lr', 'weight_decay', 'warmup')


# ---------------------------------------------------------------------------------------------------------------- configuration

def parse_multihead_kwargs(args_opt):
    """-> None without the key (the single-probe eval), else one {lr, start_lr, final_lr, weight_decay, warmup} per probe with the
    missing keys taken from `optimization`."""
    entries = args_opt.get('multihead_kwargs', None)
    if entries is None:
        return None
    if not isinstance(entries, (list, tuple)) or len(entries) == 0 or not all(isinstance(e, dict) for e in entries):
        raise ValueError("optimization.multihead_kwargs must be a non-empty list of dictionaries")
    hps = []
    for i, e in enumerate(entries):
        unknown = sorted(set(e) - set(HP_KEYS))
        if unknown:
            raise ValueError(f"optimization.multihead_kwargs[{i}]: unknown keys {unknown}; a probe may override {list(HP_KEYS)}")
        hps.append({k: e.get(k, args_opt.get(k)) for k in HP_KEYS})
    return hps


def parse_config(args_eval, resume_preempt=False):
    """The PRETRAIN, OPTIMIZATION and EXPERIMENT values both evals read, with the reference's defaults.  `args_pretrain` and
    `args_opt` are the blocks themselves, for the keys only one eval reads; the DATA block is each eval's own."""
    args_pretrain = args_eval.get('pretrain')
    args_opt = args_eval.get('optimization')
    pretrain_folder = args_pretrain.get('folder', None)
    ckp_fname = args_pretrain.get('checkpoint', None)
    return SimpleNamespace(
        # -- PRETRAIN
        args_pretrain=args_pretrain,
        checkpoint_key=args_pretrain.get('checkpoint_key', 'target_encoder'),
        model_name=args_pretrain.get('model_name', None),
        patch_size=args_pretrain.get('patch_size', None),
        pretrain_folder=pretrain_folder,
        ckp_fname=ckp_fname,
        tag=args_pretrain.get('write_tag', None),
        use_sdpa=args_pretrain.get('use_sdpa', True),
        use_SiLU=args_pretrain.get('use_silu', False),
        tight_SiLU=args_pretrain.get('tight_silu', True),
        uniform_power=args_pretrain.get('uniform_power', False),
        pretrained_path=os.path.join(pretrain_folder, ckp_fname),
        tubelet_size=args_pretrain.get('tubelet_size', 2),
        frames_per_clip=args_pretrain.get('frames_per_clip', 1),
        # -- OPTIMIZATION
        args_opt=args_opt,
        batch_size=args_opt.get('batch_size'),
        num_epochs=args_opt.get('num_epochs'),
        wd=args_opt.get('weight_decay'),
        start_lr=args_opt.get('start_lr'),
        lr=args_opt.get('lr'),
        final_lr=args_opt.get('final_lr'),
        warmup=args_opt.get('warmup'),
        use_bfloat16=args_opt.get('use_bfloat16'),
        multihead=parse_multihead_kwargs(args_opt),   # None: the single probe; a list: one bank of probes (.multihead)
        # -- EXPERIMENT-ID/TAG (optional)
        resume_checkpoint=args_eval.get('resume_checkpoint', False) or resume_preempt,
        eval_tag=args_eval.get('tag', None))


def distributed():
    import torch.distributed as dist
    return dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1


def setup_run(cfg, folder_name, csv):
    """Device, process group and the log / checkpoint paths under `<pretrain folder>/<folder_name>[<tag>/]`.  csv: open the
    single probe's CSV log (rank 0 only; the probe bank writes one per probe instead)."""
    if not torch.cuda.is_available():
        raise RuntimeError("the frozen eval computes on the GPU through libvjepa_hip.so (there is no CPU path)")
    device = torch.device('cuda:0')
    torch.cuda.set_device(device)

    world_size, rank = init_distributed()
    logger.info(f'Initialized (rank/world-size) {rank}/{world_size}')

    # -- log/checkpointing paths
    folder = os.path.join(cfg.pretrain_folder, folder_name)
    if cfg.eval_tag is not None:
        folder = os.path.join(folder, cfg.eval_tag)
    os.makedirs(folder, exist_ok=True)
    log_file = os.path.join(folder, f'{cfg.tag}_r{rank}.csv')
    csv_logger = None
    if rank == 0 and csv:
        csv_logger = CSVLogger(log_file, ('%d', 'epoch'), ('%.5f', 'loss'), ('%.5f', 'acc'))
    return SimpleNamespace(device=device, world_size=world_size, rank=rank, folder=folder, csv_logger=csv_logger,
                           latest_path=os.path.join(folder, f'{cfg.tag}-latest.pth.tar'))


def freeze(encoder):
    encoder.eval()
    for p in encoder.parameters():
        p.requires_grad = False
    return encoder


# ------------------------------------------------------------------------------------------------------------------ probe update

def probe_update(classifier, optimizer, scaler, use_bfloat16, loss=None):
    """The update of one probe: the backward of `loss` (None: the caller has done it -- the bank's one backward of the summed
    losses), gradient clipping at norm 1.0, the optimizer step -- through the GradScaler with use_bfloat16 -- and zero_grad."""
    if use_bfloat16:
        if loss is not None:
            scaler.scale(loss).backward()
        scaler.unscale_(optimizer)
        torch.nn.utils.clip_grad_norm_(classifier.parameters(), 1.0)
        scaler.step(optimizer)
        scaler.update()
    else:
        if loss is not None:
            loss.backward()
        torch.nn.utils.clip_grad_norm_(classifier.parameters(), 1.0)
        optimizer.step()
    optimizer.zero_grad()


def run_probe_epoch(training, classifier, scaler, optimizer, scheduler, wd_scheduler, data_loader, use_bfloat16, features,
                    loss_and_top1, history=None, features_grad=False, after_update=None):
    """One epoch of a single probe -> its average top-1.  What an eval brings: features(data) -> (frozen features, labels), run
    under no_grad, and loss_and_top1(features, labels) -> (loss, top-1 in percent of this batch), which applies the classifier
    (with gradients only when training) and holds the eval's own prediction arithmetic.  history (optional list): (learning rate,
    loss) of each training iteration.  The fine-tuning eval's two additions, off by default: features_grad -- training iterations
    compute the features with gradients enabled, so the probe's backward reaches the encoder; after_update(optimizer, grad_scale)
    -- called after the probe's update of a training iteration (the encoder's step), with the factor the GradScaler had put on
    the loss of that backward (1.0 without use_bfloat16)."""
    classifier.train(mode=training)
    top1_meter = AverageMeter()
    for itr, data in enumerate(data_loader):

        if training:
            scheduler.step()
            wd_scheduler.step()

        with torch.set_grad_enabled(training and features_grad):
            outputs, labels = features(data)
        with torch.set_grad_enabled(training):
            loss, top1_acc = loss_and_top1(outputs, labels)
        del outputs     # the features live no longer than the probe needs them: not across the next frozen forward
        with torch.no_grad():
            top1_meter.update(float(AllReduce.apply(top1_acc)))

        if training:
            grad_scale = scaler.get_scale() if (use_bfloat16 and after_update is not None) else 1.0
            probe_update(classifier, optimizer, scaler, use_bfloat16, loss=loss)
            if after_update is not None:
                after_update(optimizer, grad_scale)
            if history is not None:
                history.append((optimizer.param_groups[0]['lr'], float(loss.detach())))

        if itr % 20 == 0:
            logger.info('[%5d] %.3f%% (loss: %.3f) [mem: %.2e]'
                        % (itr, top1_meter.avg, float(loss.detach()), torch.cuda.max_memory_allocated() / 1024.**2))

    return top1_meter.avg


# ------------------------------------------------------------------------------------------------------------------- checkpoints

def add_module_prefix(state_dict):
    """The keys as the reference's DistributedDataParallel-wrapped classifier writes them."""
    return {'module.' + k: v for k, v in state_dict.items()}


def strip_module_prefix(state_dict):
    return {(k[len('module.'):] if k.startswith('module.') else k): v for k, v in state_dict.items()}


def classifier_state_dict(classifier):
    """The classifier's state dict with the `module.` prefix the reference's DDP-wrapped classifier writes."""
    sd = classifier.state_dict()
    return sd if isinstance(classifier, DistributedDataParallel) else add_module_prefix(sd)


def resume(r_path, restore):
    """restore(checkpoint, epoch) on the checkpoint at r_path -> its epoch; 0 when it cannot be read or restore raises."""
    try:
        checkpoint = torch.load(r_path, map_location=torch.device('cpu'))
        epoch = checkpoint['epoch']
        restore(checkpoint, epoch)
        del checkpoint
    except Exception as e:
        logger.info(f'Encountered exception when loading checkpoint {e}')
        epoch = 0
    return epoch


def load_checkpoint(device, r_path, classifier, opt, scaler, restore_extra=None):
    """restore_extra(checkpoint) (optional): what the caller keeps in the checkpoint beside the probe (extra_state of
    train_single_probe), restored with it -- if it raises, the run starts at epoch 0 like after any unreadable checkpoint."""
    def restore(checkpoint, epoch):
        # -- loading classifier (`module.`-prefixed keys, as the reference writes them)
        pretrained_dict = checkpoint['classifier']
        if not isinstance(classifier, DistributedDataParallel):
            pretrained_dict = strip_module_prefix(pretrained_dict)
        msg = classifier.load_state_dict(pretrained_dict)
        logger.info(f'loaded pretrained classifier from epoch {epoch} with msg: {msg}')

        # -- loading optimizer
        opt.load_state_dict(checkpoint['opt'])
        if scaler is not None:
            scaler.load_state_dict(checkpoint['scaler'])
        if restore_extra is not None:
            restore_extra(checkpoint)
        logger.info(f'loaded optimizers from epoch {epoch}')
        logger.info(f'read-path: {r_path}')

    return classifier, opt, scaler, resume(r_path, restore)


# --------------------------------------------------------------------------------------------------------- single-probe training

def train_single_probe(cfg, run, classifier, opt, ipe, train_epoch, val_epoch, extra_state=None, restore_extra=None):
    """The training of a single probe.  opt: what the eval's init_opt returned for `classifier`; ipe: iterations per epoch;
    train_epoch(classifier=, scaler=, optimizer=, scheduler=, wd_scheduler=, history=) and val_epoch(the same without history)
    run one epoch on the eval's loaders -> its top-1.  Returns the run's record.  extra_state() -> dict (optional): further
    entries of every checkpoint (the fine-tuned encoder and its optimizer state); restore_extra(checkpoint) reads them on resume."""
    optimizer, scaler, scheduler, wd_scheduler = opt
    if distributed():
        classifier = DistributedDataParallel(classifier, static_graph=True)

    # -- load training checkpoint
    start_epoch = 0
    if cfg.resume_checkpoint:
        classifier, optimizer, scaler, start_epoch = load_checkpoint(device=run.device, r_path=run.latest_path,
                                                                     classifier=classifier, opt=optimizer, scaler=scaler,
                                                                     restore_extra=restore_extra)
        for _ in range(start_epoch * ipe):
            scheduler.step()
            wd_scheduler.step()

    def save_checkpoint(epoch):
        save_dict = {
            'classifier': classifier_state_dict(classifier),
            'opt': optimizer.state_dict(),
            'scaler': None if scaler is None else scaler.state_dict(),
            'epoch': epoch,
            'batch_size': cfg.batch_size,
            'world_size': run.world_size,
            'lr': cfg.lr
        }
        if extra_state is not None:
            save_dict.update(extra_state())
        if run.rank == 0:
            torch.save(save_dict, run.latest_path)

    probe = dict(classifier=classifier, scaler=scaler, optimizer=optimizer, scheduler=scheduler, wd_scheduler=wd_scheduler)
    record = dict(start_epoch=start_epoch, train_acc=[], val_acc=[], train_history=[])
    for epoch in range(start_epoch, cfg.num_epochs):
        logger.info('Epoch %d' % (epoch + 1))
        train_acc = train_epoch(history=record['train_history'], **probe)
        val_acc = val_epoch(**probe)
        logger.info('[%5d] train: %.3f%% test: %.3f%%' % (epoch + 1, train_acc, val_acc))
        if run.rank == 0:
            run.csv_logger.log(epoch + 1, train_acc, val_acc)
        save_checkpoint(epoch + 1)
        record['train_acc'].append(train_acc)
        record['val_acc'].append(val_acc)
    return record


# --------------------------------------------------------------------------------------------------------- chunked encoder calls

def max_clips_per_call(width, tokens_per_clip):
    """Clips (or frames of an image encoder: tokens_per_clip is then one frame's tokens; with 1, token rows) per encoder call that
    keep the widest activation (M token rows x `width` columns: fc1's output) below 2^31 elements."""
    return max(1, (2 ** 31 - 1) // (width * tokens_per_clip))


def widest_activation(model):
    """Widest activation row of the encoder: fc1's output features (4 D for L / H, 48/11 D for ViT-g), at least 3 D (qkv)."""
    blocks = getattr(model, "blocks", None)
    fc1 = blocks[0].mlp.fc1.out_features if blocks is not None and len(blocks) else 4 * model.embed_dim
    return max(fc1, 3 * model.embed_dim)


def chunked_call(encoder, x, cap):
    """encoder(x) -> [M, N, D] in calls of at most `cap` entries along dimension 0; the calls' outputs are joined by the bit-exact
    row copy (vj_copy_rows)."""
    M = x.shape[0]
    if M <= cap:
        return encoder(x)
    out = None
    for c0 in range(0, M, cap):
        f = encoder(x[c0:c0 + cap])
        if out is None:
            out = torch.empty((M,) + tuple(f.shape[1:]), dtype=f.dtype, device=f.device)
        N, D = f.shape[1], f.shape[2]
        ops.copy_rows(f, out, 1, f.shape[0] * N, 0, M * N, c0 * N, f.shape[0] * N, D)
    return out


# ----------------------------------------------------------------------------------------------------------------------- loaders

def synthetic_dataloader(make_dataset, batch_size, world_size, rank, training, num_workers, synthetic_length=None, seed=None):
    """The loader of a synthetic split: make_dataset(length, seed) with the default length of 8 batches per rank and the split's
    seed (0 to train, 1 to validate), sharded by a DistributedSampler that shuffles the training split."""
    length = synthetic_length if synthetic_length is not None else 8 * batch_size * world_size
    dataset = make_dataset(length, (0 if training else 1) if seed is None else seed)
    sampler = torch.utils.data.distributed.DistributedSampler(dataset, num_replicas=world_size, rank=rank, shuffle=training)
    return torch.utils.data.DataLoader(dataset, sampler=sampler, batch_size=batch_size, drop_last=False,
                                       num_workers=num_workers, pin_memory=True, persistent_workers=False)
