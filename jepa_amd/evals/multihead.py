"""A bank of attentive probes in the frozen evals: `optimization.multihead_kwargs`, a list of dictionaries, one per probe, each
of which may override `lr`, `start_lr`, `final_lr`, `weight_decay` and `warmup` of `optimization` (the grid of probe learning
rates and weight decays the frozen protocol sweeps).  Both evals' `main` hand over to `run` when the key is present; without it
they run their own single-probe code, unchanged.

One AttentiveClassifierBank on one frozen forward pass per iteration; per probe its own AdamW, LR / WD schedule and GradScaler
(the evals' `init_opt`); ONE backward of the summed per-probe losses (the probes share no parameter, so each receives its own
gradient); `clip_grad_norm_(1.0)`, accuracy meter and `{tag}_p{p}_r{rank}.csv` per probe; the checkpoint carries per-probe lists
of classifier (reference format, `module.` prefix: the winner loads into the reference), optimizer and scaler state.  The update
of one probe, the prefix and the resume frame are the single-probe evals' too (.frozen); the epoch loop is this module's own: its
meters, schedules and log line are per-probe lists.
"""
import torch
import torch.nn.functional as F
from torch.nn.parallel import DistributedDataParallel

from ..src.models.attentive_pooler import AttentiveClassifierBank
from ..src.utils.distributed import AllReduce
from ..src.utils.logging import AverageMeter, CSVLogger, get_logger
from .frozen import HP_KEYS, parse_multihead_kwargs  # noqa: F401  (this module's names)
from .frozen import add_module_prefix, probe_update, resume, strip_module_prefix

logger = get_logger(__name__)


def _probes(bank):
    return (bank.module if isinstance(bank, DistributedDataParallel) else bank).probes


def run(*, hps, init_opt, features, encoder, train_loader, val_loader, num_classes, num_epochs, use_bfloat16, folder, tag, rank,
        world_size, batch_size, resume_checkpoint, distributed, device):
    """The epochs of a multi-probe eval.  features(encoder, data, device) -> (list of [B, N, D] feature tensors, one per view,
    labels): what differs between the video and the image eval.  Returns the run's record with per-probe lists."""
    P = len(hps)
    ipe = len(train_loader)
    latest_path = f'{folder}/{tag}-latest.pth.tar'
    csv_loggers = [CSVLogger(f'{folder}/{tag}_p{p}_r{rank}.csv', ('%d', 'epoch'), ('%.5f', 'loss'), ('%.5f', 'acc'))
                   for p in range(P)] if rank == 0 else None
    bank = AttentiveClassifierBank(encoder.embed_dim, encoder.num_heads, num_classes, P).to(device)
    opts = [init_opt(classifier=m, wd=hp['weight_decay'], start_lr=hp['start_lr'], ref_lr=hp['lr'], final_lr=hp['final_lr'],
                     iterations_per_epoch=ipe, warmup=hp['warmup'], num_epochs=num_epochs, use_bfloat16=use_bfloat16)
            for m, hp in zip(bank.probes, hps)]
    optimizers, scalers, schedulers, wd_schedulers = (list(t) for t in zip(*opts))
    if distributed:
        bank = DistributedDataParallel(bank, static_graph=True)

    start_epoch = 0
    if resume_checkpoint:
        start_epoch = load_checkpoint(latest_path, bank, optimizers, scalers)
        for _ in range(start_epoch * ipe):
            for s, w in zip(schedulers, wd_schedulers):
                s.step()
                w.step()

    record = dict(start_epoch=start_epoch, train_acc=[], val_acc=[], train_history=[], multihead_kwargs=hps)
    for epoch in range(start_epoch, num_epochs):
        logger.info('Epoch %d' % (epoch + 1))
        common = dict(device=device, features=features, encoder=encoder, bank=bank, scalers=scalers, optimizers=optimizers,
                      schedulers=schedulers, wd_schedulers=wd_schedulers, use_bfloat16=use_bfloat16)
        train_acc = run_one_epoch(training=True, data_loader=train_loader, history=record['train_history'], **common)
        val_acc = run_one_epoch(training=False, data_loader=val_loader, **common)
        for p in range(P):
            logger.info('[%5d] probe %d train: %.3f%% test: %.3f%%' % (epoch + 1, p, train_acc[p], val_acc[p]))
            if rank == 0:
                csv_loggers[p].log(epoch + 1, train_acc[p], val_acc[p])
        if rank == 0:
            torch.save({
                'classifier': [add_module_prefix(m.state_dict()) for m in _probes(bank)],
                'opt': [o.state_dict() for o in optimizers],
                'scaler': [None if s is None else s.state_dict() for s in scalers],
                'epoch': epoch + 1,
                'batch_size': batch_size,
                'world_size': world_size,
                'lr': [hp['lr'] for hp in hps],
                'multihead_kwargs': hps,
            }, latest_path)
        record['train_acc'].append(train_acc)
        record['val_acc'].append(val_acc)
    if record['val_acc']:
        last = record['val_acc'][-1]
        best = max(range(P), key=lambda p: last[p])
        record['best_probe'] = best
        logger.info('best probe by validation accuracy: %d (%.3f%%) with %s' % (best, last[best], hps[best]))
    return record


def run_one_epoch(device, training, features, encoder, bank, scalers, optimizers, schedulers, wd_schedulers, data_loader,
                  use_bfloat16, history=None):
    """The evals' epoch for a bank -> the per-probe average top-1.  history (optional list): per training iteration, the
    per-probe learning rates and losses."""
    bank.train(mode=training)
    criterion = torch.nn.CrossEntropyLoss()
    probes = _probes(bank)
    P = len(probes)
    meters = [AverageMeter() for _ in range(P)]
    for itr, data in enumerate(data_loader):
        if training:
            for s, w in zip(schedulers, wd_schedulers):
                s.step()
                w.step()
        with torch.no_grad():
            views, labels = features(encoder, data, device)
            if not training:
                outputs = [bank(v) for v in views]
        if training:
            outputs = [bank(v) for v in views]                                       # per view: logits [P, B, C]
        losses = [sum(criterion(o[p], labels) for o in outputs) / len(outputs) for p in range(P)]
        with torch.no_grad():
            probs = sum(F.softmax(o, dim=2) for o in outputs) / len(outputs)
            for p in range(P):
                top1_acc = 100. * probs[p].max(dim=1).indices.eq(labels).sum() / len(labels)
                meters[p].update(float(AllReduce.apply(top1_acc)))
        if training:
            if use_bfloat16:
                sum(s.scale(ls) for s, ls in zip(scalers, losses)).backward()
            else:
                sum(losses).backward()
            for m, opt, scaler in zip(probes, optimizers, scalers):
                probe_update(m, opt, scaler, use_bfloat16)
            if history is not None:
                history.append(([o.param_groups[0]['lr'] for o in optimizers], [float(ls.detach()) for ls in losses]))
        if itr % 20 == 0:
            logger.info('[%5d] best %.3f%% (mean loss: %.3f) [mem: %.2e]'
                        % (itr, max(m.avg for m in meters), float(sum(ls.detach() for ls in losses)) / P,
                           torch.cuda.max_memory_allocated() / 1024.**2))
    return [m.avg for m in meters]


def load_checkpoint(r_path, bank, optimizers, scalers):
    """Restores every probe, optimizer and scaler from the per-probe lists -> the epoch to continue from (0 when nothing loads)."""
    def restore(checkpoint, epoch):
        probes = _probes(bank)
        if len(checkpoint['classifier']) != len(probes):
            raise ValueError(f"checkpoint holds {len(checkpoint['classifier'])} probes, the config asks for {len(probes)}")
        for m, sd, opt, osd, scaler, ssd in zip(probes, checkpoint['classifier'], optimizers, checkpoint['opt'], scalers,
                                                checkpoint['scaler']):
            m.load_state_dict(strip_module_prefix(sd))
            opt.load_state_dict(osd)
            if scaler is not None:
                scaler.load_state_dict(ssd)
        logger.info(f'loaded {len(probes)} probes and their optimizers from epoch {epoch}; read-path: {r_path}')

    return resume(r_path, restore)
