"""tools/train_utils/train_utils.py of the reference (and model_fn_decorator of pcdet/models/__init__.py): the training
loop over a loader of batch dicts as data_augmentor.prepare_batch makes them.

Same names, signatures and keyword defaults as the reference.  What differs:
  * the loader is any sized iterable of batch dicts (already on the device);
  * no progress bar is required: progress goes to `logger` (any object with .info), `tbar` may be None; `tb_log` is any
    object with add_scalar(tag, value, step);
  * with the fused optimiser (fastai_optim.OptimWrapper) the gradient clipping at GRAD_NORM_CLIP is part of step(); with
    torch's own optimisers clip_grad_norm_ runs as in the reference;
  * per iteration the loop reads nothing from the device on top of the one copy get_loss makes for tb_dict: 'train/loss'
    goes to tb_log as the detached device tensor, and the loss value, the gradient norm and the optimiser's status word
    are read at the logging interval only (logger_iter_interval, the first and the last iteration of an epoch);
  * use_amp=True and a DistributedDataParallel model raise NotImplementedError (mixed precision and multi-GPU training
    are out of scope)."""
import glob
import os
import time
from collections import namedtuple

import torch
from torch.nn.utils import clip_grad_norm_

from .optimization.fastai_optim import OptimWrapper


def model_fn_decorator():
    ModelReturn = namedtuple('ModelReturn', ['loss', 'tb_dict', 'disp_dict'])

    def model_func(model, batch_dict):
        # the modules add their outputs to the dict they are given: the loader's own dict stays as it was made
        ret_dict, tb_dict, disp_dict = model(dict(batch_dict))
        loss = ret_dict['loss'].mean()
        (model if hasattr(model, 'update_global_step') else model.module).update_global_step()
        return ModelReturn(loss, tb_dict, disp_dict)

    return model_func


def _refuse(model, use_amp):
    if use_amp:
        raise NotImplementedError("use_amp=True: mixed precision is not part of this package")
    if isinstance(model, torch.nn.parallel.DistributedDataParallel):
        raise NotImplementedError("DistributedDataParallel: multi-GPU training is not part of this package")


def train_one_epoch(model, optimizer, train_loader, model_func, lr_scheduler, accumulated_iter, optim_cfg,
                    rank, tbar, total_it_each_epoch, dataloader_iter, tb_log=None, leave_pbar=False,
                    use_logger_to_record=False, logger=None, logger_iter_interval=50, cur_epoch=None,
                    total_epochs=None, ckpt_save_dir=None, ckpt_save_time_interval=300, show_gpu_stat=False, use_amp=False):
    _refuse(model, use_amp)
    if total_it_each_epoch == len(train_loader):
        dataloader_iter = iter(train_loader)
    interval = logger_iter_interval or 50
    fused = isinstance(optimizer, OptimWrapper)
    start_it = accumulated_iter % total_it_each_epoch
    ckpt_save_cnt = 1
    epoch_start = time.time()
    loss_sum, loss_cnt = None, 0
    for cur_it in range(start_it, total_it_each_epoch):
        try:
            batch = next(dataloader_iter)
        except StopIteration:
            dataloader_iter = iter(train_loader)
            batch = next(dataloader_iter)
        lr_scheduler.step(accumulated_iter, cur_epoch)
        try:
            cur_lr = float(optimizer.lr)
        except (AttributeError, TypeError):
            cur_lr = optimizer.param_groups[0]['lr']
        if tb_log is not None:
            tb_log.add_scalar('meta_data/learning_rate', cur_lr, accumulated_iter)
        model.train()
        optimizer.zero_grad()
        loss, tb_dict, disp_dict = model_func(model, batch)
        loss.backward()
        grad_norm = None
        if not fused:
            grad_norm = clip_grad_norm_(model.parameters(), optim_cfg.GRAD_NORM_CLIP)
        optimizer.step()
        if fused:
            grad_norm = optimizer.last_total_norm
        accumulated_iter += 1
        if rank != 0:
            continue
        loss_sum = loss.detach().double() if loss_sum is None else loss_sum + loss.detach()
        loss_cnt += 1
        if tb_log is not None:
            tb_log.add_scalar('train/loss', loss.detach(), accumulated_iter)
            tb_log.add_scalar('meta_data/learning_rate', cur_lr, accumulated_iter)
            for key, val in tb_dict.items():
                tb_log.add_scalar('train/' + key, val, accumulated_iter)
        if accumulated_iter % interval == 0 or cur_it == start_it or cur_it + 1 == total_it_each_epoch:
            # the only device reads of the loop's own
            if fused:
                optimizer.check_status()
            norm_val = float(grad_norm) if grad_norm is not None else float('nan')
            if tb_log is not None:
                tb_log.add_scalar('train/grad_norm', norm_val, accumulated_iter)
            if logger is not None:
                elapsed = time.time() - epoch_start
                logger.info('Train: %4d/%s [%4d/%d]  Loss: %.4g (%.3g)  LR: %.3e  Grad norm: %.4g  Acc_iter %d  '
                            'Time: %.1fs (%.3fs/it)' % (
                                (cur_epoch if cur_epoch is not None else 0) + 1, total_epochs, cur_it + 1, total_it_each_epoch,
                                float(loss.detach()), float(loss_sum) / loss_cnt, cur_lr, norm_val, accumulated_iter, elapsed,
                                elapsed / max(cur_it - start_it + 1, 1)))
        if ckpt_save_dir is not None and ckpt_save_time_interval and \
                (time.time() - epoch_start) // ckpt_save_time_interval >= ckpt_save_cnt:
            ckpt_name = os.path.join(str(ckpt_save_dir), 'latest_model')
            save_checkpoint(checkpoint_state(model, optimizer, cur_epoch, accumulated_iter), filename=ckpt_name)
            if logger is not None:
                logger.info('Save latest model to %s' % ckpt_name)
            ckpt_save_cnt += 1
    return accumulated_iter


def train_model(model, optimizer, train_loader, model_func, lr_scheduler, optim_cfg,
                start_epoch, total_epochs, start_iter, rank, tb_log, ckpt_save_dir, train_sampler=None,
                lr_warmup_scheduler=None, ckpt_save_interval=1, max_ckpt_save_num=50,
                merge_all_iters_to_one_epoch=False, use_amp=False,
                use_logger_to_record=False, logger=None, logger_iter_interval=None, ckpt_save_time_interval=None,
                show_gpu_stat=False, cfg=None):
    _refuse(model, use_amp)
    hook = cfg.get('HOOK', None) if cfg is not None else None
    if hook is not None and hook.get('DisableAugmentationHook', None) is not None:
        raise NotImplementedError("HOOK.DisableAugmentationHook: the loader is a plain iterable of batches, it has no "
                                  "augmentor to switch off")
    accumulated_iter = start_iter
    total_it_each_epoch = len(train_loader)
    if merge_all_iters_to_one_epoch:
        assert hasattr(train_loader.dataset, 'merge_all_iters_to_one_epoch')
        train_loader.dataset.merge_all_iters_to_one_epoch(merge=True, epochs=total_epochs)
        total_it_each_epoch = len(train_loader) // max(total_epochs, 1)
    dataloader_iter = iter(train_loader)
    for cur_epoch in range(start_epoch, total_epochs):
        if train_sampler is not None:
            train_sampler.set_epoch(cur_epoch)
        if lr_warmup_scheduler is not None and cur_epoch < optim_cfg.WARMUP_EPOCH:
            cur_scheduler = lr_warmup_scheduler
        else:
            cur_scheduler = lr_scheduler
        accumulated_iter = train_one_epoch(
            model, optimizer, train_loader, model_func, lr_scheduler=cur_scheduler, accumulated_iter=accumulated_iter,
            optim_cfg=optim_cfg, rank=rank, tbar=None, tb_log=tb_log, leave_pbar=(cur_epoch + 1 == total_epochs),
            total_it_each_epoch=total_it_each_epoch, dataloader_iter=dataloader_iter, cur_epoch=cur_epoch,
            total_epochs=total_epochs, use_logger_to_record=use_logger_to_record, logger=logger,
            logger_iter_interval=logger_iter_interval, ckpt_save_dir=ckpt_save_dir,
            ckpt_save_time_interval=ckpt_save_time_interval, show_gpu_stat=show_gpu_stat, use_amp=use_amp)
        trained_epoch = cur_epoch + 1
        if trained_epoch % ckpt_save_interval == 0 and rank == 0:
            ckpt_list = glob.glob(os.path.join(str(ckpt_save_dir), 'checkpoint_epoch_*.pth'))
            ckpt_list.sort(key=os.path.getmtime)
            if len(ckpt_list) >= max_ckpt_save_num:
                for old in ckpt_list[:len(ckpt_list) - max_ckpt_save_num + 1]:
                    os.remove(old)
            ckpt_name = os.path.join(str(ckpt_save_dir), 'checkpoint_epoch_%d' % trained_epoch)
            save_checkpoint(checkpoint_state(model, optimizer, trained_epoch, accumulated_iter), filename=ckpt_name)


def model_state_to_cpu(model_state):
    model_state_cpu = type(model_state)()
    for key, val in model_state.items():
        model_state_cpu[key] = val.cpu()
    return model_state_cpu


def checkpoint_state(model=None, optimizer=None, epoch=None, it=None):
    if isinstance(model, torch.nn.parallel.DistributedDataParallel):
        raise NotImplementedError("DistributedDataParallel: multi-GPU training is not part of this package")
    optim_state = optimizer.state_dict() if optimizer is not None else None
    model_state = model.state_dict() if model is not None else None
    import dfu3d_amd
    version = getattr(dfu3d_amd, '__version__', None)
    version = 'dfu3d_amd+' + version if version else 'none'
    return {'epoch': epoch, 'it': it, 'model_state': model_state, 'optimizer_state': optim_state, 'version': version}


def save_checkpoint(state, filename='checkpoint'):
    torch.save(state, '{}.pth'.format(filename))
