"""The CenterHead loss on csrc/centerloss_stage.hip (C ABI: include/dfu3d_head.h).

`center_loss` is one autograd function over all heads: the focal loss of every head's heat-map logits against its
target heat map (pcdet's FocalLossCenterNet on the clamped sigmoid) and the L1 loss of the regression maps at the target
cells (RegLossCenterNet), three launches forward and two backward whatever the number of heads.  It returns
`losses` = [hm_loss_0, loc_loss_0, ..., total] and `chan` (n_heads, code), the unweighted per-channel regression
losses; both are differentiable.  Neither direction reads the device or copies to it: the per-head tensors' addresses
travel in the kernel arguments, the upstream gradient is read from device memory.

Inputs must be float32 tensors on the GPU; any other dtype raises Dfu3dError.  Inputs that are not contiguous (for
example channels_last maps) are made contiguous first, which costs a copy; gradients are returned contiguous.  `inds`
and `masks` are the int64 tensors `CenterHead.assign_targets` returns.  A slot counts iff its mask is not zero and its
ind lies inside the map; a NaN target channel of a slot is skipped.  Results are the same bits on every run and for
every alignment of the tensors (a map 16-byte aligned is only loaded faster).  The backward recomputes from the inputs,
which are saved through autograd: overwriting one in place before backward raises.  No double backward.
"""
import ctypes

import torch

from . import _lib_head
from ._lib import Dfu3dError

C = _lib_head.CONSTANTS
MAX_HEADS = C["DFU3D_HEAD_MAX_HEADS"]
MAX_REG_MAPS = C["DFU3D_HEAD_MAX_REG_MAPS"]
MAX_CODE = C["DFU3D_HEAD_MAX_CODE"]
MAX_OBJS = C["DFU3D_HEAD_MAX_OBJS"]
FWD_PTRS = C["DFU3D_HEAD_FWD_PTRS"]
BWD_PTRS = C["DFU3D_HEAD_BWD_PTRS"]


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


def _f32_map(t, what):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise Dfu3dError("center_loss: %s must be a tensor on the GPU" % what)
    if t.dtype != torch.float32:
        raise Dfu3dError("center_loss: %s must be float32, got %s" % (what, t.dtype))
    return t.contiguous()


class _Plan:
    """The host side of one call: shapes, weights and the address tables of the C ABI."""

    def __init__(self, n_heads, with_hm, reg_ch, n_max, batch, hw, n_cls, weights):
        self.n_heads, self.with_hm, self.reg_ch, self.n_max, self.batch, self.hw = n_heads, with_hm, reg_ch, n_max, batch, hw
        self.code = sum(reg_ch)
        self.n_cls = (ctypes.c_int32 * n_heads)(*n_cls)
        self.c_reg_ch = (ctypes.c_int32 * max(len(reg_ch), 1))(*reg_ch)
        self.weights = (ctypes.c_double * (2 + MAX_CODE))(*weights)

    def call_args(self, maps):
        return (maps, self.n_cls, self.n_heads, self.batch, self.hw, self.c_reg_ch, len(self.reg_ch), self.n_max)


def _check(hms, heats, regs, targets, inds, masks, cls_weight, loc_weight, code_weights):
    n_heads = len(hms) if hms is not None else len(regs)
    if not 1 <= n_heads <= MAX_HEADS:
        raise Dfu3dError("center_loss: %d heads, between 1 and %d" % (n_heads, MAX_HEADS))
    first = hms[0] if hms is not None else regs[0][0]
    if not isinstance(first, torch.Tensor) or first.dim() != 4:
        raise Dfu3dError("center_loss: the maps must be (B, C, H, W) tensors")
    B, hw, H, W = int(first.shape[0]), int(first.shape[2] * first.shape[3]), int(first.shape[2]), int(first.shape[3])
    if B < 1 or hw < 1:
        raise Dfu3dError("center_loss: empty maps %s" % (tuple(first.shape),))
    n_cls = [0] * n_heads
    if hms is not None:
        if len(heats) != n_heads:
            raise Dfu3dError("center_loss: %d logit maps, %d target heat maps" % (n_heads, len(heats)))
        hms = [_f32_map(t, "hm of head %d" % h) for h, t in enumerate(hms)]
        heats = [_f32_map(t, "heatmap of head %d" % h) for h, t in enumerate(heats)]
        for h in range(n_heads):
            if hms[h].shape != heats[h].shape or hms[h].dim() != 4 or tuple(hms[h].shape[::3]) != (B, W) or hms[h].shape[2] != H:
                raise Dfu3dError("center_loss: head %d: hm %s against heatmap %s, batch %d, map %d x %d"
                                 % (h, tuple(hms[h].shape), tuple(heats[h].shape), B, H, W))
            n_cls[h] = int(hms[h].shape[1])
    reg_ch, n_max = [], 0
    if regs is not None:
        if not (len(regs) == len(targets) == len(inds) == len(masks) == n_heads):
            raise Dfu3dError("center_loss: every head needs regression maps, target_boxes, inds and masks")
        if not 1 <= len(regs[0]) <= MAX_REG_MAPS:
            raise Dfu3dError("center_loss: %d regression maps per head, between 1 and %d" % (len(regs[0]), MAX_REG_MAPS))
        regs = [[_f32_map(t, "a regression map of head %d" % h) for t in maps] for h, maps in enumerate(regs)]
        reg_ch = [int(t.shape[1]) for t in regs[0]]
        if sum(reg_ch) > MAX_CODE:
            raise Dfu3dError("center_loss: %d regression channels, at most %d" % (sum(reg_ch), MAX_CODE))
        targets = [_f32_map(t, "target_boxes of head %d" % h) for h, t in enumerate(targets)]
        n_max = int(targets[0].shape[1])
        if not 1 <= n_max <= MAX_OBJS:
            raise Dfu3dError("center_loss: NUM_MAX_OBJS = %d, between 1 and %d" % (n_max, MAX_OBJS))
        for h in range(n_heads):
            if [tuple(t.shape) for t in regs[h]] != [(B, c, H, W) for c in reg_ch]:
                raise Dfu3dError("center_loss: head %d: regression maps %s, expected channels %s on (%d, ., %d, %d)"
                                 % (h, [tuple(t.shape) for t in regs[h]], reg_ch, B, H, W))
            if tuple(targets[h].shape) != (B, n_max, sum(reg_ch)):
                raise Dfu3dError("center_loss: head %d: target_boxes %s, expected %s"
                                 % (h, tuple(targets[h].shape), (B, n_max, sum(reg_ch))))
            for name, t in (("inds", inds[h]), ("masks", masks[h])):
                if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.int64 or tuple(t.shape) != (B, n_max):
                    raise Dfu3dError("center_loss: head %d: %s must be int64 (%d, %d) on the GPU" % (h, name, B, n_max))
        inds = [t.contiguous() for t in inds]
        masks = [t.contiguous() for t in masks]
        if len(code_weights) != sum(reg_ch):
            raise Dfu3dError("center_loss: %d code_weights for %d regression channels" % (len(code_weights), sum(reg_ch)))
    weights = [float(cls_weight), float(loc_weight)] + [float(w) for w in code_weights]
    plan = _Plan(n_heads, hms is not None, reg_ch, n_max, B, hw, n_cls, weights)
    return plan, hms, heats, regs, targets, inds, masks


def _fwd_table(plan, hms, heats, regs, targets, inds, masks):
    tab = (ctypes.c_uint64 * (plan.n_heads * FWD_PTRS))()
    for h in range(plan.n_heads):
        row = h * FWD_PTRS
        if plan.with_hm:
            tab[row], tab[row + 1] = hms[h].data_ptr(), heats[h].data_ptr()
        if plan.reg_ch:
            tab[row + 2], tab[row + 3], tab[row + 4] = targets[h].data_ptr(), inds[h].data_ptr(), masks[h].data_ptr()
            for m, t in enumerate(regs[h]):
                tab[row + 5 + m] = t.data_ptr()
    return tab


def _split(plan, tensors):
    """The flat tensor list of _CenterLoss.apply -> (n_maps, hms, regs, heats, targets, inds, masks)."""
    n, r = plan.n_heads, len(plan.reg_ch)
    t = list(tensors)
    hms = [t.pop(0) for _ in range(n)] if plan.with_hm else None
    regs = [[t.pop(0) for _ in range(r)] for _ in range(n)] if r else None
    heats = [t.pop(0) for _ in range(n)] if plan.with_hm else None
    targets, inds, masks = ([t.pop(0) for _ in range(n)] if r else None for _ in range(3))
    return (n if plan.with_hm else 0) + n * r, hms, regs, heats, targets, inds, masks


class _CenterLoss(torch.autograd.Function):
    """apply(plan, *maps, *heats, *targets, *inds, *masks): the differentiable maps first (hm of every head, then every
    head's regression maps)."""

    @staticmethod
    def forward(ctx, plan, *tensors):
        n = plan.n_heads
        _, hms, regs, heats, targets, inds, masks = _split(plan, tensors)
        dev = tensors[0].device
        L = _lib_head.lib()
        nbytes = L.dfu3d_center_loss_scratch_bytes(n, plan.batch, plan.code)
        if nbytes < 0:
            raise Dfu3dError("center_loss: dfu3d_center_loss_scratch_bytes(%d, %d, %d) failed" % (n, plan.batch, plan.code))
        scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        losses = torch.empty(2 * n + 1, dtype=torch.float32, device=dev)
        chan = torch.empty((n, plan.code), dtype=torch.float32, device=dev)
        stats = torch.empty((n, 2), dtype=torch.float64, device=dev)
        tab = _fwd_table(plan, hms, heats, regs, targets, inds, masks)
        # (an empty `chan` has no address; the ABI wants a pointer and writes nothing through it when the code is empty)
        rc = L.dfu3d_center_loss_fwd(*plan.call_args(tab), plan.weights, _p(losses), _p(chan) if plan.code else _p(losses),
                                     _p(stats), _p(scratch), nbytes, _stream())
        _lib_head.check(rc, "dfu3d_center_loss_fwd")
        # the backward recomputes from the inputs: saved through autograd, so that an input overwritten in place between
        # forward and backward raises instead of giving the gradient of other values
        ctx.save_for_backward(stats, *tensors)
        ctx.plan = plan
        return losses, chan

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_losses, grad_chan):
        plan = ctx.plan
        n, r = plan.n_heads, len(plan.reg_ch)
        stats, tensors = ctx.saved_tensors[0], ctx.saved_tensors[1:]
        n_maps, hms, regs, heats, targets, inds, masks = _split(plan, tensors)
        for g in (grad_losses, grad_chan):
            if g is not None and g.dtype != torch.float32:
                raise Dfu3dError("center_loss backward: the gradient must be float32, got %s" % g.dtype)
        grad_losses = grad_losses.contiguous() if grad_losses is not None else None
        grad_chan = grad_chan.contiguous() if grad_chan is not None and plan.code else None
        need = ctx.needs_input_grad[1:]
        out = [None] * len(tensors)
        tab = (ctypes.c_uint64 * (n * BWD_PTRS))()
        for h in range(n):
            if plan.with_hm and need[h]:
                out[h] = torch.empty_like(hms[h])
                tab[h * BWD_PTRS] = out[h].data_ptr()
            for m in range(r):
                i = (n if plan.with_hm else 0) + h * r + m
                if need[i]:
                    out[i] = torch.empty_like(regs[h][m])
                    tab[h * BWD_PTRS + 1 + m] = out[i].data_ptr()
        if any(o is not None for o in out[:n_maps]):
            args = plan.call_args(_fwd_table(plan, hms, heats, regs, targets, inds, masks))
            rc = _lib_head.lib().dfu3d_center_loss_bwd(args[0], tab, *args[1:], plan.weights,
                                                       _p(grad_losses) if grad_losses is not None else None,
                                                       _p(grad_chan) if grad_chan is not None else None, _p(stats),
                                                       _stream())
            _lib_head.check(rc, "dfu3d_center_loss_bwd")
        return (None,) + tuple(out)


def center_loss(hms, heatmaps, regs, target_boxes, inds, masks, cls_weight=1.0, loc_weight=1.0, code_weights=None):
    """hms / heatmaps: per head (B, n_cls_h, H, W) logits and targets, or None for no focal part.  regs: per head the
    list of regression maps (B, c_m, H, W) in the order of the target's columns, with target_boxes (B, NUM_MAX_OBJS,
    sum c_m) float32 and inds / masks (B, NUM_MAX_OBJS) int64 per head; or None for no regression part.
    Returns (losses (2 n_heads + 1), chan (n_heads, sum c_m))."""
    if hms is None and regs is None:
        raise Dfu3dError("center_loss: neither heat maps nor regression maps")
    if regs is not None and code_weights is None:
        code_weights = [1.0] * sum(int(t.shape[1]) for t in regs[0])
    plan, hms, heatmaps, regs, target_boxes, inds, masks = _check(
        hms, heatmaps, regs, target_boxes, inds, masks, cls_weight, loc_weight, code_weights or [])
    maps = (hms or []) + [t for head in (regs or []) for t in head]
    extras = (heatmaps or []) + (target_boxes or []) + (inds or []) + (masks or []) if regs is not None else (heatmaps or [])
    return _CenterLoss.apply(plan, *maps, *extras)
