"""Guard bands and poisoned scratch for the tests: a TorchDispatchMode that puts every tensor a test allocates between
two bands of a known byte and hands `empty` back filled with that byte.

    with Guarded(poison=0xFF) as g:
        x = torch.from_numpy(a).cuda()          # upload: values kept, bands around it
        out = torch.empty(n, device='cuda')     # scratch / output: all 0xFF, bands around it
        op(x, out)
        torch.cuda.synchronize()
        g.check()                               # every band still holds the poison
    assert g.count == 2

Why: torch's caching allocator rounds every size up to 512 B and packs small blocks into 2 MB segments, so a kernel that
reads or writes a few elements past a buffer lands in slack or in a neighbour and nothing notices; and a fresh process
mostly gets zeroed pages, so a kernel that relies on zeroed scratch passes until the block is a recycled one.

What is intercepted: the factory ops (empty, empty_strided, empty_like, new_empty, zeros, zeros_like, new_zeros, ones,
full, full_like, new_full) and uploads (aten._to_copy whose result is on a guarded device and whose source is not), when
the result is contiguous, strided, non-empty and on one of `devices`.  The real op runs first; then guard + nbytes + guard
bytes of uint8 are allocated, all of it is filled with the poison, and the middle comes back viewed as the op's dtype and
shape.  For every op but the empty family the real result is copied in, so zeros stay zero and uploads keep their values.

Placement: the payload starts `guard_bytes` (a multiple of 512) into the allocator's block, so its alignment is what the
allocator gives; it ends at its exact byte size, so the back band begins at the first byte past the size the caller
asked for, with no rounding.

Limits: an access farther than `guard_bytes` (64 KB by default) outside a buffer is out of this detector's reach.  A
buffer the library carves into sub-buffers is guarded at its two outer ends only.  Ops that allocate their result inside
a torch kernel (arithmetic, indexing, cat, ...) are not factory calls and pass through.  Poison 0xFF reads as NaN in
floats, -1 in signed and ~0 in unsigned integers; 0x00 is the page a fresh process usually gets.

The mode is thread-local state that autograd carries to its worker threads, so a tensor made inside an
autograd.Function.backward is guarded too (tests/test_guarded_alloc_host.py checks the count on the CPU, where backward
runs on the calling thread; tests/test_gpu_guard_bands.py checks it on the device thread)."""
import sys

import torch
from torch.utils._python_dispatch import TorchDispatchMode

aten = torch.ops.aten

EMPTY_OPS = (aten.empty.memory_format, aten.empty_strided.default, aten.empty_like.default, aten.new_empty.default)
FILLED_OPS = (aten.zeros.default, aten.zeros_like.default, aten.new_zeros.default, aten.ones.default,
              aten.full.default, aten.full_like.default, aten.new_full.default)
UPLOAD_OP = aten._to_copy.default


class _Record:
    __slots__ = ("raw", "nbytes", "op", "dtype", "shape", "where")

    def __init__(self, raw, nbytes, op, dtype, shape, where):
        self.raw, self.nbytes, self.op, self.dtype, self.shape, self.where = raw, nbytes, op, dtype, shape, where

    def __str__(self):
        return "%s -> %s%s allocated at %s" % (self.op, str(self.dtype).replace("torch.", ""), list(self.shape),
                                                self.where)


def _caller():
    """file:line (function) of the innermost Python frame that is neither torch's nor this module's."""
    f = sys._getframe(1)
    torch_dir = torch.__file__.rsplit("/", 1)[0]
    while f is not None:
        name = f.f_code.co_filename
        if name != __file__ and not name.startswith(torch_dir):
            return "%s:%d (%s)" % (name, f.f_lineno, f.f_code.co_name)
        f = f.f_back
    return "<no Python frame: autograd worker thread>"


class Guarded(TorchDispatchMode):
    def __init__(self, poison=0xFF, guard_bytes=65536, devices=("cuda",)):
        super().__init__()
        assert 0 <= poison <= 0xFF and guard_bytes > 0 and guard_bytes % 512 == 0
        self.poison, self.guard, self.devices = int(poison), int(guard_bytes), tuple(devices)
        self.records = []
        self._paused = False

    @property
    def count(self):
        """Number of guarded allocations so far."""
        return len(self.records)

    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        kwargs = kwargs or {}
        out = func(*args, **kwargs)
        if self._paused or not (func in EMPTY_OPS or func in FILLED_OPS or func is UPLOAD_OP):
            return out
        if not (isinstance(out, torch.Tensor) and out.device.type in self.devices and out.layout == torch.strided
                and out.numel() > 0 and out.is_contiguous() and not kwargs.get("pin_memory")):
            return out
        if func is UPLOAD_OP and args[0].device.type in self.devices:
            return out
        return self._guard(out, func, keep=func not in EMPTY_OPS)

    def _guard(self, out, func, keep):
        g, nbytes = self.guard, out.numel() * out.element_size()
        raw = torch.empty(g + nbytes + g, dtype=torch.uint8, device=out.device)
        raw.fill_(self.poison)
        mid = raw[g:g + nbytes].view(out.dtype).view(out.shape)
        if keep:
            mid.copy_(out)
        self.records.append(_Record(raw, nbytes, str(func), out.dtype, tuple(out.shape), _caller()))
        return mid

    def check(self):
        """Assert that every front and back band still holds the poison.  Synchronises the device."""
        self._paused = True
        try:
            if not self.records:
                return
            g = self.guard
            bands = [(r, side, band) for r in self.records
                     for side, band in (("front", r.raw[:g]), ("back", r.raw[g + r.nbytes:]))]
            hurt = [False] * len(bands)
            for dev in {band.device for _, _, band in bands}:          # one read back per device
                pos = [i for i, b in enumerate(bands) if b[2].device == dev]
                for i, bad in zip(pos, torch.stack([(bands[i][2] != self.poison).any() for i in pos]).cpu().tolist()):
                    hurt[i] = bad
            msgs = []
            for (r, side, band), bad in zip(bands, hurt):
                if not bad:
                    continue
                at = torch.nonzero(band != self.poison).flatten().cpu()
                first, last = int(at[0]), int(at[-1])
                if side == "front":                    # the byte nearest the payload tells how far in front it began
                    msgs.append("%d byte(s) damaged in FRONT of %s: first damaged offset %d, nearest %d byte(s) before the "
                                "payload's first byte" % (at.numel(), r, first - g, g - last))
                else:
                    msgs.append("%d byte(s) damaged BEHIND %s: first damaged offset %d, that is %d byte(s) past the "
                                "payload's last byte (%d bytes)" % (at.numel(), r, r.nbytes + first, first + 1, r.nbytes))
            assert not msgs, "guard band damaged:\n  " + "\n  ".join(msgs)
        finally:
            self._paused = False
