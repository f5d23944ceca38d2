"""The fused optimiser step on csrc/optim_stage.hip (C ABI and numerics contract: include/dfu3d_opt.h).

`FusedAdamStep(params, exp_avg, exp_avg_sq)` owns the tensor table and the chunk map of a parameter list and runs
dfu3d_adam_step on them: gradient clipping by the global norm, true weight decay and the Adam update of every tensor in
DFU3D_OPT_LAUNCHES launches, no host read.  The table is built in pinned host memory and uploaded with one asynchronous
copy on the current stream.  It holds raw device addresses, so the object keeps a reference to every tensor whose
address is in it and compares the tuple of data_ptr()s -- gradients included -- before EVERY call; when one has moved
(a gradient replaced by a new tensor, `param.data` reassigned) the table is rebuilt and uploaded again.  All calls of one
object are expected on one stream.  Parameters, gradients and moments must be float32, contiguous and on one GPU (mixed
precision is out of scope); anything else raises Dfu3dError."""
import ctypes

import numpy as np
import torch

from . import _lib_opt
from ._lib import Dfu3dError

K = _lib_opt.CONSTANTS
CHUNK = K["DFU3D_OPT_CHUNK"]
LAUNCHES = K["DFU3D_OPT_LAUNCHES"]
ST_NONFINITE = K["DFU3D_OPT_ST_NONFINITE"]
MAX_TENSORS = K["DFU3D_OPT_MAX_TENSORS"]
MAX_CHUNKS = K["DFU3D_OPT_MAX_CHUNKS"]
MAX_LEN = K["DFU3D_OPT_MAX_LEN"]
TENSOR_WORDS = ctypes.sizeof(_lib_opt.STRUCTS["dfu3d_opt_tensor"]) // 8       # int64 words of a table record

STATUS_TEXT = {ST_NONFINITE: "the sum of the squared gradients is not finite"}


def status_message(s):
    return "; ".join(t for b, t in STATUS_TEXT.items() if s & b)


def chunk_map(lengths):
    """The chunk map of tensors of these lengths: int32 (n_chunks, 2) rows [tensor, start], tensor after tensor."""
    rows = [(i, s) for i, n in enumerate(lengths) for s in range(0, int(n), CHUNK)]
    return np.array(rows, np.int32).reshape(-1, 2)


def _check_tensor(t, what, device=None, numel=None):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise Dfu3dError("adam_step: %s must be a tensor on the GPU" % what)
    if t.dtype != torch.float32 or not t.is_contiguous():
        raise Dfu3dError("adam_step: %s must be float32 and contiguous, got %s, strides %s" % (what, t.dtype, t.stride()))
    if device is not None and t.device != device:
        raise Dfu3dError("adam_step: %s is on %s, the first parameter on %s" % (what, t.device, device))
    if numel is not None and t.numel() != numel:
        raise Dfu3dError("adam_step: %s has %d elements, its parameter %d" % (what, t.numel(), numel))
    if not 1 <= t.numel() <= MAX_LEN:
        raise Dfu3dError("adam_step: %s has %d elements, between 1 and %d" % (what, t.numel(), MAX_LEN))
    if t.data_ptr() % 4:
        raise Dfu3dError("adam_step: %s is not 4-byte aligned" % what)


class FusedAdamStep:
    """params: the tensors to update (their .grad is looked up at every call; None: no gradient in that call);
    exp_avg, exp_avg_sq: the moments, one per parameter.  After a call `norm` (2 doubles on the device) holds
    [total_norm, coef] and `status` (1 int32 on the device) has the DFU3D_OPT_ST_* bits of all calls ORed in."""

    def __init__(self, params, exp_avg, exp_avg_sq, names=None):
        self.params, self.exp_avg, self.exp_avg_sq = list(params), list(exp_avg), list(exp_avg_sq)
        n = len(self.params)
        self.names = list(names) if names is not None else ["parameter %d" % i for i in range(n)]
        if not 1 <= n <= MAX_TENSORS or len(self.exp_avg) != n or len(self.exp_avg_sq) != n or len(self.names) != n:
            raise Dfu3dError("adam_step: %d parameters (1 .. %d) with %d and %d moments"
                             % (n, MAX_TENSORS, len(self.exp_avg), len(self.exp_avg_sq)))
        for i, p in enumerate(self.params):
            _check_tensor(p, self.names[i])
        self.device = self.params[0].device
        self._check_all()
        self.lengths = [p.numel() for p in self.params]
        self._chunks = chunk_map(self.lengths)
        self.n_chunks = len(self._chunks)
        if self.n_chunks > MAX_CHUNKS:
            raise Dfu3dError("adam_step: %d chunks, at most %d" % (self.n_chunks, MAX_CHUNKS))
        L = _lib_opt.lib()
        words = n * TENSOR_WORDS + self.n_chunks
        self._table = torch.empty(words, dtype=torch.int64, device=self.device)
        self._scratch = torch.empty(L.dfu3d_opt_scratch_bytes(self.n_chunks) // 8, dtype=torch.float64, device=self.device)
        self.norm = torch.zeros(2, dtype=torch.float64, device=self.device)
        self.status = torch.zeros(1, dtype=torch.int32, device=self.device)
        self._key = None
        self._held = None
        self.uploads = 0

    def _check_all(self):
        for i, p in enumerate(self.params):
            _check_tensor(p, self.names[i], self.device)
            _check_tensor(self.exp_avg[i], "exp_avg of " + self.names[i], self.device, p.numel())
            _check_tensor(self.exp_avg_sq[i], "exp_avg_sq of " + self.names[i], self.device, p.numel())

    def _upload(self, grads, key):
        self._check_all()
        if [p.numel() for p in self.params] != self.lengths:
            raise Dfu3dError("adam_step: a parameter has changed its length")
        for i, g in enumerate(grads):
            if g is not None:
                _check_tensor(g, "the gradient of " + self.names[i], self.device, self.lengths[i])
        n = len(self.params)
        # a fresh pinned block per upload: the one before may still be the source of a copy in flight (the allocator
        # of pinned memory hands a block out again only after the copies that read it)
        host = torch.empty(self._table.numel(), dtype=torch.int64, pin_memory=True)
        h = host.numpy()
        h[:n * TENSOR_WORDS].reshape(n, TENSOR_WORDS)[:] = np.array(
            [[key[4 * i], key[4 * i + 1], key[4 * i + 2], key[4 * i + 3], self.lengths[i]] for i in range(n)], np.int64)
        h[n * TENSOR_WORDS:].view(np.int32).reshape(-1, 2)[:] = self._chunks
        self._table.copy_(host, non_blocking=True)
        # the table names these addresses: they stay alive as long as it does
        self._held = (list(self.params), list(grads), list(self.exp_avg), list(self.exp_avg_sq))
        self._key = key
        self.uploads += 1

    def step(self, lr, beta1, beta2, eps, weight_decay, max_norm, bias_correction1, bias_correction2):
        grads = [p.grad for p in self.params]
        key = tuple(a for i, p in enumerate(self.params)
                    for a in (p.data_ptr(), 0 if grads[i] is None else grads[i].data_ptr(), self.exp_avg[i].data_ptr(),
                              self.exp_avg_sq[i].data_ptr()))
        if key != self._key:
            self._upload(grads, key)
        n = len(self.params)
        base = self._table.data_ptr()
        rc = _lib_opt.lib().dfu3d_adam_step(
            ctypes.c_void_p(base), n, ctypes.c_void_p(base + 8 * n * TENSOR_WORDS), self.n_chunks, float(lr), float(beta1),
            float(beta2), float(eps), float(weight_decay), float(max_norm), float(bias_correction1), float(bias_correction2),
            ctypes.c_void_p(self._scratch.data_ptr()), ctypes.c_void_p(self.norm.data_ptr()),
            ctypes.c_void_p(self.status.data_ptr()), ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream))
        _lib_opt.check(rc, "dfu3d_adam_step")

    def check_status(self):
        """One host read of the status word; raises Dfu3dError on any bit and clears the word."""
        s = int(self.status.item())
        if s:
            self.status.zero_()
            raise Dfu3dError("adam_step: status %d (%s)" % (s, status_message(s)))
