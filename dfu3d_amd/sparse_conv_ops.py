"""Sparse 3-D convolution on csrc/sparseconv_stage.hip (C ABI and every rule: csrc/dfu3d_spc.h): the index plan of a list
of SubMConv3d / SparseConv3d layers, and the convolution itself with both gradients behind one autograd.Function.

build_plan   indices int32 (N, 4) [b, z, y, x], count (device int), the layers -> Plan: the site set of every level, then
             ONE read from the device (every level's count and the status word), then each layer's neighbour and
             inverse table at exact size.  Layers with the same input level, kernel, stride and padding share tables.
sparse_conv  features (n_in, Cin), weight (Cout, kz, ky, kx, Cin), a layer's tables -> (n_out, Cout); differentiable in
             features and weight.  Nothing in it reads from the device.

float32 / int32 and contiguous, anything else raises Dfu3dError.  Every element of every output is written by the
kernels (torch.empty here), on the current stream."""
import collections
import ctypes

import torch

from . import _lib_spc
from ._lib import Dfu3dError
from .stages import _chk, _stream

K = _lib_spc.CONSTANTS
LAUNCHES_INDEX = K["DFU3D_SPC_LAUNCHES_INDEX"]
LAUNCHES_DOWNSAMPLE = K["DFU3D_SPC_LAUNCHES_DOWNSAMPLE"]
LAUNCHES_TABLES = K["DFU3D_SPC_LAUNCHES_TABLES"]
LAUNCHES_FORWARD = K["DFU3D_SPC_LAUNCHES_FORWARD"]
LAUNCHES_DGRAD = K["DFU3D_SPC_LAUNCHES_DGRAD"]
LAUNCHES_WGRAD = K["DFU3D_SPC_LAUNCHES_WGRAD"]
WGRAD_CHUNK = K["DFU3D_SPC_WGRAD_CHUNK"]
MAX_CHANNELS = K["DFU3D_SPC_MAX_CHANNELS"]
MAX_ROWS = K["DFU3D_SPC_MAX_ROWS"]
BAD_COORD = K["DFU3D_SPC_ST_BAD_COORD"]
DUP_SITE = K["DFU3D_SPC_ST_DUP_SITE"]
STATUS_TEXT = {BAD_COORD: "a row with a cell outside the spatial shape or a batch index outside the batch",
               DUP_SITE: "two rows in one cell"}

# a layer of a plan: the level it reads (0: the plan's input; j: the output of the j-th distinct strided layer), its
# geometry (3 ints each, z y x) and whether it is submanifold (output sites = input sites)
LayerSpec = collections.namedtuple("LayerSpec", "in_level kernel stride padding subm")
# a site set: indices (rows, 4) at exact size, count: its device int, table: the cell table while the plan is built
# (None in a finished plan), made for table_rows rows
Level = collections.namedtuple("Level", "indices count rows spatial_shape table table_rows")
LayerTables = collections.namedtuple("LayerTables", "nbr inv in_level out_level kv n_in n_out")
Plan = collections.namedtuple("Plan", "levels tables status batch_size host_reads")


def status_message(word):
    return "; ".join(t for b, t in STATUS_TEXT.items() if word & b) or "ok"


def _triple(v):
    t = tuple(int(e) for e in (v if isinstance(v, (tuple, list)) else (v, v, v)))
    if len(t) != 3:
        raise Dfu3dError("sparse_conv: a kernel size, stride or padding has 3 values (z, y, x), got %r" % (v,))
    return t


def layer(in_level, kernel, stride=1, padding=None, subm=False):
    """LayerSpec with whole numbers spread over the three axes; a submanifold layer has stride 1 and padding k // 2."""
    k = _triple(kernel)
    s = (1, 1, 1) if subm else _triple(stride)
    p = tuple(e // 2 for e in k) if subm else _triple(0 if padding is None else padding)
    return LayerSpec(int(in_level), k, s, p, bool(subm))


def output_shape(shape, kernel, stride, padding):
    """THE GEOMETRY of the header, per axis."""
    return tuple((d + 2 * p - k) // s + 1 for d, k, s, p in zip(shape, kernel, stride, padding))


def capacity(rows, batch_size, out_shape, kernel, stride):
    """THE CAPACITY BOUND of the header."""
    reach = 1
    for k, s in zip(kernel, stride):
        reach *= -(-k // s)
    return min(rows * reach, batch_size * out_shape[0] * out_shape[1] * out_shape[2])


def _i3(v):
    return ctypes.cast((ctypes.c_int32 * 3)(*v), ctypes.c_void_p), v


def _empty(dev, rows, *rest, dtype=torch.int32):
    # (a block of no rows still has an address the library may be given)
    return torch.empty((max(rows, 1),) + rest, dtype=dtype, device=dev)[:rows]


def _check_spec(spec, shape):
    k, s, p = spec.kernel, spec.stride, spec.padding
    if any(e not in (1, 3) for e in k) or any(e not in (1, 2) for e in s) or any(not 0 <= q < e for q, e in zip(p, k)):
        raise Dfu3dError("sparse_conv: kernel %s (1 or 3), stride %s (1 or 2), padding %s (0 .. k - 1)" % (k, s, p))
    if spec.subm and (any(e != 1 for e in s) or any(q != e // 2 for q, e in zip(p, k))):
        raise Dfu3dError("sparse_conv: a submanifold layer has stride 1 and padding k // 2, got %s, %s" % (s, p))
    out = output_shape(shape, k, s, p)
    if min(out) < 1:
        raise Dfu3dError("sparse_conv: kernel %s does not fit the shape %s with padding %s" % (k, tuple(shape), p))
    return out


def build_plan(indices, count, batch_size, spatial_shape, layers):
    """indices int32 (N, 4) [b, z, y, x] on the GPU, count: int32 (1) on the same GPU, rows at or beyond it are never
    read (None: all N); spatial_shape (D, H, W); layers: LayerSpecs in an order in which every in_level exists when it is
    read -> Plan.  Plan.levels[j].indices has exactly the level's rows; the features given to sparse_conv for a layer
    are the first Plan.levels[in_level].rows rows of what belongs to `indices`.  Plan.status: the DFU3D_SPC_ST_* bits."""
    if not isinstance(indices, torch.Tensor) or indices.dim() != 2 or indices.shape[1] != 4:
        raise Dfu3dError("build_plan: indices must have the shape (N, 4)")
    dev, N, B = indices.device, int(indices.shape[0]), int(batch_size)
    shape0 = tuple(int(e) for e in spatial_shape)
    if len(shape0) != 3 or min(shape0) < 1 or B < 1:
        raise Dfu3dError("build_plan: spatial_shape %r (3 values, 1 or more), batch_size %d (1 or more)" % (shape0, B))
    layers = [sp if isinstance(sp, LayerSpec) else layer(*sp) for sp in layers]
    L = _lib_spc.lib()
    st = _stream()
    n_levels = 1 + len({(sp.in_level, sp.kernel, sp.stride, sp.padding) for sp in layers if not sp.subm})
    word = torch.zeros(1 + n_levels, dtype=torch.int32, device=dev)         # status, then every level's count
    status = word[:1]
    if count is None:
        word[1:2].fill_(N)
    else:
        word[1:2].copy_(torch.clamp(count.reshape(1), 0, N))
    ip = _chk(indices, "build_plan: indices", torch.int32) if N else None

    def table_for(rows):
        nbytes = int(L.dfu3d_spc_table_bytes(rows))
        if nbytes == 0:
            raise Dfu3dError("build_plan: %d rows are out of range (DFU3D_ERANGE)" % rows)
        return torch.empty(nbytes, dtype=torch.uint8, device=dev), nbytes

    table, nbytes = table_for(N)
    c_shape, _ = _i3(shape0)
    _lib_spc.check(L.dfu3d_spc_index(ip, _chk(word[1:2], "count", torch.int32), N, B, c_shape,
                                     _chk(table, "table", torch.uint8), nbytes, _chk(status, "status", torch.int32), st),
                   "dfu3d_spc_index")
    # every level's geometry first (host arithmetic only): [capacity, shape], and what each new level is made from
    geom, made, out_level, todo = [[N, shape0]], {}, [], []
    for sp in layers:
        if not 0 <= sp.in_level < len(geom):
            raise Dfu3dError("build_plan: a layer reads level %d, %d exist so far" % (sp.in_level, len(geom)))
        rows_in, shape_in = geom[sp.in_level]
        out_shape = _check_spec(sp, shape_in)
        if sp.subm:
            out_level.append(sp.in_level)
            continue
        key = (sp.in_level, sp.kernel, sp.stride, sp.padding)
        if key not in made:
            kv = sp.kernel[0] * sp.kernel[1] * sp.kernel[2]
            cap = max(capacity(rows_in, B, out_shape, sp.kernel, sp.stride), 1)
            sbytes = int(L.dfu3d_spc_scratch_bytes(rows_in, cap, kv)) if cap <= MAX_ROWS else 0
            if sbytes == 0:
                raise Dfu3dError("build_plan: %d input rows, %d output rows at most are out of range (DFU3D_ERANGE)"
                                 % (rows_in, cap))
            made[key] = len(geom)
            geom.append([cap, out_shape])
            todo.append((sp, made[key], sbytes))
        out_level.append(made[key])
    # every level's site set; [indices at capacity, count view, capacity, shape, table].  ONE scratch for all of them, the
    # largest any needs: the calls follow each other on one stream
    raw = [[indices, word[1:2], N, shape0, table]]
    scratch = torch.empty(max([sb for _, _, sb in todo] + [16]), dtype=torch.uint8, device=dev)
    for sp, j, sbytes in todo:
        src, (cap, out_shape) = raw[sp.in_level], geom[j]
        out_idx = torch.empty((cap, 4), dtype=torch.int32, device=dev)
        out_table, tbytes = table_for(cap)
        rc = L.dfu3d_spc_downsample(
            _chk(src[0], "indices", torch.int32) if src[2] else None, _chk(src[1], "count", torch.int32), src[2],
            _chk(src[4], "table", torch.uint8), B, _i3(src[3])[0], _i3(sp.kernel)[0], _i3(sp.stride)[0],
            _i3(sp.padding)[0], cap, _chk(scratch, "scratch", torch.uint8), sbytes,
            _chk(out_idx, "out_indices", torch.int32), _chk(word[1 + j:2 + j], "out_count", torch.int32),
            _chk(out_table, "out_table", torch.uint8), tbytes, st)
        _lib_spc.check(rc, "dfu3d_spc_downsample")
        raw.append([out_idx, word[1 + j:2 + j], cap, out_shape, out_table])
    host = word.cpu().tolist()                                               # THE one read from the device
    del scratch
    # exact size from here on: a made level's rows are copied out of its capacity block, which is then let go
    levels = [Level(r[0][:host[1 + j]].clone() if j else r[0][:host[1 + j]], r[1], host[1 + j], r[3], r[4], r[2])
              for j, r in enumerate(raw)]
    del raw
    shared, tables = {}, []
    for sp, oj in zip(layers, out_level):
        key = (sp.in_level, sp.kernel, sp.stride, sp.padding, sp.subm)
        if key not in shared:
            lin, lout = levels[sp.in_level], levels[oj]
            kv = sp.kernel[0] * sp.kernel[1] * sp.kernel[2]
            nbr, inv = _empty(dev, lout.rows, kv), _empty(dev, lin.rows, kv)
            rc = L.dfu3d_spc_tables(
                lin.rows, _chk(lin.table, "table", torch.uint8), lin.table_rows,
                _chk(lout.indices, "out_indices", torch.int32) if lout.rows else None,
                _chk(lout.count, "out_count", torch.int32), lout.rows, _chk(lout.table, "table", torch.uint8),
                lout.table_rows, B, _i3(lin.spatial_shape)[0], _i3(sp.kernel)[0], _i3(sp.stride)[0], _i3(sp.padding)[0],
                _chk(nbr, "nbr", torch.int32) if lout.rows else None, _chk(inv, "inv", torch.int32) if lin.rows else None,
                st)
            _lib_spc.check(rc, "dfu3d_spc_tables")
            shared[key] = LayerTables(nbr, inv, sp.in_level, oj, kv, lin.rows, lout.rows)
        tables.append(shared[key])
    # the cell tables have done their work: the plan keeps the levels without them
    levels = [lv._replace(table=None) for lv in levels]
    return Plan(levels, tables, host[0], B, 1)


def _weight_dims(w, kv):
    if w.dim() != 5 or w.shape[1] * w.shape[2] * w.shape[3] != kv:
        raise Dfu3dError("sparse_conv: weight (Cout, kz, ky, kx, Cin) with kz * ky * kx = %d, got %s"
                         % (kv, tuple(w.shape)))
    cout, cin = int(w.shape[0]), int(w.shape[4])
    if not (1 <= cin <= MAX_CHANNELS and 1 <= cout <= MAX_CHANNELS):
        raise Dfu3dError("sparse_conv: %d -> %d channels, at most %d (DFU3D_ERANGE)" % (cin, cout, MAX_CHANNELS))
    return cin, cout


def conv_forward(x, w, t):
    """THE SUM of the header: x float32 (t.n_in, Cin), w float32 (Cout, kz, ky, kx, Cin) -> y float32 (t.n_out, Cout)."""
    cin, cout = _weight_dims(w, t.kv)
    if x.dim() != 2 or tuple(x.shape) != (t.n_in, cin):
        raise Dfu3dError("sparse_conv: features %s, the layer reads (%d, %d)" % (tuple(x.shape), t.n_in, cin))
    y = _empty(x.device, t.n_out, cout, dtype=torch.float32)
    rc = _lib_spc.lib().dfu3d_spc_forward(
        _chk(x, "sparse_conv: features", torch.float32) if t.n_in else None, t.n_in,
        _chk(t.nbr, "nbr", torch.int32) if t.n_out else None, t.n_out, t.kv, _chk(w, "sparse_conv: weight", torch.float32),
        cin, cout, _chk(y, "y", torch.float32) if t.n_out else None, _stream())
    _lib_spc.check(rc, "dfu3d_spc_forward")
    return y


def conv_dgrad(dy, w, t):
    """THE FEATURE GRADIENT: dy float32 (t.n_out, Cout) -> dx float32 (t.n_in, Cin)."""
    cin, cout = _weight_dims(w, t.kv)
    if tuple(dy.shape) != (t.n_out, cout):
        raise Dfu3dError("sparse_conv: the output gradient %s, the layer writes (%d, %d)" % (tuple(dy.shape), t.n_out, cout))
    dx = _empty(dy.device, t.n_in, cin, dtype=torch.float32)
    rc = _lib_spc.lib().dfu3d_spc_dgrad(
        _chk(dy, "sparse_conv: dy", torch.float32) if t.n_out else None, t.n_out,
        _chk(t.inv, "inv", torch.int32) if t.n_in else None, t.n_in, t.kv, _chk(w, "sparse_conv: weight", torch.float32),
        cin, cout, _chk(dx, "dx", torch.float32) if t.n_in else None, _stream())
    _lib_spc.check(rc, "dfu3d_spc_dgrad")
    return dx


def conv_wgrad(x, dy, t, weight_shape):
    """THE WEIGHT GRADIENT: -> dw float32 of weight_shape (Cout, kz, ky, kx, Cin)."""
    cout, cin = int(weight_shape[0]), int(weight_shape[4])
    if tuple(x.shape) != (t.n_in, cin) or tuple(dy.shape) != (t.n_out, cout):
        raise Dfu3dError("sparse_conv: features %s and output gradient %s do not fit the layer" % (tuple(x.shape), tuple(dy.shape)))
    L = _lib_spc.lib()
    dw = torch.empty(tuple(weight_shape), dtype=torch.float32, device=x.device)
    nbytes = int(L.dfu3d_spc_wgrad_scratch_bytes(t.n_out, t.kv, cin, cout))
    scratch = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=x.device)
    rc = L.dfu3d_spc_wgrad(
        _chk(x, "sparse_conv: features", torch.float32) if t.n_in else None, t.n_in,
        _chk(dy, "sparse_conv: dy", torch.float32) if t.n_out else None,
        _chk(t.nbr, "nbr", torch.int32) if t.n_out else None, t.n_out, t.kv, cin, cout,
        _chk(scratch, "scratch", torch.uint8), nbytes, _chk(dw, "dw", torch.float32), _stream())
    _lib_spc.check(rc, "dfu3d_spc_wgrad")
    return dw


class _SparseConv(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, t):
        x, w = x.contiguous(), w.contiguous()
        ctx.t = t
        ctx.save_for_backward(x, w)
        return conv_forward(x, w, t)

    @staticmethod
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        dy = dy.contiguous()
        dx = conv_dgrad(dy, w, ctx.t) if ctx.needs_input_grad[0] else None
        dw = conv_wgrad(x, dy, ctx.t, w.shape) if ctx.needs_input_grad[1] else None
        return dx, dw, None


def sparse_conv(features, weight, tables):
    """features float32 (tables.n_in, Cin), weight float32 (Cout, kz, ky, kx, Cin) -> (tables.n_out, Cout), with the
    gradients of the header behind it.  No bias."""
    return _SparseConv.apply(features, weight, tables)
