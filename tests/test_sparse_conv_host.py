"""The sparse-convolution stage without a GPU.  THE INDEPENDENT PIN: the restatement of csrc/dfu3d_spc.h
(tests/sparse_conv_ref.py) against torch.nn.functional.conv3d in float64 on the dense canvas -- site sets, row order,
y, dx and dw of all five layer geometries of the voxel backbones.  Then the exact fmaf of the restatement against
libm's, the agreement of the header with its binding, host-side argument validation before any launch, the scratch
sizes, the shape arithmetic, the backbones' state-dict keys and the 1.x weight layout."""
import ctypes
import ctypes.util
import json
import os

import numpy as np
import pytest

from dfu3d_amd import _build, _lib, _lib_spc
from tests import sparse_conv_ref as R

f32 = np.float32
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g24_spconv_backbone_keys.json")
# the five layers of the backbones: kernel, stride, padding, submanifold
LAYERS = [((3, 3, 3), (1, 1, 1), (1, 1, 1), True), ((3, 3, 3), (2, 2, 2), (1, 1, 1), False),
          ((3, 3, 3), (2, 2, 2), (0, 1, 1), False), ((3, 1, 1), (2, 1, 1), (0, 0, 0), False),
          ((3, 1, 1), (2, 1, 1), (1, 0, 0), False)]
SYMBOLS = ['dfu3d_spc_dgrad', 'dfu3d_spc_downsample', 'dfu3d_spc_forward', 'dfu3d_spc_index', 'dfu3d_spc_scratch_bytes',
           'dfu3d_spc_table_bytes', 'dfu3d_spc_tables', 'dfu3d_spc_version', 'dfu3d_spc_wgrad',
           'dfu3d_spc_wgrad_scratch_bytes']


# ---- the exact fmaf ------------------------------------------------------------------------------------------------------
def libm_fmaf(a, b, c):
    libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
    libm.fmaf.restype = ctypes.c_float
    libm.fmaf.argtypes = [ctypes.c_float] * 3
    return np.array([libm.fmaf(float(u), float(v), float(t)) for u, v, t in zip(a, b, c)], f32)


def test_fmaf_against_libm_on_random_and_halfway_cases():
    rng = np.random.default_rng(0)
    a, b, c = (rng.standard_normal(30000).astype(f32) for _ in range(3))
    c = (c * np.exp2(rng.integers(-40, 40, 30000))).astype(f32)
    assert R.fmaf(a, b, c).tobytes() == libm_fmaf(a, b, c).tobytes()
    # Halfway cases.  With e = 2^-12, (1 + e) * (1 - e + e^2) = 1 + e^3 exactly, both factors float32; so
    # a * b = 2^-24 * (1 + 2^-36) and a * b + 1 = 1 + 2^-24 + 2^-60 lies just ABOVE the midpoint of 1 and 1 + 2^-23: fmaf
    # gives 1 + 2^-23.  A float64 add drops the 2^-60, lands on the midpoint, and the cast (ties to even) gives 1.
    e = 2.0 ** -12
    a1, b1 = f32(1 + e), f32((1 - e + e * e) * 2.0 ** -24)
    assert float(a1) * float(b1) == 2.0 ** -24 * (1 + 2.0 ** -36)
    cases = [(a1, b1, f32(1)), (-a1, b1, f32(-1)), (a1, f32(float(b1) * 2.0 ** 10), f32(2.0 ** 10)),
             (f32(1), f32(2.0 ** -24), f32(1)), (f32(1), f32(2.0 ** -24), f32(1 + 2.0 ** -23)),   # exact ties: to even
             (f32(3), f32(2.0 ** -25), f32(1)), (f32(1e-30), f32(1e-30), f32(0)),
             (f32(2.0 ** -100), f32(2.0 ** -30), f32(2.0 ** -149)), (f32(-1), f32(2.0 ** -140), f32(2.0 ** -149))]
    x = np.array([t[0] for t in cases], f32)
    y = np.array([t[1] for t in cases], f32)
    z = np.array([t[2] for t in cases], f32)
    want = libm_fmaf(x, y, z)
    assert R.fmaf(x, y, z).tobytes() == want.tobytes()
    plain = (x.astype(np.float64) * y.astype(np.float64) + z.astype(np.float64)).astype(f32)
    assert (plain.view(np.uint32) != want.view(np.uint32)).any()                   # the add-then-cast form IS wrong here


# ---- the independent pin ------------------------------------------------------------------------------------------------
def face_and_corner_sites(rng, B, shape, n):
    """n random cells and every corner, plus a cell on each face, of every scene; distinct, in random order."""
    D, H, W = shape
    fixed = [(b, z, y, x) for b in range(B) for z in (0, D - 1) for y in (0, H - 1) for x in (0, W - 1)]
    fixed += [(b, D // 2, H // 2, x) for b in range(B) for x in (0, W - 1)]
    fixed += [(b, D // 2, y, W // 2) for b in range(B) for y in (0, H - 1)]
    fixed += [(b, z, H // 2, W // 2) for b in range(B) for z in (0, D - 1)]
    ids = rng.permutation(B * D * H * W)[:n]
    rnd = np.stack([ids // (D * H * W), (ids // (H * W)) % D, (ids // W) % H, ids % W], 1)
    idx = np.unique(np.concatenate([np.array(fixed), rnd]), axis=0)
    return idx[rng.permutation(len(idx))].astype(np.int32)


@pytest.mark.parametrize("case", range(len(LAYERS)))
def test_the_restatement_against_a_dense_float64_convolution(case):
    import torch
    import torch.nn.functional as F
    k, s, p, subm = LAYERS[case]
    rng = np.random.default_rng(100 + case)
    B, shape, cin, cout = 2, (7, 6, 8), 5, 6
    idx = face_and_corner_sites(rng, B, shape, 110)
    levels, tabs, status = R.plan(idx, len(idx), B, shape, [(0, k, s, p, subm)])
    nbr, inv, _, lout = tabs[0]
    oidx, osh = levels[lout]
    assert status == 0 and osh == R.out_shape(shape, k, s, p)
    x = rng.standard_normal((len(idx), cin)).astype(f32)
    w = rng.standard_normal((cout,) + k + (cin,)).astype(f32)
    dy = rng.standard_normal((len(oidx), cout)).astype(f32)
    wf = w.reshape(cout, -1, cin)

    def canvas(rows, feats, sh):
        c = torch.zeros((B, feats.shape[1]) + tuple(sh), dtype=torch.float64)
        c[rows[:, 0], :, rows[:, 1], rows[:, 2], rows[:, 3]] = torch.from_numpy(feats).double()
        return c

    def at(c, rows):
        return c[rows[:, 0], :, rows[:, 1], rows[:, 2], rows[:, 3]].detach().numpy()
    dense = canvas(idx, x, shape).requires_grad_(True)
    wt = torch.from_numpy(w).double().permute(0, 4, 1, 2, 3).contiguous().requires_grad_(True)
    out = F.conv3d(dense, wt, stride=s, padding=p)
    assert tuple(out.shape[2:]) == tuple(osh)
    # the site set: the cells with an input in their window (strided), the input cells (submanifold); the order: first seen
    occupied = canvas(idx, np.ones((len(idx), 1), f32), shape)
    window = F.conv3d(occupied, torch.ones((1, 1) + k, dtype=torch.float64), stride=s, padding=p)[:, 0] > 0
    mask = torch.zeros_like(window)
    mask[oidx[:, 0], oidx[:, 1], oidx[:, 2], oidx[:, 3]] = True
    assert len(np.unique(oidx, axis=0)) == len(oidx)
    if subm:
        assert np.array_equal(oidx, idx)
    else:
        assert (mask == window).all()
        # a cell outside the set is exactly 0 for bias-free weights
        assert not out.detach()[~mask[:, None].expand_as(out)].any()
        first = {}
        for i, cell in enumerate(idx.tolist()):
            for K, j in enumerate(R.offsets(k)):
                t = [cell[1 + a] + p[a] - j[a] for a in range(3)]
                if all(t[a] >= 0 and t[a] % s[a] == 0 and t[a] // s[a] < osh[a] for a in range(3)):
                    first.setdefault((cell[0],) + tuple(t[a] // s[a] for a in range(3)), (i, K))
        assert [tuple(r) for r in oidx.tolist()] == sorted(first, key=first.get)
    # nbr[o][K] == i exactly when inv[i][K] == o
    o_, K_ = np.nonzero(nbr >= 0)
    assert (inv[nbr[o_, K_], K_] == o_).all() and (nbr >= 0).sum() == (inv >= 0).sum() > 0
    # values within gamma_n * sum |x w|, the sum of absolute values by the same dense convolution
    def gamma(n):
        return n * 2.0 ** -24 / (1 - n * 2.0 ** -24)
    kv = k[0] * k[1] * k[2]
    y = R.forward(x, nbr, wf)
    mag = F.conv3d(dense.detach().abs(), wt.detach().abs(), stride=s, padding=p)
    assert (np.abs(y.astype(np.float64) - at(out, oidx)) <= gamma(kv * cin) * at(mag, oidx)).all()
    g = canvas(oidx, dy, osh)                                # (the output cells that are no sites have no gradient)
    out.backward(g)
    dxs = R.dgrad(dy, inv, wf)
    dws = R.wgrad(x, dy, nbr).reshape(w.shape)
    da = dense.detach().abs().requires_grad_(True)
    wa = wt.detach().abs().requires_grad_(True)
    F.conv3d(da, wa, stride=s, padding=p).backward(g.abs())
    assert (np.abs(dxs.astype(np.float64) - at(dense.grad, idx)) <= gamma(kv * cout) * at(da.grad, idx)).all()
    dw_ref, dw_mag = (t.grad.permute(0, 2, 3, 4, 1).numpy() for t in (wt, wa))
    assert (np.abs(dws.astype(np.float64) - dw_ref) <= gamma(len(oidx)) * dw_mag).all()
    assert np.abs(y).max() > 0 and np.abs(dxs).max() > 0 and np.abs(dws).max() > 0


def test_the_restatement_on_bad_rows_duplicates_and_chunks():
    idx = np.array([[0, 1, 1, 1], [0, 1, 1, 2], [0, 1, 1, 1], [1, 0, 0, 0], [0, 3, 0, 0], [0, 1, 1, 0], [-1] * 4], np.int32)
    levels, tabs, status = R.plan(idx, 6, 1, (3, 3, 3), [(0,) + LAYERS[0], (0,) + LAYERS[1]])
    assert status == R.BAD_COORD | R.DUP_SITE and len(levels[0][0]) == 6
    nbr, inv = tabs[0][:2]
    assert nbr[0, 13] == 0 and nbr[0, 14] == 1 and nbr[0, 12] == 5 and (nbr[[2, 3, 4]] == -1).all()
    assert not np.isin(nbr, [2, 3, 4]).any() and inv[1, 14] == 0 and inv[5, 12] == 0 and (inv[[2, 3, 4]] == -1).all()
    # row 0 at (1, 1, 1) of a 3^3 shape, stride 2, padding 1: t = in + 1 - j is even for j = 0 (o = 1) and j = 2 (o = 0),
    # K ascending: (jz, jy, jx) = (0, 0, 0) first -> o = (1, 1, 1), then (0, 0, 2) -> (1, 1, 0), ...
    assert levels[1][1] == (2, 2, 2) and levels[1][0][:3].tolist() == [[0, 1, 1, 1], [0, 1, 1, 0], [0, 1, 0, 1]]
    assert len(levels[1][0]) == 8
    # the chunked weight gradient: two chunks of 3 rows and one of 1 against one chain over all rows, which differs
    rng = np.random.default_rng(5)
    x, dy = rng.standard_normal((7, 2)).astype(f32), rng.standard_normal((7, 3)).astype(f32)
    tab = np.arange(7, dtype=np.int32)[:, None]
    a, b = R.wgrad(x, dy, tab, chunk=3), R.wgrad(x, dy, tab, chunk=7)
    parts = [R.wgrad(x[o:o + 3], dy[o:o + 3], np.arange(len(x[o:o + 3]), dtype=np.int32)[:, None], chunk=3) for o in (0, 3, 6)]
    assert a.tobytes() == (parts[0].astype(np.float64) + parts[1] + parts[2]).astype(f32).tobytes()
    assert np.allclose(a, b, rtol=1e-5, atol=1e-6) and R.WGRAD_CHUNK == _lib_spc.CONSTANTS['DFU3D_SPC_WGRAD_CHUNK']


# ---- header, binding, validation ------------------------------------------------------------------------------------------
def test_header_and_binding_agree():
    assert _lib_spc.HEADER == os.path.join(_build.CSRC, "dfu3d_spc.h") and _lib_spc.HEADER in _build._deps()
    assert os.path.join(_build.CSRC, "sparseconv_stage.hip") in _build.sources()
    assert _lib_spc.header_symbols() == SYMBOLS
    L = _lib_spc.lib()
    assert all(hasattr(L, s) for s in SYMBOLS) and L.dfu3d_spc_version() == _lib_spc.header_version() == 1
    K = _lib_spc.CONSTANTS
    assert K == {'DFU3D_SPC_VERSION': 1, 'DFU3D_SPC_LAUNCHES_INDEX': 2, 'DFU3D_SPC_LAUNCHES_DOWNSAMPLE': 5,
                 'DFU3D_SPC_LAUNCHES_TABLES': 2, 'DFU3D_SPC_LAUNCHES_FORWARD': 1, 'DFU3D_SPC_LAUNCHES_DGRAD': 1,
                 'DFU3D_SPC_LAUNCHES_WGRAD': 2, 'DFU3D_SPC_WGRAD_CHUNK': 1024, 'DFU3D_SPC_MAX_CHANNELS': 256,
                 'DFU3D_SPC_MAX_KV': 27, 'DFU3D_SPC_KEY_BITS': 62, 'DFU3D_SPC_MAX_ROWS': 2 ** 26, 'DFU3D_SPC_MAX_BATCH': 65535,
                 'DFU3D_SPC_TABLE_PER_ROW': 2, 'DFU3D_SPC_ST_BAD_COORD': 1, 'DFU3D_SPC_ST_DUP_SITE': 2,
                 'DFU3D_SPC_ROW_THREADS': 1024, 'DFU3D_SPC_GEMM_THREADS': 256, 'DFU3D_SPC_WGRAD_THREADS': 64,
                 'DFU3D_SPC_TILE_K': 32}
    assert (R.BAD_COORD, R.DUP_SITE) == (1, 2)
    i32, vp, sz = ctypes.c_int32, ctypes.c_void_p, ctypes.c_size_t
    S = _lib_spc.SIGNATURES
    assert S['dfu3d_spc_scratch_bytes'] == (sz, [i32] * 3) and S['dfu3d_spc_table_bytes'] == (sz, [i32])
    assert S['dfu3d_spc_wgrad_scratch_bytes'] == (sz, [i32] * 4)                   # rows, offsets, channels: no launch size
    assert S['dfu3d_spc_forward'] == (i32, [vp, i32, vp, i32, i32, vp, i32, i32, vp, vp])
    assert S['dfu3d_spc_dgrad'] == S['dfu3d_spc_forward']
    assert S['dfu3d_spc_wgrad'] == (i32, [vp, i32, vp, vp, i32, i32, i32, i32, vp, sz, vp, vp])
    assert S['dfu3d_spc_index'] == (i32, [vp, vp, i32, i32, vp, vp, sz, vp, vp])
    assert len(S['dfu3d_spc_downsample'][1]) == 17 and len(S['dfu3d_spc_tables'][1]) == 16
    from dfu3d_amd import sparse_conv_ops as ops
    assert ops.status_message(0) == "ok" and "outside" in ops.status_message(1) and "one cell" in ops.status_message(3)
    assert ops.WGRAD_CHUNK == 1024 and ops.MAX_CHANNELS == 256


def P(k):
    return ctypes.c_void_p(16 * (k + 1))                                           # an address no call may touch


def i3(*v):
    return ctypes.cast((ctypes.c_int32 * 3)(*v), ctypes.c_void_p)


def test_bad_arguments_return_before_any_launch():
    """Every call passes device pointers no kernel may touch: a launch would fault (or, without a GPU, fail with
    DFU3D_ELAUNCH); each must come back with the validation's own code."""
    L = _lib_spc.lib()
    OK, EINVAL, ERANGE = (_lib.CONSTANTS[k] for k in ("DFU3D_OK", "DFU3D_EINVAL", "DFU3D_ERANGE"))
    K = _lib_spc.CONSTANTS
    big = 1 << 40

    def index(indices=P(0), count=P(1), N=100, B=2, shape=(41, 1600, 1408), table=P(2), nbytes=big, status=P(3)):
        return L.dfu3d_spc_index(indices, count, N, B, i3(*shape), table, nbytes, status, None)
    for name in ("indices", "count", "table", "status"):
        assert index(**{name: None}) == EINVAL, name
    assert L.dfu3d_spc_index(P(0), P(1), 100, 2, None, P(2), big, P(3), None) == EINVAL
    assert index(N=-1) == EINVAL and index(B=0) == EINVAL and index(shape=(0, 4, 4)) == EINVAL and index(shape=(4, 4, -1)) == EINVAL
    assert index(table=ctypes.c_void_p(24)) == EINVAL and index(indices=ctypes.c_void_p(20)) == EINVAL
    assert index(nbytes=L.dfu3d_spc_table_bytes(100) - 1) == EINVAL
    assert index(N=K['DFU3D_SPC_MAX_ROWS'] + 1) == ERANGE and index(B=K['DFU3D_SPC_MAX_BATCH'] + 1) == ERANGE
    assert index(B=1, shape=(2 ** 20, 2 ** 21, 2 ** 21)) == ERANGE and index(B=65535, shape=(2 ** 31 - 1,) * 3) == ERANGE

    def down(N_in=100, cap=800, B=2, shape=(41, 1600, 1408), k=(3, 3, 3), s=(2, 2, 2), p=(1, 1, 1), sbytes=big, tbytes=big, **ptr):
        a = dict(in_indices=P(0), in_count=P(1), in_table=P(2), scratch=P(3), out_indices=P(4), out_count=P(5), out_table=P(6))
        a.update(ptr)
        return L.dfu3d_spc_downsample(a['in_indices'], a['in_count'], N_in, a['in_table'], B, i3(*shape), i3(*k), i3(*s),
                                      i3(*p), cap, a['scratch'], sbytes, a['out_indices'], a['out_count'], a['out_table'],
                                      tbytes, None)
    for name in ("in_indices", "in_count", "in_table", "scratch", "out_indices", "out_count", "out_table"):
        assert down(**{name: None}) == EINVAL, name
    assert down(N_in=-1) == EINVAL and down(cap=0) == EINVAL and down(cap=799) == EINVAL       # below THE CAPACITY BOUND
    assert down(k=(2, 3, 3)) == EINVAL and down(k=(5, 3, 3)) == EINVAL and down(s=(3, 2, 2)) == EINVAL and down(s=(0, 1, 1)) == EINVAL
    assert down(p=(3, 1, 1)) == EINVAL and down(p=(-1, 1, 1)) == EINVAL and down(k=(1, 1, 1), p=(1, 0, 0)) == EINVAL
    assert down(shape=(2, 8, 8), p=(0, 1, 1)) == EINVAL                                    # the kernel does not fit
    assert down(sbytes=L.dfu3d_spc_scratch_bytes(100, 800, 27) - 1) == EINVAL
    assert down(tbytes=L.dfu3d_spc_table_bytes(800) - 1) == EINVAL and down(scratch=ctypes.c_void_p(8)) == EINVAL
    assert down(N_in=K['DFU3D_SPC_MAX_ROWS'] + 1, cap=K['DFU3D_SPC_MAX_ROWS']) == ERANGE
    assert down(N_in=2 ** 26, cap=2 ** 26 + 1) == ERANGE and down(B=70000) == ERANGE

    def tables(N_in=100, in_rows=100, N_out=100, out_rows=100, B=2, shape=(41, 1600, 1408), k=(3, 3, 3), s=(1, 1, 1),
               p=(1, 1, 1), **ptr):
        a = dict(in_table=P(0), out_indices=P(1), out_count=P(2), out_table=P(3), nbr=P(4), inv=P(5))
        a.update(ptr)
        return L.dfu3d_spc_tables(N_in, a['in_table'], in_rows, a['out_indices'], a['out_count'], N_out, a['out_table'],
                                  out_rows, B, i3(*shape), i3(*k), i3(*s), i3(*p), a['nbr'], a['inv'], None)
    for name in ("in_table", "out_indices", "out_count", "out_table", "nbr", "inv"):
        assert tables(**{name: None}) == EINVAL, name
    assert tables(N_in=-1) == EINVAL and tables(N_out=-1) == EINVAL and tables(in_rows=99) == EINVAL and tables(out_rows=99) == EINVAL
    assert tables(k=(3, 3, 4)) == EINVAL and tables(B=0) == EINVAL and tables(in_rows=2 ** 26 + 1) == ERANGE

    def gemm(fn, N_in=100, N_out=90, KV=27, cin=16, cout=32, **ptr):
        a = dict(src=P(0), tab=P(1), w=P(2), out=P(3))
        a.update(ptr)
        if fn == "forward":
            return L.dfu3d_spc_forward(a['src'], N_in, a['tab'], N_out, KV, a['w'], cin, cout, a['out'], None)
        return L.dfu3d_spc_dgrad(a['src'], N_out, a['tab'], N_in, KV, a['w'], cin, cout, a['out'], None)
    for fn in ("forward", "dgrad"):
        for name in ("src", "tab", "w", "out"):
            assert gemm(fn, **{name: None}) == EINVAL, (fn, name)
        assert gemm(fn, N_in=-1) == EINVAL and gemm(fn, N_out=-1) == EINVAL and gemm(fn, KV=0) == EINVAL and gemm(fn, KV=28) == EINVAL
        assert gemm(fn, cin=0) == EINVAL and gemm(fn, cout=0) == EINVAL
        assert gemm(fn, cin=257) == ERANGE and gemm(fn, cout=257) == ERANGE and gemm(fn, N_in=2 ** 26 + 1) == ERANGE
    assert gemm("forward", N_out=0, tab=None, out=None) == OK and gemm("dgrad", N_in=0, tab=None, out=None) == OK   # nothing to do

    def wgrad(N_in=100, N_out=90, KV=27, cin=16, cout=32, nbytes=big, **ptr):
        a = dict(x=P(0), dy=P(1), nbr=P(2), scratch=P(3), dw=P(4))
        a.update(ptr)
        return L.dfu3d_spc_wgrad(a['x'], N_in, a['dy'], a['nbr'], N_out, KV, cin, cout, a['scratch'], nbytes, a['dw'], None)
    for name in ("x", "dy", "nbr", "scratch", "dw"):
        assert wgrad(**{name: None}) == EINVAL, name
    assert wgrad(nbytes=L.dfu3d_spc_wgrad_scratch_bytes(90, 27, 16, 32) - 1) == EINVAL and wgrad(scratch=ctypes.c_void_p(8)) == EINVAL
    assert wgrad(KV=0) == EINVAL and wgrad(cin=300) == ERANGE and wgrad(N_out=-2) == EINVAL


def test_scratch_bytes():
    L = _lib_spc.lib()
    for rows in (0, 1, 8, 9, 1000, 2 ** 26):
        entries = max(16, 1 << max(2 * rows - 1, 0).bit_length())
        assert L.dfu3d_spc_table_bytes(rows) == 12 * entries and entries >= 2 * rows
    assert L.dfu3d_spc_table_bytes(-1) == 0 and L.dfu3d_spc_table_bytes(2 ** 26 + 1) == 0
    for bad in ((-1, 8, 27), (8, 0, 27), (8, 8, 0), (8, 8, 28), (2 ** 26 + 1, 8, 1), (2 ** 26, 8, 27 * 2)):
        assert L.dfu3d_spc_scratch_bytes(*bad) == 0, bad
    assert L.dfu3d_spc_scratch_bytes(2 ** 26, 2 ** 26, 27) > 2 ** 32               # no 32-bit wrap-around
    for n, cap, kv in ((100, 800, 27), (0, 1, 27), (5000, 10000, 3), (1024, 2048, 27)):
        cand, entries = n * kv, max(16, 1 << (2 * cap - 1).bit_length())
        blocks = max(1, -(-cand // 1024))
        up = lambda v: -(-v // 16) * 16                                            # noqa: E731
        assert L.dfu3d_spc_scratch_bytes(n, cap, kv) == up(4 * cand) + 4 * entries + up(4 * (blocks + 1))
    assert L.dfu3d_spc_wgrad_scratch_bytes(0, 27, 16, 32) == 0
    assert L.dfu3d_spc_wgrad_scratch_bytes(1, 27, 16, 32) == L.dfu3d_spc_wgrad_scratch_bytes(1024, 27, 16, 32) == 27 * 16 * 32 * 4
    assert L.dfu3d_spc_wgrad_scratch_bytes(1025, 27, 16, 32) == 2 * 27 * 16 * 32 * 4
    assert L.dfu3d_spc_wgrad_scratch_bytes(2 ** 26, 27, 256, 256) > 2 ** 32
    for bad in ((-1, 27, 1, 1), (1, 0, 1, 1), (1, 27, 0, 1), (1, 27, 1, 257)):
        assert L.dfu3d_spc_wgrad_scratch_bytes(*bad) == 0


def test_output_shapes_of_the_kitti_grid():
    from dfu3d_amd import sparse_conv_ops as ops
    shape = (41, 1600, 1408)
    chain = [LAYERS[1], LAYERS[1], LAYERS[2]]                                       # spconv2, spconv3, spconv4
    steps = []
    for k, s, p, _ in chain:
        shape = ops.output_shape(shape, k, s, p)
        steps.append(shape)
    assert steps == [(21, 800, 704), (11, 400, 352), (5, 200, 176)]
    assert ops.output_shape(steps[-1], *LAYERS[3][:3]) == (2, 200, 176) and ops.output_shape(steps[-1], *LAYERS[4][:3]) == (3, 200, 176)
    assert steps == [R.out_shape(a, *chain[i][:3]) for i, a in enumerate([(41, 1600, 1408)] + steps[:2])]
    assert ops.capacity(1000, 4, (21, 800, 704), (3, 3, 3), (2, 2, 2)) == 8000 and ops.capacity(1000, 1, (2, 3, 3), (3, 3, 3), (2, 2, 2)) == 18
    assert ops.capacity(1000, 4, (2, 200, 176), (3, 1, 1), (2, 1, 1)) == 2000
    assert tuple(ops.layer(0, 3, subm=True)) == (0, (3, 3, 3), (1, 1, 1), (1, 1, 1), True)
    assert tuple(ops.layer(2, (3, 1, 1), (2, 1, 1), 0)) == (2, (3, 1, 1), (2, 1, 1), (0, 0, 0), False)


# ---- the modules ----------------------------------------------------------------------------------------------------------
def test_state_dict_keys_of_both_backbones_and_the_plan_they_ask_for():
    from dfu3d_amd.pcdet_kitti import spconv_utils as S
    from dfu3d_amd.pcdet_kitti.spconv_backbone import VoxelBackBone8x, VoxelResBackBone8x
    golden = json.load(open(GOLDEN))
    for cls in (VoxelBackBone8x, VoxelResBackBone8x):
        m = cls({}, golden["input_channels"], [1408, 1600, 40])
        assert [(k, list(v.shape)) for k, v in m.state_dict().items()] == [tuple(e) for e in map(tuple, golden[cls.__name__])]
        assert m.sparse_shape == [41, 1600, 1408] and m.num_point_features == 128
        specs = S.chain_specs(m)
        assert [sp.in_level for sp in specs if not sp.subm] == [0, 1, 2, 3] and specs[-1].kernel == (3, 1, 1)
        assert len({tuple(sp) for sp in specs}) == 8                               # four submanifold and four strided tables
        assert S.find_all_spconv_keys(m) == {k for k, v in m.state_dict().items() if v.dim() == 5}
    assert VoxelResBackBone8x({}, 4, [8, 8, 8]).backbone_channels['x_conv4'] == 128
    assert VoxelBackBone8x({'last_pad': (1, 0, 0)}, 4, [8, 8, 8]).conv_out[0].padding == (1, 0, 0)
    assert VoxelResBackBone8x({'USE_BIAS': False}, 4, [8, 8, 8]).conv1[0].conv1.bias is None
    with pytest.raises(NotImplementedError):
        S.SparseInverseConv3d(4, 4, 3)


def voxel_model_cfg():
    from tests import centerpoint_cases as C
    cfg = dict(C.SMALL_MODEL)
    cfg['VFE'] = {'NAME': 'MeanVFE'}
    cfg['BACKBONE_3D'] = {'NAME': 'VoxelResBackBone8x'}
    cfg['MAP_TO_BEV'] = {'NAME': 'HeightCompression', 'NUM_BEV_FEATURES': 256}
    return cfg, dict(class_names=C.SMALL_DATASET['class_names'], grid_size=[32, 32, 40],
                     point_cloud_range=C.SMALL_DATASET['point_cloud_range'], voxel_size=C.SMALL_DATASET['voxel_size'],
                     num_point_features=4)


def test_centerpoint_takes_the_voxel_modules_only_with_the_keyword():
    import torch
    from dfu3d_amd.pcdet_kitti.centerpoint import CenterPoint
    from dfu3d_amd.pcdet_kitti.spconv_backbone import VoxelResBackBone8x
    cfg, ds = voxel_model_cfg()
    with pytest.raises(NotImplementedError, match="BACKBONE_3D"):
        CenterPoint(cfg, 3, **ds)
    with pytest.raises(NotImplementedError, match="MeanVFE|HeightCompression"):
        CenterPoint({k: v for k, v in cfg.items() if k != 'BACKBONE_3D'}, 3, **ds)
    model = CenterPoint(cfg, 3, sparse_3d=True, **ds)
    names = [type(m).__name__ for m in model.module_list]
    assert names[:3] == ['MeanVFE', 'VoxelResBackBone8x', 'HeightCompression'] and isinstance(model.backbone_3d, VoxelResBackBone8x)
    assert model.backbone_2d is not None and 'backbone_3d.conv_input.0.weight' in model.state_dict()
    # the 1.x layouts: (k, k, k, Cin, Cout), where the transpose or the permutation gives this model's shape
    state = {k: v.clone() for k, v in model.state_dict().items()}
    torch.manual_seed(0)
    w = torch.randn_like(state['backbone_3d.conv2.0.0.weight'])                    # (32, 3, 3, 3, 16)
    old = {k: v for k, v in state.items()}
    old['backbone_3d.conv2.0.0.weight'] = w.permute(1, 2, 3, 4, 0).contiguous()    # (3, 3, 3, 16, 32)
    sq = torch.randn_like(state['backbone_3d.conv_out.0.weight'])                  # (128, 3, 1, 1, 128)
    old['backbone_3d.conv_out.0.weight'] = sq.permute(1, 2, 3, 4, 0).contiguous()  # (3, 1, 1, 128, 128)
    new = model.adapt_spconv_weights(old)
    assert torch.equal(new['backbone_3d.conv2.0.0.weight'], w) and torch.equal(new['backbone_3d.conv_out.0.weight'], sq)
    assert all(new[k] is old[k] for k in old if k not in ('backbone_3d.conv2.0.0.weight', 'backbone_3d.conv_out.0.weight'))
    model.load_state_dict(new, strict=True)
