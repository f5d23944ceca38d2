"""GPU: the pillar scatter (bevscatter_stage.hip, include/dfu3d_bev.h) and its Python surface against the NumPy
restatement (tests/pillar_scatter_ref.py) and golden G16(a), bit for bit, forward and backward."""
import ctypes
import json
import warnings

import numpy as np
import pytest

from tests import centerpoint_cases as K
from tests import pillar_scatter_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# (id, B, C, nz, ny, nx, P, what it is there to catch)
CASES = [
    ("smallest", 1, 1, 1, 1, 1, 1, {}),
    ("ragged_tiles_empty_sample", 3, 64, 1, 37, 70, 2072, dict(empty=(1,), corners=(0, 2))),     # 40 % of 2 x 2590 cells
    ("full_tiny_c", 2, 5, 1, 64, 64, 8192, {}),
    ("c_above_64", 2, 96, 1, 33, 129, 500, {}),
    ("channel_limit", 1, 256, 1, 8, 8, 40, {}),
    ("scatter3d", 2, 8, 4, 19, 23, 900, {}),
    ("no_pillars", 2, 7, 1, 5, 9, 0, {}),
]


def _inputs(case):
    _, B, C, nz, ny, nx, P, kw = case
    if P == 0:
        return np.zeros((0, C), np.float32), np.zeros((0, 4), np.int32)
    return K.scatter_inputs(B, C, (nx, ny, nz), P, 1700 + C + nx, **kw)


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _run(f, coords, B, grid, **kw):
    from dfu3d_amd import bev_ops
    info = bev_ops.ScatterInfo()
    canvas = bev_ops.pillar_scatter(_dev(f), _dev(coords), B, grid, info=info, **kw)
    return canvas, info


@pytest.fixture(scope="module")
def restated():
    """Every case's restated canvas, cell map and gradient, computed once and left unchanged."""
    out = {}
    for case in CASES:
        name, B, C, nz, ny, nx, P, _ = case
        f, coords = _inputs(case)
        canvas, cell_map, status = R.scatter(f, coords, B, (nx, ny, nz))
        gc = np.random.default_rng(len(name)).standard_normal(canvas.shape).astype(np.float32)
        flat = gc.reshape(-1)
        flat[0] = np.float32(np.nan)
        if flat.size > 1:
            flat[1] = np.float32(-0.0)
        out[name] = (f, coords, canvas, cell_map, status, gc, R.scatter_backward(gc, coords, B, (nx, ny, nz), cell_map, P))
    return out


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_stage_equals_the_restatement_forward_and_backward(restated, case):
    import torch
    from dfu3d_amd import _lib_bev
    name, B, C, nz, ny, nx, P, _ = case
    f, coords, want, want_map, want_status, gc, want_grad = restated[name]
    assert want_status == 0
    ft = _dev(f).requires_grad_(True)
    from dfu3d_amd import bev_ops
    info = bev_ops.ScatterInfo()
    canvas = bev_ops.pillar_scatter(ft, _dev(coords), B, (nx, ny, nz), info=info)
    assert canvas.shape == (B, C * nz, ny, nx) and canvas.is_contiguous()
    assert R.same_bits(canvas.detach().cpu().numpy(), want)
    assert np.array_equal(info.cell_map.cpu().numpy(), want_map) and int(info.status.item()) == 0
    # autograd through the op
    canvas.backward(_dev(gc))
    assert R.same_bits(ft.grad.cpu().numpy(), want_grad)
    # and the entry point alone, into rows pre-filled with NaN: every row is written
    gf = torch.full((max(P, 1), C), float('nan'), device=DEV)
    g = _dev(gc)
    ct = _dev(coords)
    rc = _lib_bev.lib().dfu3d_pillar_scatter_backward(
        ctypes.c_void_p(g.data_ptr()), ctypes.c_void_p(ct.data_ptr()) if P else None, 4, P, None, C, B, nz, ny, nx,
        ctypes.c_void_p(info.cell_map.data_ptr()), ctypes.c_void_p(gf.data_ptr()), None)
    torch.cuda.synchronize()
    assert rc == 0 and R.same_bits(gf.cpu().numpy()[:P], want_grad)
    # a second run: the same bits
    again, info2 = _run(f, coords, B, (nx, ny, nz))
    assert torch.equal(again.view(torch.int32), canvas.detach().view(torch.int32)) and torch.equal(info2.cell_map, info.cell_map)


def test_three_column_coords_and_unaligned_out(restated):
    """[b, y, x] coordinates; an `out` whose address is not a multiple of 16 bytes takes the scalar stores."""
    import torch
    f, coords, want, _, _, _, _ = restated["c_above_64"]
    _, B, C, nz, ny, nx, P, _ = CASES[3]
    c3 = np.ascontiguousarray(coords[:, [0, 2, 3]])
    buf = torch.full((want.size + 1,), float('nan'), device=DEV)
    got, _ = _run(f, c3, B, (nx, ny, nz), out=buf[1:])
    assert got.data_ptr() == buf.data_ptr() + 4 and R.same_bits(got.cpu().numpy(), want) and bool(torch.isnan(buf[0]))
    f, coords, want, _, _, _, _ = restated["full_tiny_c"]
    buf = torch.full((want.size + 1,), float('nan'), device=DEV)
    got, _ = _run(f, coords, 2, (64, 64, 1), out=buf[1:])
    assert R.same_bits(got.cpu().numpy(), want)


def test_g16_through_the_modules():
    import torch
    from dfu3d_amd.pcdet_kitti import pointpillar_scatter as M
    g = K.golden()
    meta = json.loads(bytes(g["meta"]).decode())
    for name, cls, B, C, grid, P, seed in K.SCATTER_CASES:
        mod = getattr(M, cls)(K.cfg({'NUM_BEV_FEATURES': C * grid[2], 'INPUT_SHAPE': list(grid)}), grid_size=list(grid))
        ft = _dev(g[name + '_features']).requires_grad_(True)
        d = mod({'pillar_features': ft, 'voxel_coords': _dev(g[name + '_coords']), 'batch_size': B})
        want = R.dense(g[name + '_canvas_idx'], g[name + '_canvas_val'], g[name + '_canvas_shape'])
        assert R.same_bits(d['spatial_features'].detach().cpu().numpy(), want)
        mod.check_status()
        if name == 's2':
            assert d['spatial_features'].shape == (2, 32, 19, 23)
        if name == K.GRAD_CASE:
            gc = np.random.default_rng(meta['grad_seed']).standard_normal(want.shape).astype(np.float32)
            d['spatial_features'].backward(_dev(gc))
            assert R.same_bits(ft.grad.cpu().numpy(), g[name + '_grad_features'])
        # int64 coordinates, as a reference pipeline may hand them over
        d2 = mod({'pillar_features': ft.detach(), 'voxel_coords': _dev(g[name + '_coords']).long(), 'batch_size': B})
        assert torch.equal(d2['spatial_features'].view(torch.int32), d['spatial_features'].detach().view(torch.int32))


def test_out_prefilled_with_nan_is_fully_written(restated):
    import torch
    for name in ("ragged_tiles_empty_sample", "no_pillars", "scatter3d"):
        f, coords, want, _, _, _, _ = restated[name]
        case = next(c for c in CASES if c[0] == name)
        _, B, C, nz, ny, nx, P, _ = case
        out = torch.full(want.shape, float('nan'), device=DEV)
        got, _ = _run(f, coords, B, (nx, ny, nz), out=out)
        assert got.data_ptr() == out.data_ptr()
        assert R.same_bits(out.cpu().numpy(), want)
        assert int(torch.isnan(out).sum()) == int(np.isnan(want).sum())


def test_row_order_does_not_matter(restated):
    f, coords, want, _, _, _, _ = restated["ragged_tiles_empty_sample"]
    perm = np.random.default_rng(3).permutation(len(f))
    for order in (np.arange(len(f))[::-1], perm):
        got, _ = _run(f[order], coords[order], 3, (70, 37, 1))
        assert R.same_bits(got.cpu().numpy(), want)


def test_capacity_form_never_reads_beyond_the_device_count(restated):
    import torch
    f, coords, _, _, _, gc, _ = restated["c_above_64"]
    _, B, C, nz, ny, nx, P, _ = CASES[3]
    n = 321
    want, want_map, _ = R.scatter(f[:n], coords[:n], B, (nx, ny, nz))
    fp, cp = f.copy(), coords.copy()
    fp[n:] = np.nan
    cp[n:] = np.random.default_rng(4).integers(-2 ** 31, 2 ** 31 - 1, size=cp[n:].shape, dtype=np.int64).astype(np.int32)
    cp[n] = coords[0]                                                 # a duplicate of row 0, were it read
    n_dev = torch.tensor([n], dtype=torch.int32, device=DEV)
    ft = _dev(fp).requires_grad_(True)
    from dfu3d_amd import bev_ops
    info = bev_ops.ScatterInfo()
    got = bev_ops.pillar_scatter(ft, _dev(cp), B, (nx, ny, nz), n_pillars=n_dev, info=info)
    assert R.same_bits(got.detach().cpu().numpy(), want) and int(info.status.item()) == 0
    assert np.array_equal(info.cell_map.cpu().numpy(), want_map)
    got.backward(_dev(gc))
    wg = R.scatter_backward(gc, cp, B, (nx, ny, nz), want_map, P, n_pillars=n)
    assert R.same_bits(ft.grad.cpu().numpy(), wg) and not R.bits(wg[n:]).any()


def test_three_rows_on_one_cell():
    import torch
    from dfu3d_amd import bev_ops
    from dfu3d_amd._lib import Dfu3dError
    B, C, grid = 2, 70, (66, 5, 1)
    f, coords = K.scatter_inputs(B, C, grid, 200, 5)
    free = ~((coords[:, 0] == 1) & (coords[:, 2] == 2) & np.isin(coords[:, 3], [63, 64, 65]))
    f, coords = f[free], coords[free]                      # nobody sits on the three cells used below
    P = len(f)
    assert P >= 197
    rows = [17, 150, 60]                                   # 150 is the highest: it wins wherever it stands in the list
    left, right = [1, 0, 2, 63], [1, 0, 2, 65]              # the neighbours along x, across a run boundary
    keep = [5, 190]
    coords[rows] = [1, 0, 2, 64]
    coords[keep[0]], coords[keep[1]] = left, right
    want, want_map, status = R.scatter(f, coords, B, grid)
    assert status == R.ST_DUPLICATE and want_map[(1 * 5 + 2) * 66 + 64] == 150
    ft = _dev(f).requires_grad_(True)
    info = bev_ops.ScatterInfo()
    got = bev_ops.pillar_scatter(ft, _dev(coords), B, grid, info=info)
    host = got.detach().cpu().numpy()
    assert int(info.status.item()) == bev_ops.ST_DUPLICATE and R.same_bits(host, want)
    assert R.same_bits(host[1, :, 2, 64], f[150]) and R.same_bits(host[1, :, 2, 63], f[keep[0]])
    assert R.same_bits(host[1, :, 2, 65], f[keep[1]])
    gc = np.random.default_rng(6).standard_normal(want.shape).astype(np.float32)
    got.backward(_dev(gc))
    grad = ft.grad.cpu().numpy()
    assert R.same_bits(grad, R.scatter_backward(gc, coords, B, grid, want_map, P))
    assert not R.bits(grad[[17, 60]]).any() and R.same_bits(grad[150], gc[1, :, 2, 64])
    with pytest.raises(Dfu3dError, match="one cell"):
        bev_ops.pillar_scatter(_dev(f), _dev(coords), B, grid, check=True)
    del torch


def test_bad_coordinates_are_dropped():
    from dfu3d_amd import bev_ops
    from dfu3d_amd._lib import Dfu3dError
    B, C, grid = 2, 6, (11, 7, 1)
    nx, ny, nz = grid
    f, coords = K.scatter_inputs(B, C, grid, 60, 7)
    clean_rows = np.setdiff1d(np.arange(60), [3, 9, 21, 40, 59])
    base, base_map, _ = R.scatter(f[clean_rows], coords[clean_rows], B, grid)
    for row, bad in zip((3, 9, 21, 40, 59), ([-1, 0, 2, 2], [B, 0, 2, 2], [0, 0, ny, 2], [1, 0, 3, -1], [0, 1, 2, 2])):
        coords[row] = bad
    want, want_map, status = R.scatter(f, coords, B, grid)
    assert status == R.ST_BAD_COORD and R.same_bits(want, base)              # every other cell as without the rows
    ft = _dev(f).requires_grad_(True)
    info = bev_ops.ScatterInfo()
    got = bev_ops.pillar_scatter(ft, _dev(coords), B, grid, info=info)
    assert int(info.status.item()) == bev_ops.ST_BAD_COORD and R.same_bits(got.detach().cpu().numpy(), want)
    assert np.array_equal(info.cell_map.cpu().numpy(), want_map)
    gc = np.random.default_rng(8).standard_normal(want.shape).astype(np.float32)
    got.backward(_dev(gc))
    grad = ft.grad.cpu().numpy()
    assert R.same_bits(grad, R.scatter_backward(gc, coords, B, grid, want_map, 60))
    assert not R.bits(grad[[3, 9, 21, 40, 59]]).any() and np.abs(grad[clean_rows]).min() > 0
    with pytest.raises(Dfu3dError, match="outside the canvas"):
        bev_ops.pillar_scatter(_dev(f), _dev(coords), B, grid, check=True)
    del base_map


def test_launch_count_does_not_depend_on_the_batch(monkeypatch):
    import torch
    from dfu3d_amd import _lib, _lib_bev
    L = _lib.load_variant("count")
    L.dfu3d_debug_launch_count.restype = ctypes.c_longlong
    L.dfu3d_debug_launch_count.argtypes = [ctypes.c_int]
    monkeypatch.setattr(_lib, "_LIB", L)
    monkeypatch.setattr(_lib_bev, "_BOUND", _lib_bev.bind(L))
    fwd, bwd = [], []
    for B, P in ((1, 1), (4, 5000)):
        grid = (96, 80, 1)
        f, coords = K.scatter_inputs(B, 16, grid, P, 9)
        ft = _dev(f).requires_grad_(True)
        from dfu3d_amd import bev_ops
        L.dfu3d_debug_launch_count(1)
        canvas = bev_ops.pillar_scatter(ft, _dev(coords), B, grid)
        fwd.append(int(L.dfu3d_debug_launch_count(1)))
        canvas.backward(torch.ones_like(canvas))
        bwd.append(int(L.dfu3d_debug_launch_count(1)))
        want, _, _ = R.scatter(f, coords, B, grid)
        assert R.same_bits(canvas.detach().cpu().numpy(), want)
    torch.cuda.synchronize()
    assert fwd[0] == fwd[1] and 0 < fwd[0] <= 3 and bwd == [1, 1], (fwd, bwd)


def test_module_forward_makes_no_host_synchronisation(restated):
    """torch's sync debug mode counts torch's own synchronising calls; the library never synchronises."""
    import torch
    from dfu3d_amd.pcdet_kitti.pointpillar_scatter import PointPillarScatter
    from dfu3d_amd._lib import Dfu3dError
    f, coords, want, _, _, _, _ = restated["ragged_tiles_empty_sample"]
    mod = PointPillarScatter({'NUM_BEV_FEATURES': 64}, grid_size=[70, 37, 1])
    ft, ct = _dev(f), _dev(coords)
    mod({'pillar_features': ft, 'voxel_coords': ct, 'batch_size': 3})                       # warm
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        d = mod({'pillar_features': ft, 'voxel_coords': ct, 'batch_size': 3})
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert R.same_bits(d['spatial_features'].cpu().numpy(), want)
    torch.cuda.set_sync_debug_mode("warn")
    try:
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter("always")
            mod({'pillar_features': ft, 'voxel_coords': ct, 'batch_size': 3}, check=True)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert len([x for x in w if "synchroniz" in str(x.message)]) == 1, [str(x.message) for x in w]
    # batch_size comes from the batch_dict: a trailing empty sample keeps its canvas
    d = mod({'pillar_features': ft, 'voxel_coords': ct, 'batch_size': 4})
    assert d['spatial_features'].shape == (4, 64, 37, 70) and not d['spatial_features'][3].any()
    with pytest.raises(Dfu3dError):
        mod({'pillar_features': ft.double(), 'voxel_coords': ct, 'batch_size': 3})
