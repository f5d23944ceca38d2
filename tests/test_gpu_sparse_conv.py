"""The sparse-convolution stage on the GPU (csrc/sparseconv_stage.hip) against tests/sparse_conv_ref.py, the sequential
restatement of csrc/dfu3d_spc.h: site sets, both tables, the counts and the status word as integers; y, dx and dw as
float32 values bit for bit, the sign of zero set aside (the header says why).  The shapes are the smallest that cross the
kernels' edges: the 64- and 128-row tiles, the 32-channel tile and its staging depth, the weight gradient's chunk."""
import functools
import warnings

import numpy as np
import pytest

from tests import sparse_conv_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
f32 = np.float32
SUBM3 = (0, (3, 3, 3), (1, 1, 1), (1, 1, 1), True)
DOWN3 = (0, (3, 3, 3), (2, 2, 2), (1, 1, 1), False)


def cu(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def random_sites(rng, n, B, shape):
    """n distinct cells, in random order, as [b, z, y, x]."""
    cells = B * shape[0] * shape[1] * shape[2]
    ids = rng.permutation(cells)[:n]
    x, r = ids % shape[2], ids // shape[2]
    y, r = r % shape[1], r // shape[1]
    return np.stack([r // shape[0], r % shape[0], y, x], 1).astype(np.int32)


def gpu_plan(idx, count, B, shape, layers):
    from dfu3d_amd import sparse_conv_ops as ops
    cnt = None if count is None else cu(np.array([count], np.int32))
    return ops.build_plan(cu(idx), cnt, B, shape, [ops.LayerSpec(*sp) for sp in layers])


def same_values(got, exp, what):
    got = got.detach().cpu().numpy()
    assert got.shape == exp.shape and got.dtype == exp.dtype, (what, got.shape, exp.shape)
    bad = np.argwhere(R.canon(got) != R.canon(exp))
    assert len(bad) == 0, (what, len(bad), bad[:4].tolist(), got[tuple(bad[0])], exp[tuple(bad[0])])


def check_plan(plan, levels, tabs, status):
    assert plan.status == status and plan.host_reads == 1 and len(plan.levels) == len(levels)
    for j, (lv, (idx, sh)) in enumerate(zip(plan.levels, levels)):
        assert lv.rows == len(idx) and tuple(lv.spatial_shape) == tuple(sh), (j, lv.rows, len(idx))
        assert int(lv.count.item()) == len(idx)
        assert (lv.indices.cpu().numpy() == idx).all(), ("indices of level", j)
    for i, (t, (nbr, inv, lin, lout)) in enumerate(zip(plan.tables, tabs)):
        assert (t.in_level, t.out_level, t.n_in, t.n_out) == (lin, lout, len(inv), len(nbr)), i
        assert (t.nbr.cpu().numpy() == nbr).all(), ("nbr of layer", i)
        assert (t.inv.cpu().numpy() == inv).all(), ("inv of layer", i)


def check(idx, count, B, shape, layers, chans, seed=0, status=0):
    """Plan and every layer (forward and both gradients through the autograd.Function) against the restatement."""
    import torch
    from dfu3d_amd import sparse_conv_ops as ops
    plan = gpu_plan(idx, count, B, shape, layers)
    levels, tabs, st = R.plan(idx, len(idx) if count is None else count, B, shape, layers)
    assert st == status
    check_plan(plan, levels, tabs, status)
    rng = np.random.default_rng(seed)
    for i, ((cin, cout), sp) in enumerate(zip(chans, layers)):
        nbr, inv, _, _ = tabs[i]
        kv = nbr.shape[1]
        x = rng.standard_normal((len(inv), cin)).astype(f32)
        w = rng.standard_normal((cout,) + tuple(sp[1]) + (cin,)).astype(f32)
        dy = rng.standard_normal((len(nbr), cout)).astype(f32)
        tx, tw = cu(x).requires_grad_(True), cu(w).requires_grad_(True)
        y = ops.sparse_conv(tx, tw, plan.tables[i])
        y.backward(cu(dy))
        torch.cuda.synchronize()
        wf = w.reshape(cout, kv, cin)
        same_values(y, R.forward(x, nbr, wf), ("y", i))
        same_values(tx.grad, R.dgrad(dy, inv, wf), ("dx", i))
        same_values(tw.grad, R.wgrad(x, dy, nbr).reshape(w.shape), ("dw", i))
    return plan, levels, tabs


@pytest.mark.parametrize("rows,cin,cout", [(1, 3, 16), (31, 4, 16), (32, 5, 7), (33, 16, 32), (65, 64, 128),
                                           (65, 128, 128), (129, 33, 65)])
def test_rows_and_channels(rows, cin, cout):
    rng = np.random.default_rng(rows * 1000 + cin)
    idx = random_sites(rng, rows, 2, (4, 5, 6))
    check(idx, None, 2, (4, 5, 6), [SUBM3, DOWN3], [(cin, cout), (cin, cout)], seed=rows)


def test_rows_beyond_two_chunks_of_the_weight_gradient():
    from dfu3d_amd import sparse_conv_ops as ops
    rows = 2 * ops.WGRAD_CHUNK + 53
    assert ops.WGRAD_CHUNK == R.WGRAD_CHUNK
    rng = np.random.default_rng(7)
    idx = random_sites(rng, rows, 2, (6, 20, 24))
    check(idx, None, 2, (6, 20, 24), [SUBM3, DOWN3], [(5, 7), (3, 4)], seed=7)


def test_a_tile_with_no_neighbour_at_most_offsets_and_a_dense_block():
    # a lattice of pitch 4: the centre offset alone for the submanifold layer, one offset per row for the strided one
    g = np.stack(np.meshgrid(np.arange(0, 8, 4), np.arange(0, 16, 4), np.arange(0, 20, 4), indexing="ij"), -1).reshape(-1, 3)
    lattice = np.concatenate([np.zeros((len(g), 1), int), g], 1).astype(np.int32)
    _, _, tabs = check(lattice, None, 1, (8, 16, 20), [SUBM3, DOWN3], [(16, 32), (16, 32)], seed=1)
    assert ((tabs[0][0] >= 0).sum(1) == 1).all() and (tabs[0][0][:, 13] == np.arange(len(lattice))).all()
    d = np.stack(np.meshgrid(np.arange(4), np.arange(4), np.arange(4), indexing="ij"), -1).reshape(-1, 3)
    dense = np.concatenate([np.zeros((64, 1), int), d], 1).astype(np.int32)
    _, _, tabs = check(dense, None, 1, (4, 4, 4), [SUBM3, DOWN3], [(8, 8), (8, 8)], seed=2)
    assert (tabs[0][0] >= 0).sum() == 10 ** 3 and len(tabs[1][0]) == 8


def test_all_backbone_layers_an_empty_scene_and_shared_tables():
    rng = np.random.default_rng(3)
    shape = (17, 10, 12)
    idx = random_sites(rng, 150, 3, shape)
    idx = idx[idx[:, 0] != 1]                                                # scene 1 is empty
    corners = np.array([[b, z, y, x] for b in (0, 2) for z in (0, 16) for y in (0, 9) for x in (0, 11)], np.int32)
    idx = np.unique(np.concatenate([corners, idx]), axis=0)
    idx = idx[rng.permutation(len(idx))]
    layers = [SUBM3, SUBM3, DOWN3, (1, (3, 3, 3), (1, 1, 1), (1, 1, 1), True), (1, (3, 3, 3), (2, 2, 2), (0, 1, 1), False),
              (2, (3, 1, 1), (2, 1, 1), (0, 0, 0), False), (2, (3, 1, 1), (2, 1, 1), (0, 0, 0), False), DOWN3,
              (2, (3, 1, 1), (2, 1, 1), (1, 0, 0), False)]
    plan, levels, _ = check(idx, None, 3, shape, layers, [(4, 6)] * len(layers), seed=3)
    assert plan.tables[0] is plan.tables[1] and plan.tables[5] is plan.tables[6] and plan.tables[2] is plan.tables[7]
    assert [lv[1] for lv in levels] == [shape, (9, 5, 6), (4, 3, 3), (1, 3, 3), (2, 3, 3)]
    assert not (levels[1][0][:, 0] == 1).any()


def test_a_padded_tail_bad_rows_and_duplicates():
    rng = np.random.default_rng(4)
    shape = (5, 6, 7)
    idx = random_sites(rng, 90, 2, shape)
    padded = np.concatenate([idx, np.full((37, 4), -1, np.int32)])
    check(padded, 90, 2, shape, [SUBM3, DOWN3], [(4, 16), (4, 16)], seed=4)           # the count below N: status 0
    check(padded, 50, 2, shape, [SUBM3, DOWN3], [(4, 16), (4, 16)], seed=5)
    bad = idx.copy()
    bad[7] = (2, 0, 0, 0)                                                          # batch index beyond B
    bad[20] = (0, 5, 0, 0)                                                         # z beyond the shape
    bad[21] = (1, 0, -1, 0)
    plan, _, tabs = check(bad, None, 2, shape, [SUBM3, DOWN3], [(4, 16), (4, 16)], seed=6, status=R.BAD_COORD)
    assert (tabs[0][0][[7, 20, 21]] == -1).all() and not np.isin(tabs[0][0], [7, 20, 21]).any()
    dup = idx.copy()
    dup[60] = dup[11]
    dup[61] = dup[11]
    dup[3] = (0, 9, 9, 9)
    _, _, tabs = check(dup, None, 2, shape, [SUBM3, DOWN3], [(4, 16), (4, 16)], seed=7, status=R.BAD_COORD | R.DUP_SITE)
    assert tabs[0][0][11, 13] == 11 and (tabs[0][0][[60, 61]] == -1).all() and not np.isin(tabs[1][0], [60, 61]).any()
    check(padded, 0, 2, shape, [SUBM3, DOWN3], [(4, 16), (4, 16)], seed=8)            # no row at all


def test_a_grid_beyond_31_bits_of_cells():
    shape = (41, 2048, 2048)
    B = 16                                                                         # the far corner's key needs 32 bits
    far = np.array([[15, 40, 2047, 2047], [15, 40, 2047, 2046], [15, 39, 2047, 2047], [0, 0, 0, 0], [15, 40, 2046, 2047],
                    [14, 40, 2047, 2047], [15, 0, 2047, 0]], np.int32)
    _, levels, tabs = check(far, None, B, shape, [SUBM3, DOWN3], [(4, 8), (4, 8)], seed=9)
    assert (tabs[0][0][0] >= 0).sum() == 4 and levels[1][0][0].tolist() == [15, 20, 1023, 1023]
    assert ((15 * 41 + 40) * 2048 + 2047) * 2048 + 2047 > 2 ** 31


@functools.lru_cache(maxsize=None)
def medium():
    rng = np.random.default_rng(10)
    shape = (6, 12, 14)
    idx = random_sites(rng, 300, 2, shape)
    x = rng.standard_normal((300, 16)).astype(f32)
    w = rng.standard_normal((32, 3, 3, 3, 16)).astype(f32)
    levels, tabs, _ = R.plan(idx, 300, 2, shape, [SUBM3, DOWN3])
    dy = [rng.standard_normal((len(t[0]), 32)).astype(f32) for t in tabs]
    wf = w.reshape(32, 27, 16)
    exp = [(R.forward(x, t[0], wf), R.dgrad(g, t[1], wf), R.wgrad(x, g, t[0]).reshape(w.shape)) for t, g in zip(tabs, dy)]
    return idx, shape, x, w, dy, exp


def run_medium():
    """-> plan tables and y, dx, dw of both layers, as tensors."""
    from dfu3d_amd import sparse_conv_ops as ops
    idx, shape, x, w, dy, _ = medium()
    plan = gpu_plan(idx, None, 2, shape, [SUBM3, DOWN3])
    out = []
    for t, g in zip(plan.tables, dy):
        tx, tw = cu(x).requires_grad_(True), cu(w).requires_grad_(True)
        y = ops.sparse_conv(tx, tw, t)
        y.backward(cu(g))
        out += [t.nbr, t.inv, y.detach(), tx.grad, tw.grad]
    return tuple(out)


def verify_medium(out, which=(0, 1)):
    exp = medium()[5]
    for i in which:
        for k, name in enumerate(("y", "dx", "dw")):
            got = out[5 * i + 2 + k]
            assert (R.canon(got) == R.canon(exp[i][k])).all(), (i, name)


def test_guard_bands_poisoned_scratch_and_the_same_bits_twice():
    from tests.test_gpu_guard_bands import both_poisons
    first = both_poisons(run_medium, verify_medium, min_count=20)
    again = both_poisons(run_medium, verify_medium, min_count=20)
    for a, b in zip(first, again):
        assert a.dtype == b.dtype and a.tobytes() == b.tobytes()


def test_launch_counts_and_host_reads(monkeypatch):
    import ctypes
    import torch
    from dfu3d_amd import _lib, _lib_spc, sparse_conv_ops as ops
    idx, shape, x, w, dy, _ = medium()
    layers = [ops.LayerSpec(*SUBM3), ops.LayerSpec(*DOWN3)]
    didx, dx_, dw_, dg = cu(idx), cu(x), cu(w), [cu(g) for g in dy]
    ops.build_plan(didx, None, 2, shape, layers)                                   # library loaded, allocator warm
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("warn")
    try:
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            plan = ops.build_plan(didx, None, 2, shape, layers)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert len([c for c in caught if "synchroniz" in str(c.message)]) == 1 == plan.host_reads
    torch.cuda.set_sync_debug_mode("error")                                        # the convolution itself: no read at all
    try:
        for t, g in zip(plan.tables, dg):
            tx, tw = dx_.clone().requires_grad_(True), dw_.clone().requires_grad_(True)
            ops.sparse_conv(tx, tw, t).backward(g)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    L = _lib.load_variant("count")
    L.dfu3d_debug_launch_count.restype = ctypes.c_longlong
    L.dfu3d_debug_launch_count.argtypes = [ctypes.c_int]
    monkeypatch.setattr(_lib, "_LIB", L)
    monkeypatch.setattr(_lib_spc, "_BOUND", _lib_spc.bind(L))
    L.dfu3d_debug_launch_count(1)
    plan = ops.build_plan(didx, None, 2, shape, layers)
    assert int(L.dfu3d_debug_launch_count(1)) == ops.LAUNCHES_INDEX + ops.LAUNCHES_DOWNSAMPLE + 2 * ops.LAUNCHES_TABLES
    for t, g in zip(plan.tables, dg):
        y = ops.conv_forward(dx_, dw_, t)
        assert int(L.dfu3d_debug_launch_count(1)) == ops.LAUNCHES_FORWARD
        gx = ops.conv_dgrad(g, dw_, t)
        assert int(L.dfu3d_debug_launch_count(1)) == ops.LAUNCHES_DGRAD
        gw = ops.conv_wgrad(dx_, g, t, dw_.shape)
        assert int(L.dfu3d_debug_launch_count(1)) == ops.LAUNCHES_WGRAD
    torch.cuda.synchronize()
    verify_medium([None] * 7 + [y.cpu().numpy(), gx.cpu().numpy(), gw.cpu().numpy()], which=(1,))
