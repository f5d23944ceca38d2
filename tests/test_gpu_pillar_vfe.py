"""The pillar feature encoder on the GPU (csrc/pillar_stage.hip, dfu3d_amd/pillar_ops.py, pcdet_kitti/dynamic_pillar_vfe.py)
against the numpy restatement tests/pillar_vfe_ref.py, bit for bit, and against golden G13."""
import json
import os
import warnings

import numpy as np
import pytest

from tests import pillar_vfe_ref as R

pytestmark = pytest.mark.gpu

# synthetic geometry: every edge is a float32 number (voxel 0.5), 37 x 53 cells so that a batch sample's cells end inside
# a word of the occupancy bitmap (1961 = 61 * 32 + 9)
GEO = dict(point_cloud_range=[0.0, -2.0, -1.0, 18.5, 24.5, 3.0], voxel_size=[0.5, 0.5, 4.0], grid_size=[37, 53, 1])


@pytest.fixture(scope="module")
def g13(golden_dir):
    g = np.load(os.path.join(golden_dir, "g13_pillar_vfe.npz"))
    return g, json.loads(bytes(g["meta"]).decode())


def hip_group(pts, batch_size, geo=GEO, layout=R.LAYOUT_PILLAR, abs_xyz=True, dist=False, check=True):
    import torch
    from dfu3d_amd import pillar_ops
    return pillar_ops.pillar_group(torch.from_numpy(np.ascontiguousarray(pts, np.float32)).cuda(), batch_size,
                                   geo['point_cloud_range'], geo['voxel_size'], geo['grid_size'], layout=layout,
                                   use_absolute_xyz=abs_xyz, with_distance=dist, check=check)


def check_group(pts, batch_size, geo=GEO, layout=R.LAYOUT_PILLAR, abs_xyz=True, dist=False, status=0):
    """Every output of pillar_group equals the restatement's; returns (group, ref group, ref features)."""
    pts = np.ascontiguousarray(pts, np.float32)
    ref = R.group(pts, batch_size, geo['point_cloud_range'], geo['voxel_size'], geo['grid_size'], layout)
    offs = tuple(geo['voxel_size'][k] / 2 + geo['point_cloud_range'][k] for k in range(3))
    feats = R.features(pts, ref, geo['point_cloud_range'], geo['voxel_size'], offs, layout, abs_xyz, dist)
    g = hip_group(pts, batch_size, geo, layout, abs_xyz, dist, check=False)
    assert (g.n_kept, g.P, g.status) == (len(ref['kept_idx']), len(ref['unq_cnt']), status)
    assert ref['status'] == status
    for k in ('kept_idx', 'unq_inv', 'unq_cnt', 'coords', 'offsets', 'plist'):
        got = getattr(g, k).cpu().numpy()
        assert got.dtype == np.int32 and got.shape == ref[k].shape and np.array_equal(got, ref[k]), k
    got = g.features.cpu().numpy()
    assert got.shape == feats.shape and np.array_equal(got.view(np.uint32), feats.view(np.uint32))
    return g, ref, feats


def random_points(rng, n, batch_size, geo=GEO, cols=5, margin=1.0):
    r = geo['point_cloud_range']
    pts = np.zeros((n, cols), np.float32)
    pts[:, 0] = rng.integers(batch_size, size=n)
    pts[:, 1] = rng.uniform(r[0] - margin, r[3] + margin, n)
    pts[:, 2] = rng.uniform(r[1] - margin, r[4] + margin, n)
    pts[:, 3] = rng.uniform(r[2], r[5], n)
    pts[:, 4:] = rng.uniform(0, 1, (n, cols - 4))
    return pts


@pytest.mark.parametrize("name", sorted(R.CFGS))
def test_group_and_features_g13(g13, name):
    g, _ = g13
    cfg = R.CFGS[name]
    m = cfg['model_cfg']
    grp, ref, feats = check_group(g[name + '_points'], cfg['batch_size'], cfg, cfg['layout'], m['USE_ABSLOTE_XYZ'],
                                  m['WITH_DISTANCE'])
    for k in ('unq_inv', 'unq_cnt', 'coords'):
        assert np.array_equal(getattr(grp, k).cpu().numpy(), g[name + '_' + k]), k
    assert np.array_equal(grp.features.cpu().numpy(), g[name + '_features_in'])


def test_no_points_and_no_kept_points():
    g, _, _ = check_group(np.zeros((0, 5), np.float32), 2)
    assert g.features.shape == (0, 10) and g.coords.shape == (0, 4) and g.offsets.cpu().tolist() == [0]
    rng = np.random.default_rng(1)
    pts = random_points(rng, 300, 2)
    pts[:, 1] += 100.0                                                               # all outside: P = 0
    g, _, _ = check_group(pts, 2, dist=True)
    assert (g.n_kept, g.P) == (0, 0)
    import torch
    from dfu3d_amd import pillar_ops
    x = torch.zeros((0, 32), device='cuda', requires_grad=True)
    out = pillar_ops.pillar_max_concat(x, g)
    assert out.shape == (0, 64) and pillar_ops.pillar_max(x, g).shape == (0, 32)
    out.sum().backward()
    assert x.grad.shape == (0, 32)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
@pytest.mark.parametrize("layout", [R.LAYOUT_PILLAR, R.LAYOUT_SIMPLE2D])
def test_small_sizes(n, layout):
    rng = np.random.default_rng(100 + n)
    check_group(random_points(rng, n, 3, cols=6), 3, layout=layout, abs_xyz=(n % 2 == 1), dist=(n != 64))


def test_range_edges_and_signed_zero():
    r = GEO['point_cloud_range']
    f = np.float32
    up, down = (lambda v: np.nextafter(f(v), f(np.inf))), (lambda v: np.nextafter(f(v), f(-np.inf)))
    xs = [r[0], r[3], up(r[0]), down(r[0]), up(r[3]), down(r[3]), -0.0, 5.0, 5.0, 5.0, 5.0, 5.0, 5.0, 3e38, -3e38, 1e10]
    ys = [0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, r[1], r[4], up(r[1]), down(r[1]), up(r[4]), down(r[4]), 0.0, 0.0, -1e10]
    pts = np.zeros((len(xs), 5), np.float32)
    pts[:, 1], pts[:, 2], pts[:, 3] = xs, ys, 0.5
    pts[:, 0] = np.arange(len(xs)) % 2
    g, ref, _ = check_group(pts, 2, dist=True)
    assert ref['kept_idx'].tolist() == [0, 2, 5, 6, 7, 9, 12]                        # on / inside range_min kept, range_max dropped
    assert np.signbit(pts[6, 1]) and g.coords.cpu().numpy()[:, 3].min() == 0
    check_group(pts, 2, layout=R.LAYOUT_SIMPLE2D)


def test_first_and_last_cell_and_bitmap_word_edges():
    B, (nx, ny) = 3, GEO['grid_size'][:2]
    rng = np.random.default_rng(7)
    pts = random_points(rng, 500, B)
    pts[0, :3] = [B - 1, 18.25, 24.25]                                               # cell (B-1, nx-1, ny-1)
    pts[1, :3] = [0, 0.25, -1.75]                                                    # cell 0
    g, ref, _ = check_group(pts, B)
    c = g.coords.cpu().numpy()
    assert c[0].tolist() == [0, 0, 0, 0] and c[-1].tolist() == [B - 1, 0, ny - 1, nx - 1]
    # every cell of the grid occupied once: keys 0 .. B*nx*ny - 1 cross every word boundary of the bitmap
    cells = np.arange(B * nx * ny)
    full = np.zeros((len(cells), 5), np.float32)
    full[:, 0] = cells // (nx * ny)
    full[:, 1] = (cells % (nx * ny)) // ny * 0.5 + 0.25
    full[:, 2] = (cells % ny) * 0.5 - 1.75
    full = full[rng.permutation(len(cells))]
    g, _, _ = check_group(full, B)
    assert g.P == B * nx * ny


def long_pillar_points(rng, sizes=(1, 64, 65, 1500), extra=700, B=2):
    """Pillars of the given sizes in cells of their own, their points spread among `extra` random ones."""
    pts = [random_points(rng, extra, B)]
    for k, s in enumerate(sizes):
        p = random_points(rng, s, B)
        p[:, 0] = k % B
        p[:, 1] = 2.0 + k + rng.uniform(0.01, 0.49, s)                               # cell x = 4 + 2k, y = 10: nothing else there
        p[:, 2] = 3.0 + rng.uniform(0.01, 0.49, s)
        pts.append(p)
    pts = np.concatenate(pts)
    keep = ~((np.floor(pts[:extra, 2] / 0.5) == 6) & (pts[:extra, 1] >= 2.0) & (pts[:extra, 1] < 9.0))
    pts = np.concatenate([pts[:extra][keep], pts[extra:]])
    return pts[rng.permutation(len(pts))]


def test_pillars_of_1_64_65_1500_points():
    rng = np.random.default_rng(11)
    g, ref, _ = check_group(long_pillar_points(rng), 2, dist=True)
    assert {1, 64, 65, 1500} <= set(ref['unq_cnt'].tolist())


def test_200k_points_more_than_65535_pillars():
    rng = np.random.default_rng(12)
    geo = dict(point_cloud_range=[0.0, -64.0, -3.0, 128.0, 64.0, 1.0], voxel_size=[0.25, 0.25, 4.0], grid_size=[512, 512, 1])
    g, ref, _ = check_group(random_points(rng, 200000, 2, geo), 2, geo)
    assert g.P > 65535


@pytest.mark.parametrize("bad", ["nan_x", "inf_y", "batch_-1", "batch_B"])
def test_bad_point_sets_the_status_bit_and_changes_nothing_else(bad):
    from dfu3d_amd._lib import Dfu3dError
    B = 2
    rng = np.random.default_rng(13)
    clean = random_points(rng, 400, B)
    row = np.array([[0, 5.2, 5.2, 0.5, 0.5]], np.float32)
    if bad == "nan_x":
        row[0, 1] = np.nan
    elif bad == "inf_y":
        row[0, 2] = np.inf
    else:
        row[0, 0] = -1 if bad == "batch_-1" else B
    pts = np.concatenate([clean[:200], row, clean[200:]])
    g, _, _ = check_group(pts, B, status=R.ST_BAD_POINT)
    c, _, _ = check_group(clean, B)
    for k in ('unq_inv', 'unq_cnt', 'coords', 'offsets', 'plist', 'features'):
        assert np.array_equal(getattr(g, k).cpu().numpy(), getattr(c, k).cpu().numpy()), k
    k0, k1 = g.kept_idx.cpu().numpy(), c.kept_idx.cpu().numpy()
    assert np.array_equal(k0 - (k0 > 200), k1)
    with pytest.raises(Dfu3dError, match="non-finite|batch index"):
        hip_group(pts, B)


def test_pillar_group_reads_the_device_once():
    """torch's sync debug mode warns on every synchronising call of torch's own; the library itself never synchronises."""
    import torch
    rng = np.random.default_rng(14)
    pts = torch.from_numpy(random_points(rng, 3000, 2)).cuda()
    from dfu3d_amd import pillar_ops
    args = (pts, 2, GEO['point_cloud_range'], GEO['voxel_size'], GEO['grid_size'])
    pillar_ops.pillar_group(*args)                                                   # library loaded, allocator warm
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("warn")
    try:
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter("always")
            g = pillar_ops.pillar_group(*args)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    sync = [str(x.message) for x in w if "synchroniz" in str(x.message)]
    print(sync)
    assert len(sync) == 1, sync
    assert g.P > 0


# ---- pillar_max / pillar_max_concat -------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def max_group():
    """One grouping with pillars of 1, 64, 65, 129, 200 and 1500 rows (the share-a-pillar path starts above 128)."""
    rng = np.random.default_rng(21)
    pts = long_pillar_points(rng, sizes=(1, 64, 65, 1500, 129, 200), extra=500)
    g, ref, _ = check_group(pts, 2)
    return g, ref


def check_max(x, g, inv, rng, kind):
    """Forward and backward of pillar_max and pillar_max_concat on x against the restatement, bit for bit."""
    import torch
    from dfu3d_amd import pillar_ops
    P, (n, C) = g.P, x.shape
    ref_max, ref_arg = R.pillar_max(x, inv, P)
    xt = torch.from_numpy(x).cuda().requires_grad_(True)
    x_max, arg = pillar_ops.pillar_max(xt, g, return_arg=True)
    assert np.array_equal(x_max.detach().cpu().numpy().view(np.uint32), ref_max.view(np.uint32)), kind
    assert np.array_equal(arg.cpu().numpy(), ref_arg), kind
    gm = rng.normal(size=(P, C)).astype(np.float32)
    x_max.backward(torch.from_numpy(gm).cuda())
    assert np.array_equal(xt.grad.cpu().numpy().view(np.uint32), R.pillar_max_backward(gm, ref_arg, n).view(np.uint32)), kind
    xt.grad = None
    cat = pillar_ops.pillar_max_concat(xt, g)
    assert np.array_equal(cat.detach().cpu().numpy().view(np.uint32), R.pillar_max_concat(x, inv, P)[0].view(np.uint32)), kind
    gc = rng.normal(size=(n, 2 * C)).astype(np.float32)
    cat.backward(torch.from_numpy(gc).cuda())
    want = R.pillar_max_concat_backward(gc, ref_arg, inv)
    assert np.array_equal(xt.grad.cpu().numpy().view(np.uint32), want.view(np.uint32)), kind


@pytest.mark.parametrize("C", [1, 32, 64, 100, 256])
def test_pillar_max_channels_ties_and_long_pillars(max_group, C):
    g, ref = max_group
    rng = np.random.default_rng(30 + C)
    n, inv = g.n_kept, ref['unq_inv']
    check_max(rng.normal(size=(n, C)).astype(np.float32), g, inv, rng, "random")
    x = np.maximum(rng.normal(size=(n, C)), 0).astype(np.float32)                    # after a ReLU: ties at zero
    x[:, ::3] = 0.0                                                                  # all-zero columns: arg is the lowest row
    check_max(x, g, inv, rng, "relu")
    check_max(rng.integers(-2, 3, size=(n, C)).astype(np.float32), g, inv, rng, "equal maxima at distinct rows")
    check_max(np.full((n, C), -np.inf, np.float32), g, inv, rng, "all -inf")


@pytest.mark.parametrize("name", sorted(R.CFGS))
def test_pillar_max_on_g13_x(g13, name):
    g, _ = g13
    cfg = R.CFGS[name]
    grp, ref, _ = check_group(g[name + '_points'], cfg['batch_size'], cfg, cfg['layout'],
                              cfg['model_cfg']['USE_ABSLOTE_XYZ'], cfg['model_cfg']['WITH_DISTANCE'])
    import torch
    from dfu3d_amd import pillar_ops
    rng = np.random.default_rng(40)
    for i in range(len(cfg['model_cfg']['NUM_FILTERS'])):
        x = g['%s_l%d_x' % (name, i)]
        check_max(x, grp, ref['unq_inv'], rng, "g13 layer %d" % i)
        got = pillar_ops.pillar_max(torch.from_numpy(x).cuda(), grp)
        assert np.array_equal(got.cpu().numpy(), g['%s_l%d_x_max' % (name, i)])


def test_pillar_max_refuses_what_it_does_not_compute(max_group):
    import torch
    from dfu3d_amd import pillar_ops
    from dfu3d_amd._lib import Dfu3dError
    g, _ = max_group
    x = torch.zeros((g.n_kept, 32), device='cuda')
    for bad in (x.half(), x.double(), x.t().contiguous().t(), x[:-1], torch.zeros((g.n_kept, 257), device='cuda'), x.cpu()):
        with pytest.raises(Dfu3dError):
            pillar_ops.pillar_max(bad, g)
        with pytest.raises(Dfu3dError):
            pillar_ops.pillar_max_concat(bad, g)


# ---- the modules --------------------------------------------------------------------------------------------------------
def make_module(g, name, device):
    import torch
    from dfu3d_amd.pcdet_kitti import dynamic_pillar_vfe as M
    cfg = R.CFGS[name]
    vfe = getattr(M, cfg['cls'])(model_cfg=cfg['model_cfg'], num_point_features=cfg['num_point_features'],
                                 voxel_size=cfg['voxel_size'], grid_size=cfg['grid_size'],
                                 point_cloud_range=cfg['point_cloud_range'])
    vfe.load_state_dict({k: torch.from_numpy(g['%s_sd_%s' % (name, k)].copy()) for k in vfe.state_dict()}, strict=True)
    return vfe.to(device)


def composition(g, name, layers, device, dtype, train):
    """The encoder in torch alone: unq_inv from the restatement, the feature matrix with torch on the CPU (index_add_ for
    the mean, sequential there; torch.norm), then torch's Linear / BatchNorm1d and scatter_reduce('amax') on `device`.
    `layers`: the module's pfn_layers (their linear / norm are used as they are).  Returns the final features."""
    import torch
    cfg = R.CFGS[name]
    m = cfg['model_cfg']
    pts = g[name + '_points']
    ref = R.group(pts, cfg['batch_size'], cfg['point_cloud_range'], cfg['voxel_size'], cfg['grid_size'], cfg['layout'])
    p = torch.from_numpy(pts[ref['kept_idx']])
    inv = torch.from_numpy(ref['unq_inv'].astype(np.int64))
    xyz = p[:, 1:4].contiguous()
    ox, oy, oz = R.offsets_of(cfg)
    cxy = torch.from_numpy(ref['cxy'])
    f_center = torch.zeros_like(xyz)
    f_center[:, 0] = xyz[:, 0] - (cxy[:, 0] * cfg['voxel_size'][0] + ox)
    f_center[:, 1] = xyz[:, 1] - (cxy[:, 1] * cfg['voxel_size'][1] + oy)
    f_center[:, 2] = xyz[:, 2] - oz
    raw = p[:, 1:] if m['USE_ABSLOTE_XYZ'] else p[:, 4:]
    if cfg['layout'] == R.LAYOUT_PILLAR:
        P = len(ref['unq_cnt'])
        mean = torch.zeros(P, 3).index_add_(0, inv, xyz) / torch.from_numpy(ref['unq_cnt']).float()[:, None]
        cols = [raw, xyz - mean[inv], f_center]
    else:
        cols = [f_center, raw]
    if m['WITH_DISTANCE']:
        cols.append(torch.norm(p[:, 1:4], 2, dim=1, keepdim=True))
    x = torch.cat(cols, 1).to(device=device, dtype=dtype)
    inv = inv.to(device)
    P = len(ref['unq_cnt'])
    for layer in layers:
        x = layer.linear(x)
        x = layer.norm(x) if layer.use_norm else x
        x = torch.relu(x)
        x_max = torch.zeros(P, x.shape[1], device=device, dtype=dtype).scatter_reduce(
            0, inv.view(-1, 1).expand_as(x), x, 'amax', include_self=False)
        x = x_max if layer.last_vfe else torch.cat([x, x_max[inv]], 1)
    return x


def run_module(vfe, g, name):
    import torch
    out = vfe({'points': torch.from_numpy(g[name + '_points'].copy()).cuda(), 'batch_size': R.CFGS[name]['batch_size']})
    return out


@pytest.mark.parametrize("name", sorted(R.CFGS))
@pytest.mark.parametrize("train", [False, True])
def test_module_equals_torch_composition_and_g13(g13, name, train):
    """Bit-equal to the torch-only composition; against G13's final features within four times the deviation that
    composition shows (it differs from G13 only by the GPU's against the CPU's GEMM / BatchNorm rounding; a wiring error is
    of order 1).  Measured on an MI355X (torch 2.10 ROCm 7.0): the composition deviates from G13 by 3.8e-6 (A, eval),
    3.3e-6 (A, train), 0 (B), 9.5e-7 (C, eval), 1.3e-6 (C, train); the HIP path by the same figures."""
    import torch
    g, meta = g13
    vfe = make_module(g, name, 'cuda').train(train)
    twin = make_module(g, name, 'cuda').train(train)
    out = run_module(vfe, g, name)
    feats = out['pillar_features']
    with torch.no_grad():
        comp = composition(g, name, twin.pfn_layers, 'cuda', torch.float32, train)
    assert sorted(k for k in out if k not in ('points', 'batch_size')) == meta[name + '_out_keys']
    coords = out[meta[name + '_coords_key']]
    assert coords.dtype == torch.int32 and np.array_equal(coords.cpu().numpy(), g[name + '_coords'])
    if 'voxel_features' in out:
        assert out['voxel_features'] is out['pillar_features']
    assert torch.equal(feats.detach(), comp)
    for a, b in zip(vfe.state_dict().values(), twin.state_dict().values()):         # BatchNorm's running statistics too
        assert torch.equal(a, b)
    want = g[name + ('_final_train' if train else '_final_eval')]
    dev_comp = float(np.abs(comp.cpu().numpy() - want).max())
    dev_hip = float(np.abs(feats.detach().cpu().numpy() - want).max())
    print("G13 %s train=%s: composition deviates %.3e, HIP path %.3e" % (name, train, dev_comp, dev_hip))
    assert dev_comp < 1e-3                                                           # the composition itself is wired right
    assert dev_hip <= 4 * dev_comp


@pytest.mark.parametrize("name", sorted(R.CFGS))
def test_module_two_runs_bit_equal_and_gradients(g13, name):
    """Two runs give the same bits (outputs and parameter gradients).  Parameter gradients against a float64 CPU run of
    the composition: the margin is four times the deviation of the float32 GPU composition from the same float64 result.
    Measured on an MI355X: the composition deviates by up to 3.0e-4 where the gradient reaches 6.5e2 (A, first linear weight),
    2.3e-5 at 1.0e2 (B), 6.6e-5 at 3.3e2 (C); the HIP path by the same figures."""
    import torch
    g, _ = g13
    rng = np.random.default_rng(50)
    runs = []
    for _ in range(2):
        vfe = make_module(g, name, 'cuda').train()
        feats = run_module(vfe, g, name)['pillar_features']
        if not runs:
            w = rng.normal(size=tuple(feats.shape)).astype(np.float32)
        (feats * torch.from_numpy(w).cuda()).sum().backward()
        runs.append((feats.detach().clone(), [p.grad.clone() for p in vfe.parameters()]))
    assert torch.equal(runs[0][0], runs[1][0])
    for a, b in zip(runs[0][1], runs[1][1]):
        assert torch.equal(a, b)
    grads = {}
    for key, device, dtype in (('f64', 'cpu', torch.float64), ('comp', 'cuda', torch.float32)):
        twin = make_module(g, name, device).to(dtype).train()
        out = composition(g, name, twin.pfn_layers, device, dtype, True)
        (out * torch.from_numpy(w).to(device=device, dtype=dtype)).sum().backward()
        grads[key] = [p.grad.double().cpu().numpy() for p in twin.parameters()]
    for i, (hip, f64, comp) in enumerate(zip(runs[0][1], grads['f64'], grads['comp'])):
        dev_comp = np.abs(comp - f64).max()
        dev_hip = np.abs(hip.double().cpu().numpy() - f64).max()
        scale = np.abs(f64).max()
        print("%s parameter %d: |grad| <= %.3e, composition deviates %.3e, HIP path %.3e" % (name, i, scale, dev_comp, dev_hip))
        assert dev_hip <= 4 * dev_comp, (i, dev_hip, dev_comp)
