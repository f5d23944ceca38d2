"""Float32 restatement of the dynamic pillar feature encoder in numpy: the expectation of every exact check of
csrc/pillar_stage.hip.  Sums are sequential in ascending point index (np.add.at), the argument of a maximum is the
lowest row among equals, and the backward of the two scatter functions is written out.  Golden G13
(tests/golden/g13_pillar_vfe.npz) pins this restatement to the reference's own orchestration."""
import numpy as np

LAYOUT_PILLAR, LAYOUT_SIMPLE2D = 0, 1
ST_BAD_POINT = 1

CFG_A = dict(name='A', cls='DynamicPillarVFE', layout=LAYOUT_PILLAR, point_cloud_range=[0, -51.2, -5, 51.2, 51.2, 3],
             voxel_size=[0.2, 0.2, 8], grid_size=[256, 512, 1], num_point_features=4, batch_size=3,
             model_cfg=dict(USE_NORM=True, WITH_DISTANCE=False, USE_ABSLOTE_XYZ=True, NUM_FILTERS=[64, 64]))
CFG_B = dict(name='B', cls='DynamicPillarVFE', layout=LAYOUT_PILLAR, point_cloud_range=[-3.7, -5.3, -2, 3.7, 5.3, 2],
             voxel_size=[0.2, 0.2, 4], grid_size=[37, 53, 1], num_point_features=5, batch_size=2,
             model_cfg=dict(USE_NORM=False, WITH_DISTANCE=True, USE_ABSLOTE_XYZ=False, NUM_FILTERS=[32]))
CFG_C = dict(name='C', cls='DynamicPillarVFESimple2D', layout=LAYOUT_SIMPLE2D, point_cloud_range=[0, -8, -3, 16, 8, 1],
             voxel_size=[0.25, 0.25, 4], grid_size=[64, 64, 1], num_point_features=4, batch_size=2,
             model_cfg=dict(USE_NORM=True, WITH_DISTANCE=False, USE_ABSLOTE_XYZ=True, NUM_FILTERS=[32, 32]))
CFGS = {'A': CFG_A, 'B': CFG_B, 'C': CFG_C}


def offsets_of(cfg):
    """The reference's centre offsets: Python floats."""
    return tuple(cfg['voxel_size'][k] / 2 + cfg['point_cloud_range'][k] for k in range(3))


def _fma(a, b, c):
    """float32 fma(a, b, c) through float64: the product of two float32 is exact there, and the one further rounding of
    the sum differs from the fused one only on a tie of probability 2^-29 per operation."""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def group(points, batch_size, point_cloud_range, voxel_size, grid_size, layout=LAYOUT_PILLAR):
    """points (N, 1 + F) float32 -> dict(kept_idx, unq_inv, unq_cnt, coords, offsets, plist, status, cxy)."""
    points = np.ascontiguousarray(points, np.float32)
    rmin = np.asarray(point_cloud_range[:2], np.float32)
    vox = np.asarray(voxel_size[:2], np.float32)
    nx, ny = int(grid_size[0]), int(grid_size[1])
    bf, xy = points[:, 0], points[:, 1:3]
    with np.errstate(invalid='ignore', over='ignore'):
        finite = np.isfinite(xy).all(1)
        batch_ok = (bf > np.float32(-1)) & (bf < np.float32(batch_size))
        f = np.floor((xy - rmin) / vox)
        inside = (f[:, 0] >= 0) & (f[:, 0] < np.float32(nx)) & (f[:, 1] >= 0) & (f[:, 1] < np.float32(ny))
    bad = ~finite | ~batch_ok
    keep = inside & ~bad
    kept_idx = np.flatnonzero(keep).astype(np.int32)
    c = f[keep].astype(np.int32)
    key = bf[keep].astype(np.int32) * np.int32(nx * ny) + c[:, 0] * np.int32(ny) + c[:, 1]
    unq, inv, cnt = np.unique(key, return_inverse=True, return_counts=True)
    inv = inv.reshape(-1)
    b, cell = unq // (nx * ny), unq % (nx * ny)
    zero = np.zeros_like(b)
    if layout == LAYOUT_PILLAR:
        coords = np.stack([b, zero, cell % ny, cell // ny], 1)
    else:
        coords = np.stack([b, cell % ny, cell // ny], 1)
    return dict(kept_idx=kept_idx, unq_inv=inv.astype(np.int32), unq_cnt=cnt.astype(np.int32),
                coords=coords.astype(np.int32),
                offsets=np.concatenate([[0], np.cumsum(cnt)]).astype(np.int32),
                plist=np.argsort(inv, kind='stable').astype(np.int32), status=int(ST_BAD_POINT if bad.any() else 0),
                cxy=c.astype(np.float32))


def features(points, g, point_cloud_range, voxel_size, offsets, layout=LAYOUT_PILLAR, use_absolute_xyz=True,
             with_distance=False):
    """The matrix entering the first PFN layer, float32 (n_kept, width)."""
    p = np.ascontiguousarray(points, np.float32)[g['kept_idx']]
    xyz = p[:, 1:4]
    vx, vy = np.float32(voxel_size[0]), np.float32(voxel_size[1])
    ox, oy, oz = (np.float32(o) for o in offsets)
    f_center = np.stack([xyz[:, 0] - (g['cxy'][:, 0] * vx + ox), xyz[:, 1] - (g['cxy'][:, 1] * vy + oy), xyz[:, 2] - oz], 1)
    raw = p[:, 1:] if use_absolute_xyz else p[:, 4:]
    if layout == LAYOUT_PILLAR:
        s = np.zeros((len(g['unq_cnt']), 3), np.float32)
        np.add.at(s, g['unq_inv'], xyz)                              # sequential, ascending point index
        mean = s / g['unq_cnt'].astype(np.float32)[:, None]
        cols = [raw, xyz - mean[g['unq_inv']], f_center]
    else:
        cols = [f_center, raw]
    if with_distance:
        cols.append(np.sqrt(_fma(xyz[:, 2], xyz[:, 2], _fma(xyz[:, 1], xyz[:, 1], xyz[:, 0] * xyz[:, 0])))[:, None])
    return np.ascontiguousarray(np.concatenate(cols, 1), np.float32)


def pillar_max(x, unq_inv, P):
    """x (n, C) -> x_max (P, C), arg (P, C) int32: the lowest row among equal maxima."""
    x = np.asarray(x, np.float32)
    n, C = x.shape
    if n == 0:
        return np.zeros((0, C), np.float32), np.zeros((0, C), np.int32)
    order = np.argsort(unq_inv, kind='stable')
    starts = np.concatenate([[0], np.cumsum(np.bincount(unq_inv, minlength=P))[:-1]])
    xs = x[order]
    x_max = np.maximum.reduceat(xs, starts, axis=0)
    rows = np.where(xs == x_max[unq_inv[order]], order[:, None], np.iinfo(np.int32).max)
    arg = np.minimum.reduceat(rows, starts, axis=0).astype(np.int32)
    return x_max, arg


def pillar_max_concat(x, unq_inv, P):
    x_max, arg = pillar_max(x, unq_inv, P)
    return np.concatenate([np.asarray(x, np.float32), x_max[unq_inv]], 1), arg


def pillar_max_backward(grad_max, arg, n):
    """grad_x (n, C): grad_max routed to arg, zero elsewhere."""
    P, C = arg.shape
    gx = np.zeros((n, C), np.float32)
    if P:
        gx[arg, np.arange(C)[None, :]] = np.asarray(grad_max, np.float32)
    return gx


def pillar_max_concat_backward(grad_cat, arg, unq_inv):
    """grad_x (n, C) = grad_cat[:, :C] + (per-pillar sum of grad_cat[:, C:], sequential in ascending row, routed to arg)."""
    P, C = arg.shape
    g = np.asarray(grad_cat, np.float32)
    s = np.zeros((P, C), np.float32)
    np.add.at(s, unq_inv, g[:, C:])
    return g[:, :C] + pillar_max_backward(s, arg, g.shape[0])
