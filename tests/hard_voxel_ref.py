"""A sequential NumPy / Python restatement of THE RULE and THE MEAN of csrc/dfu3d_hvox.h (transform_points_to_voxels and
MeanVFE for a batch): rows taken one by one in their order, every float32 operation done on its own."""
import numpy as np

BAD_POINT, BAD_COUNT = 1, 2
F32 = np.float32


def cells(xyz, range_min, voxel_size, grid):
    """xyz float32 (n, 3) -> (inside bool (n), cell int64 (n, 3) as [x, y, z], finite bool (n)): c_j = floor(fl32(fl32(p_j -
    range_min_j) / voxel_size_j)), OUT where a c_j is NaN, negative or >= fl32(grid_j), compared as floats."""
    xyz = np.asarray(xyz, F32).reshape(-1, 3)
    rmin, vs = np.asarray(range_min, F32), np.asarray(voxel_size, F32)
    inside = np.ones(len(xyz), bool)
    cell = np.zeros((len(xyz), 3), np.int64)
    with np.errstate(all="ignore"):
        for j in range(3):
            d = np.subtract(xyz[:, j], rmin[j], dtype=F32)
            q = np.floor(np.divide(d, vs[j], dtype=F32))
            ok = (q >= F32(0.0)) & (q < F32(int(grid[j])))      # a NaN fails both
            inside &= ok
            cell[:, j] = np.where(ok, q, 0).astype(np.int64)
    finite = np.isfinite(xyz).all(axis=1)
    return inside & finite, cell, finite


def hard_voxels(points, point_cnt, range_min, voxel_size, grid, max_points, max_voxels, out_cols=None):
    """points float32 (R, 1 + C); point_cnt (B) -> dict of the padded outputs of dfu3d_hard_voxels, V_cap rows."""
    points = np.asarray(points, F32)
    R, C = points.shape[0], points.shape[1] - 1
    B, T = len(point_cnt), int(max_points)
    oc = C if out_cols is None else int(out_cols)
    cap = min(B * int(max_voxels), R)
    status = 0
    out = {"voxel_cnt": np.zeros(B, np.int32), "voxel_coords": np.full((cap, 4), -1, np.int32),
           "voxel_num_points": np.zeros(cap, np.int32), "voxels": np.zeros((cap, T, oc), F32),
           "point_voxel": np.full(R, -1, np.int32)}
    inside, cell, finite = cells(points[:, 1:4], range_min, voxel_size, grid)
    start, nv = 0, 0
    for b in range(B):
        n = int(point_cnt[b])
        if n < 0:
            status |= BAD_COUNT
            n = 0
        if start + n > R:
            status |= BAD_COUNT
            n = R - start
        table, made = {}, 0
        for g in range(start, start + n):
            if not finite[g]:
                status |= BAD_POINT
            if not inside[g]:
                continue
            key = (int(cell[g, 2]), int(cell[g, 1]), int(cell[g, 0]))
            v = table.get(key)
            if v is None:
                if made >= max_voxels:
                    continue
                v = nv + made
                made += 1
                table[key] = v
                out["voxel_coords"][v] = (b,) + key
            s = out["voxel_num_points"][v]
            if s < T:
                out["voxels"][v, s] = points[g, 1:1 + oc]
                out["voxel_num_points"][v] = s + 1
                out["point_voxel"][g] = v
        out["voxel_cnt"][b] = made
        nv += made
        start += n
    out["n_voxels"] = np.array([nv], np.int32)
    out["status"] = np.array([status], np.int32)
    out["voxel_mean"] = mean(out["voxels"], out["voxel_num_points"])
    return out


def mean(voxels, num_points):
    """THE MEAN: acc = +0.0f, acc = fl32(acc + v) over the stored rows in slot order, fl32(acc / (float)max(count, 1))."""
    voxels = np.asarray(voxels, F32)
    V, T, C = voxels.shape
    acc = np.zeros((V, C), F32)
    with np.errstate(all="ignore"):
        for s in range(T):
            live = (np.asarray(num_points) > s)[:, None]
            acc = np.where(live, np.add(acc, voxels[:, s, :], dtype=F32), acc)
        return np.divide(acc, np.maximum(np.asarray(num_points), 1).astype(F32)[:, None], dtype=F32)
