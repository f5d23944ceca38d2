"""NumPy float32 restatements of the PointNet++ ops of include/dfu3d_pn2.h, and the case tables of their tests.
Importable without the reference and without a GPU.  Every array operation below is one float32 operation per element,
in the order of the C header's expressions (NumPy does not contract a product and a sum)."""
import numpy as np

F32 = np.float32

# (B, N, npoint): farthest point sampling
FPS_CASES = [(1, 1, 1), (2, 63, 63), (3, 1000, 37), (2, 1025, 256)]
# the register shapes of dfu3d_pn2_fps no case above launches: <1024,2> (2049 > 2048 takes <1024,4>), <1024,4> at its upper
# edge, <1024,8> on both of its edges
FPS_SHAPE_CASES = [(2, 2049, 64), (2, 4096, 64), (2, 4097, 64), (2, 8192, 64)]
# N per kernel of the dispatch ladder, for the lattice cloud: <256,1>, <256,4>, <1024,2>, <1024,4>, <1024,8>, <1024,16>, big
FPS_LATTICE_N = [200, 1000, 2000, 4000, 8000, 16000, 17000]
FPS_LEVEL1 = (2, 16384, 4096)                # the configuration's first level
FPS_BIG = (1, 16384 + 1000, 96)              # above DFU3D_PN2_FPS_ONCHIP: the form with the minima in the scratch
BALL_N = [1, 64, 65, 1000]
BALL_M = [1, 70]
BALL_NSAMPLE_ALL = [1, 16, 33]
GROUP_C = [1, 3, 67]
NN_M = [1, 2, 3, 64, 257]

# the small model of golden G19
G19_CFG = {
    'SA_CONFIG': {'NPOINTS': [64, 16], 'RADIUS': [[0.5, 1.0], [1.0, 2.0]], 'NSAMPLE': [[4, 8], [4, 8]],
                  'MLPS': [[[8, 16], [8, 16]], [[16, 32], [16, 32]]]},
    'FP_MLPS': [[16, 16], [16, 16]],
}
G19_B, G19_N, G19_EXTRA = 2, 256, 1
# BACKBONE_3D of pointrcnn_nuscenes2kitti.yaml
FULL_CFG = {
    'SA_CONFIG': {'NPOINTS': [4096, 1024, 256, 64], 'RADIUS': [[0.1, 0.5], [0.5, 1.0], [1.0, 2.0], [2.0, 4.0]],
                  'NSAMPLE': [[16, 32], [16, 32], [16, 32], [16, 32]],
                  'MLPS': [[[16, 16, 32], [32, 32, 64]], [[64, 64, 128], [64, 96, 128]],
                           [[128, 196, 256], [128, 196, 256]], [[256, 256, 512], [256, 384, 512]]]},
    'FP_MLPS': [[128, 128], [256, 256], [512, 512], [512, 512]],
}
FULL_INPUT_CHANNELS = 4


def cloud(seed, B, N, scale=4.0):
    """(B, N, 3) float32 from a continuous distribution."""
    return (np.random.default_rng(seed).normal(0.0, 1.0, (B, N, 3)) * scale).astype(F32)


def lattice_cloud(seed, B, N, pitch=0.25, span=2):
    """(B, N, 3) float32 on a lattice: integer multiples of `pitch` in [-span, span] * pitch, so every float32 operation of
    a squared distance is exact, points repeat ((2 * span + 1) ** 3 cells) and the maxima of farthest point sampling tie."""
    return (np.random.default_rng(seed).integers(-span, span + 1, (B, N, 3)) * pitch).astype(F32)


def sqdist(a, b):
    """a (..., 3), b (..., 3) -> (a.x-b.x)*(a.x-b.x) + (a.y-b.y)*(a.y-b.y) + (a.z-b.z)*(a.z-b.z), float32, left to right."""
    a, b = np.asarray(a, F32), np.asarray(b, F32)
    dx, dy, dz = a[..., 0] - b[..., 0], a[..., 1] - b[..., 1], a[..., 2] - b[..., 2]
    with np.errstate(all='ignore'):
        return (dx * dx + dy * dy) + dz * dz


def fps(xyz, npoint, ties=None):
    """xyz (B, N, 3) -> idx int32 (B, npoint), new_xyz (B, npoint, 3).  First pick 0, running minimum from 1e10, then the
    largest running minimum, the LOWEST index among equals.  ties: a list that receives (b, step) of every step with more
    than one candidate at the maximum."""
    xyz = np.asarray(xyz, F32)
    B, N, _ = xyz.shape
    idx = np.zeros((B, npoint), np.int32)
    for b in range(B):
        run = np.full(N, 1e10, F32)
        old = 0
        for s in range(1, npoint):
            d = sqdist(xyz[b], xyz[b, old])
            with np.errstate(invalid='ignore'):
                run = np.where(d < run, d, run)
            old = int(np.argmax(run))                    # the first of the maxima
            if ties is not None and int((run == run[old]).sum()) > 1:
                ties.append((b, s))
            idx[b, s] = old
    return idx, np.take_along_axis(xyz, idx[..., None].astype(np.int64), axis=1)


def ball_query(xyz, centres, radius, nsample):
    """-> int32 (B, M, nsample): the first nsample indices, ascending, with d2 < radius * radius (strict, float32); the
    rest the first hit; zeros without one."""
    xyz, centres = np.asarray(xyz, F32), np.asarray(centres, F32)
    B, M = centres.shape[:2]
    r2 = F32(radius) * F32(radius)
    out = np.zeros((B, M, nsample), np.int32)
    for b in range(B):
        for m in range(M):
            with np.errstate(invalid='ignore'):
                hits = np.nonzero(sqdist(centres[b, m], xyz[b]) < r2)[0][:nsample]
            if len(hits):
                out[b, m] = hits[0]
                out[b, m, :len(hits)] = hits
    return out


def group(xyz, centres, features, idx, use_xyz=True):
    """-> (B, (3 if use_xyz) + C, M, nsample): xyz[idx] - centre, then features[idx]."""
    parts = []
    ii = idx.astype(np.int64)
    B = idx.shape[0]
    if use_xyz:
        g = np.stack([np.asarray(xyz, F32)[b][ii[b]] for b in range(B)])            # (B, M, ns, 3)
        parts.append((g - np.asarray(centres, F32)[:, :, None, :]).transpose(0, 3, 1, 2))
    if features is not None:
        parts.append(np.stack([np.asarray(features, F32)[b][:, ii[b]] for b in range(B)]))
    return np.concatenate(parts, axis=1)


def three_nn(unknown, known):
    """-> dist float32 (B, n, 3) = sqrt(squared distance), idx int32 (B, n, 3)."""
    d2, idx = three_nn_sq(unknown, known)
    return np.sqrt(d2), idx


def three_nn_sq(unknown, known):
    """-> squared distance float32 (B, n, 3), idx int32 (B, n, 3): a cascade of strict < over ascending k (= a stable
    sort); unfilled ranks +inf, index 0."""
    unknown, known = np.asarray(unknown, F32), np.asarray(known, F32)
    B, n = unknown.shape[:2]
    d2 = np.full((B, n, 3), np.inf, F32)
    idx = np.zeros((B, n, 3), np.int32)
    for b in range(B):
        for j in range(n):
            d = sqdist(unknown[b, j], known[b])
            order = np.argsort(d, kind='stable')
            order = order[d[order] < np.inf][:3]
            d2[b, j, :len(order)] = d[order]
            idx[b, j, :len(order)] = order
    return d2, idx


def three_interpolate(features, idx, weight):
    """-> (B, C, n): w0 * f[i0] + w1 * f[i1] + w2 * f[i2], products rounded, summed left to right."""
    features, weight = np.asarray(features, F32), np.asarray(weight, F32)
    B = features.shape[0]
    f = [np.stack([features[b][:, idx[b, :, r].astype(np.int64)] for b in range(B)]) for r in range(3)]
    w = [weight[:, None, :, r] for r in range(3)]
    return (w[0] * f[0] + w[1] * f[1]) + w[2] * f[2]


def gather_backward(grad_out, idx, N, weight=None, k=1):
    """grad_out (B, C, E / k), idx (B, E) -> (B, C, N): np.add.at adds sequentially in entry order, from +0.0, float32."""
    grad_out = np.asarray(grad_out, F32)
    B, C = grad_out.shape[:2]
    g = grad_out.reshape(B, C, -1)
    flat = idx.reshape(B, -1).astype(np.int64)
    E = flat.shape[1]
    out = np.zeros((B, C, N), F32)
    for b in range(B):
        vals = g[b][:, np.arange(E) // k]                                         # (C, E)
        if weight is not None:
            vals = np.asarray(weight, F32).reshape(B, E)[b][None, :] * vals
        for c in range(C):
            np.add.at(out[b, c], flat[b], vals[c])
    return out


def invert(idx, N):
    """idx (E) -> csr (N + 1), list (E): the entries of a source in ascending entry number."""
    order = np.argsort(idx, kind='stable').astype(np.int32)
    csr = np.zeros(N + 1, np.int32)
    csr[1:] = np.cumsum(np.bincount(idx, minlength=N))
    return csr, order
