"""The rules of dfu3d_amd/csrc/dfu3d_spc.h restated sequentially in NumPy: SITES, THE GEOMETRY, THE OUTPUT SITES, THE
TABLES, THE SUM, THE FEATURE GRADIENT and THE WEIGHT GRADIENT.  Nothing here shares code with the package.

fmaf: an EXACT float32 fused multiply-add for arrays.  The product of two float32 is exact in float64 (48 bits); the sum
with the float32 addend is formed in float64 with round-to-odd (TwoSum gives the error of the rounded sum; an inexact sum
whose last bit is even moves to its odd neighbour on the side of the error), and a 53-bit round-to-odd result rounds to
the same float32 as the exact sum does (53 >= 2 * 24 + 2).  A plain float64 add followed by the cast is wrong at halfway
cases; tests/test_sparse_conv_host.py compares this one against libm's fmaf on random and on constructed halfway cases."""
import numpy as np

f32, f64 = np.float32, np.float64
BAD_COORD, DUP_SITE = 1, 2
WGRAD_CHUNK = 1024


def fmaf(a, b, c):
    p = np.asarray(a, f32).astype(f64) * np.asarray(b, f32).astype(f64)
    c = np.asarray(c, f32).astype(f64)
    p, c = np.broadcast_arrays(p, c)
    s = p + c
    bb = s - p
    e = (p - (s - bb)) + (c - bb)
    even = (np.ascontiguousarray(s).view(np.int64) & 1) == 0
    fix = (e != 0) & even & np.isfinite(s)
    s = np.where(fix, np.nextafter(s, np.where(e > 0, np.inf, -np.inf)), s)
    return s.astype(f32)


def out_shape(shape, k, s, p):
    return tuple((d + 2 * pp - kk) // ss + 1 for d, kk, ss, pp in zip(shape, k, s, p))


def offsets(k):
    return [(jz, jy, jx) for jz in range(k[0]) for jy in range(k[1]) for jx in range(k[2])]


def sites(indices, count, B, shape):
    """-> (owner {(b, z, y, x): row}, status) of the rows below the count."""
    n = min(max(int(count), 0), len(indices))
    owner, status = {}, 0
    for i in range(n):
        b, z, y, x = (int(v) for v in indices[i])
        if not (0 <= b < B and 0 <= z < shape[0] and 0 <= y < shape[1] and 0 <= x < shape[2]):
            status |= BAD_COORD
        elif (b, z, y, x) in owner:
            status |= DUP_SITE
        else:
            owner[(b, z, y, x)] = i
    return owner, status


def downsample(indices, count, B, shape, k, s, p):
    """THE OUTPUT SITES of a strided layer -> out_indices int32 (n_out, 4) in first-seen order."""
    owner, _ = sites(indices, count, B, shape)
    osh = out_shape(shape, k, s, p)
    seen, out = set(), []
    for i in range(min(max(int(count), 0), len(indices))):
        cell = tuple(int(v) for v in indices[i])
        if owner.get(cell) != i:
            continue
        for j in offsets(k):
            t = [cell[1 + a] + p[a] - j[a] for a in range(3)]
            if any(t[a] < 0 or t[a] % s[a] for a in range(3)):
                continue
            o = tuple(t[a] // s[a] for a in range(3))
            if any(o[a] >= osh[a] for a in range(3)):
                continue
            key = (cell[0],) + o
            if key not in seen:
                seen.add(key)
                out.append(key)
    return np.array(out, np.int32).reshape(-1, 4)


def tables(in_indices, in_count, out_indices, out_count, B, shape, k, s, p):
    """THE TABLES -> nbr int32 (len(out_indices), KV), inv int32 (len(in_indices), KV)."""
    osh = out_shape(shape, k, s, p)
    own_in, _ = sites(in_indices, in_count, B, shape)
    own_out, _ = sites(out_indices, out_count, B, osh)
    offs = offsets(k)
    nbr = np.full((len(out_indices), len(offs)), -1, np.int32)
    inv = np.full((len(in_indices), len(offs)), -1, np.int32)
    for cell, o in own_out.items():
        for K, j in enumerate(offs):
            r = own_in.get((cell[0],) + tuple(cell[1 + a] * s[a] - p[a] + j[a] for a in range(3)), -1)
            nbr[o, K] = r
            if r >= 0:
                inv[r, K] = o
    return nbr, inv


def plan(indices, count, B, shape, layers):
    """layers: (in_level, kernel, stride, padding, subm) -> (levels [(indices, shape)], per layer (nbr, inv, in_level,
    out_level), status): levels at exact size, a new one per distinct strided (in_level, kernel, stride, padding)."""
    n = min(max(int(count), 0), len(indices))
    _, status = sites(indices, n, B, shape)
    levels, made, out = [(np.asarray(indices[:n], np.int32), tuple(shape))], {}, []
    for lv, k, s, p, subm in layers:
        idx, sh = levels[lv]
        if subm:
            oj = lv
        else:
            key = (lv, tuple(k), tuple(s), tuple(p))
            if key not in made:
                made[key] = len(levels)
                levels.append((downsample(idx, len(idx), B, sh, k, s, p), out_shape(sh, k, s, p)))
            oj = made[key]
        out.append(tables(idx, len(idx), levels[oj][0], len(levels[oj][0]), B, sh, k, s, p) + (lv, oj))
    return levels, out, status


def gather_sum(src, tab, w_nkm):
    """out[r][n]: acc = +0.0; K ascending, m ascending: acc = fmaf(src[tab[r][K]][m], w_nkm[n][K][m], acc)."""
    R, KV = tab.shape
    N, _, M = w_nkm.shape
    acc = np.zeros((R, N), f32)
    for K in range(KV):
        rows = tab[:, K]
        g = np.where((rows >= 0)[:, None], src[np.maximum(rows, 0)] if len(src) else np.zeros((R, M), f32), f32(0.0))
        for m in range(M):
            acc = fmaf(g[:, m:m + 1], w_nkm[None, :, K, m], acc)
    return acc


def forward(x, nbr, w):
    """THE SUM.  w (Cout, KV, Cin)."""
    return gather_sum(x, nbr, w)


def dgrad(dy, inv, w):
    """THE FEATURE GRADIENT.  w (Cout, KV, Cin)."""
    return gather_sum(dy, inv, np.ascontiguousarray(w.transpose(2, 1, 0)))


def wgrad(x, dy, nbr, chunk=WGRAD_CHUNK):
    """THE WEIGHT GRADIENT -> (Cout, KV, Cin)."""
    n_out, KV = nbr.shape
    cin, cout = x.shape[1], dy.shape[1]
    total = np.zeros((cout, KV, cin), f64)
    for o0 in range(0, n_out, chunk):
        acc = np.zeros((cout, KV, cin), f32)
        for o in range(o0, min(o0 + chunk, n_out)):
            rows = nbr[o]
            g = np.where((rows >= 0)[:, None], x[np.maximum(rows, 0)] if len(x) else np.zeros((KV, cin), f32), f32(0.0))
            acc = fmaf(dy[o][:, None, None], g[None, :, :], acc)
        total = total + acc.astype(f64)
    return total.astype(f32)


def canon(a):
    """float32 values with the sign of zero removed, as bit patterns."""
    a = np.asarray(a, f32) + f32(0.0)
    return np.ascontiguousarray(a).view(np.uint32)
