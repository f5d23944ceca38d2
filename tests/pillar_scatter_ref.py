"""NumPy restatement of the pillar-to-BEV scatter (include/dfu3d_bev.h) and its backward, with the stage's rules: a row
outside the canvas is dropped (ST_BAD_COORD), the highest row index owns a cell that several rows name (ST_DUPLICATE),
values move as 32-bit words.  Checker only; the loops are over rows, not over cells."""
import numpy as np

ST_BAD_COORD, ST_DUPLICATE = 1, 2


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(bits(a), bits(b))


def cells(coords, batch_size, grid, n=None):
    """coords (P, 3|4) -> (cell (n) int64 with -1 for a row outside the canvas, over the first n rows)."""
    nx, ny, nz = (int(v) for v in grid)
    c = np.asarray(coords)[:len(coords) if n is None else n].astype(np.int64)
    b, x, y = c[:, 0], c[:, -1], c[:, -2]
    z = c[:, 1] if c.shape[1] == 4 else np.zeros(len(c), np.int64)
    ok = (b >= 0) & (b < batch_size) & (z >= 0) & (z < nz) & (y >= 0) & (y < ny) & (x >= 0) & (x < nx)
    return np.where(ok, ((b * nz + z) * ny + y) * nx + x, -1)


def scatter(features, coords, batch_size, grid, n_pillars=None):
    """-> canvas float32 (B, C * nz, ny, nx), cell_map int32 (B * nz * ny * nx), status."""
    nx, ny, nz = (int(v) for v in grid)
    f = bits(features)
    n = len(f) if n_pillars is None else max(0, min(int(n_pillars), len(f)))
    C = f.shape[1]
    cell = cells(coords, batch_size, grid, n)
    n_cells = batch_size * nz * ny * nx
    cell_map = np.full(n_cells, -1, np.int32)
    status = ST_BAD_COORD if (cell < 0).any() else 0
    rows = np.flatnonzero(cell >= 0)
    if len(np.unique(cell[rows])) != len(rows):
        status |= ST_DUPLICATE
    cell_map[cell[rows]] = rows                          # ascending rows, sequential assignment: the highest row stays
    canvas = np.zeros((batch_size, C, nz * ny * nx), np.uint32)
    own = np.flatnonzero(cell_map >= 0)
    canvas[own // (nz * ny * nx), :, own % (nz * ny * nx)] = f[cell_map[own]]
    return canvas.view(np.float32).reshape(batch_size, C * nz, ny, nx), cell_map, status


def scatter_backward(grad_canvas, coords, batch_size, grid, cell_map, n_rows, n_pillars=None):
    """-> grad_features float32 (n_rows, C): the gradient at the row's cell if the row owns it, +0.0 otherwise.  Rows at or
    beyond n_pillars are not touched by the stage; they are +0.0 here."""
    nx, ny, nz = (int(v) for v in grid)
    vol = nz * ny * nx
    g = bits(grad_canvas).reshape(batch_size, -1, vol)
    n = n_rows if n_pillars is None else max(0, min(int(n_pillars), n_rows))
    cell = cells(coords, batch_size, grid, n)
    out = np.zeros((n_rows, g.shape[1]), np.uint32)
    own = np.flatnonzero((cell >= 0) & (cell_map[np.maximum(cell, 0)] == np.arange(n)))
    out[own] = g[cell[own] // vol, :, cell[own] % vol]
    return out.view(np.float32)


def sparse(canvas):
    """A canvas as (flat indices of the words that are not +0.0, their values, shape)."""
    w = bits(canvas).reshape(-1)
    idx = np.flatnonzero(w)
    return idx.astype(np.int64), np.asarray(canvas, np.float32).reshape(-1)[idx], np.array(canvas.shape, np.int64)


def dense(idx, val, shape):
    out = np.zeros(int(np.prod(shape)), np.float32)
    out[idx] = val
    return out.reshape([int(v) for v in shape])
