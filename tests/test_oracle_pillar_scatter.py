"""CPU: the NumPy restatement of the pillar scatter (tests/pillar_scatter_ref.py) against golden G16(a) -- the reference's
PointPillarScatter / PointPillarScatter3d run unmodified -- bit for bit, canvas and gradient."""
import json

import numpy as np
import pytest

from tests import centerpoint_cases as K
from tests import pillar_scatter_ref as R


@pytest.fixture(scope="module")
def g16():
    g = K.golden()
    return g, json.loads(bytes(g["meta"]).decode())


@pytest.mark.parametrize("case", K.SCATTER_CASES, ids=[c[0] for c in K.SCATTER_CASES])
def test_restatement_equals_the_reference_canvas(g16, case):
    g, _ = g16
    name, _, B, C, grid, P, _ = case
    f, coords = g[name + '_features'], g[name + '_coords']
    assert f.shape == (P, C) and coords.shape == (P, 4) and coords.dtype == np.int32
    want = R.dense(g[name + '_canvas_idx'], g[name + '_canvas_val'], g[name + '_canvas_shape'])
    canvas, cell_map, status = R.scatter(f, coords, B, grid)
    assert status == 0 and (cell_map >= 0).sum() == P
    assert canvas.shape == (B, C * grid[2], grid[1], grid[0]) and R.same_bits(canvas, want)
    assert np.isnan(canvas).sum() == 1 and np.isinf(canvas).sum() == 1          # the planted values arrived
    assert (R.bits(canvas) == 0x80000000).sum() == 1                             # and the -0.0


def test_restated_backward_equals_the_reference_gradient(g16):
    g, meta = g16
    name, _, B, C, grid, P, _ = next(c for c in K.SCATTER_CASES if c[0] == K.GRAD_CASE)
    coords = g[name + '_coords']
    shape = [int(v) for v in g[name + '_canvas_shape']]
    gc = np.random.default_rng(meta['grad_seed']).standard_normal(shape).astype(np.float32)
    _, cell_map, _ = R.scatter(g[name + '_features'], coords, B, grid)
    got = R.scatter_backward(gc, coords, B, grid, cell_map, P)
    assert R.same_bits(got, g[name + '_grad_features']) and np.abs(got).min() > 0


def test_duplicate_and_drop_rules():
    """What the reference does not define: the highest row wins, rows outside the canvas are dropped."""
    f = np.arange(1, 13, dtype=np.float32).reshape(6, 2)
    coords = np.array([[0, 0, 1, 1], [0, 0, 1, 1], [0, 0, 2, 0], [1, 0, 0, 0], [0, 0, 3, 0], [0, 0, 1, 1]], np.int32)
    canvas, cell_map, status = R.scatter(f, coords, 1, (2, 3, 1))
    assert status == R.ST_BAD_COORD | R.ST_DUPLICATE
    assert list(cell_map) == [-1, -1, -1, 5, 2, -1]
    assert list(canvas[0, :, 1, 1]) == [11, 12] and list(canvas[0, :, 2, 0]) == [5, 6] and np.count_nonzero(canvas) == 4
    gc = np.arange(100, 112, dtype=np.float32).reshape(1, 2, 3, 2)
    gf = R.scatter_backward(gc, coords, 1, (2, 3, 1), cell_map, 6)
    assert not R.bits(gf[[0, 1, 3, 4]]).any()
    assert list(gf[5]) == [103, 109] and list(gf[2]) == [104, 110]
    # the capacity form: rows at or beyond n_pillars are not read
    c2, m2, s2 = R.scatter(f, coords, 1, (2, 3, 1), n_pillars=3)
    assert s2 == R.ST_DUPLICATE and list(m2) == [-1, -1, -1, 1, 2, -1] and list(c2[0, :, 1, 1]) == [3, 4]
