"""GPU: dfu3d_fov_ingest (ingest_ops.fov_ingest) against the NumPy restatement tests/ingest_ref.py -- kept rows, offsets,
flags and box counts exactly, no tolerance and no point left out.  The rows of a scene are pairwise distinct, so the kept
rows and their offsets determine the flags; they are recovered from them and compared as well."""
import numpy as np
import pytest

from tests import ingest_cases as K
from tests import ingest_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SHAPES = K.SHAPES                                      # 375 x 1242 and 900 x 1600


def _calibs(B):
    return [R.synthetic_calib(cu=SHAPES[b % 2][1] / 2 - 0.5, cv=SHAPES[b % 2][0] / 2 - 0.5, fu=720.0 + 300 * (b % 2),
                              fv=720.0 + 300 * (b % 2), yaw=0.03 * b) for b in range(B)]


def _cloud(rng, n, C):
    """Points all around the sensor: in front and behind, inside and outside the image."""
    p = np.stack([rng.uniform(-30, 45, n), rng.uniform(-25, 25, n), rng.uniform(-3, 2, n)] +
                 [rng.random(n) for _ in range(C - 3)], 1)
    return np.ascontiguousarray(p, np.float32)


def _run(scenes, calibs, shapes, boxes=None, mode=None):
    import torch
    from dfu3d_amd import ingest_ops as ops
    mode = mode if mode is not None else (ops.EMIT | (ops.COUNT if boxes is not None else 0))
    C = scenes[0].shape[1]
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)           # noqa: E731
    off = np.concatenate([[0], np.cumsum([len(s) for s in scenes])]).astype(np.int64)
    kw = {}
    if boxes is not None:
        kw = dict(boxes=t(np.concatenate([np.asarray(b, np.float64).reshape(-1, 7) for b in boxes], 0)),
                  box_off=t(np.concatenate([[0], np.cumsum([len(b) for b in boxes])]).astype(np.int32)))
    r = ops.fov_ingest(t(np.concatenate(list(scenes) + [np.zeros((0, C), np.float32)], 0)), t(off),
                       t(np.stack([c.record() for c in calibs])), t(np.array(shapes, np.int32).reshape(-1, 2)), mode=mode, **kw)
    assert int(r.status.item()) == 0
    out_off = r.out_off.cpu().numpy() if r.out_off is not None else None
    rows = r.points[:int(out_off[-1])].cpu().numpy() if out_off is not None else None
    return rows, out_off, (r.box_cnt.cpu().numpy() if r.box_cnt is not None else None)


def _void(a):
    return np.ascontiguousarray(a).view(np.dtype((np.void, a.shape[1] * 4))).reshape(-1)


def _check(scenes, calibs, shapes, boxes=None, mode=None):
    """One launch against the restatement; -> (reference flags per scene, reference counts)."""
    from dfu3d_amd import ingest_ops as ops
    rows, off, cnt = _run(scenes, calibs, shapes, boxes, mode)
    want_rows, want_off, flags, want_cnt = R.fov_ingest(scenes, calibs, shapes, boxes)
    if mode is None or mode & ops.EMIT:
        assert off.dtype == np.int64 and off.tolist() == want_off.tolist()
        assert rows.shape == want_rows.shape and np.array_equal(rows.view(np.uint32), want_rows.view(np.uint32))
        for b, (s, f) in enumerate(zip(scenes, flags)):
            if len(s) and not np.isnan(s).any():                       # distinct rows: the flags follow from the kept rows
                assert len(np.unique(_void(s))) == len(s)
                assert np.array_equal(np.isin(_void(s), _void(rows[off[b]:off[b + 1]])), f), b
    else:
        assert rows is None and off is None
    if boxes is not None and (mode is None or mode & ops.COUNT):
        assert cnt.dtype == np.int32 and np.array_equal(cnt, want_cnt)
    else:
        assert cnt is None
    return flags, want_cnt


@pytest.mark.parametrize("C", [3, 4, 5])
def test_sizes_around_the_wave_and_the_chunk(C):
    rng = np.random.default_rng(180 + C)
    # B = 1 with no point at all
    _check([_cloud(rng, 0, C)], _calibs(1), [SHAPES[0]])
    # an empty scene in the middle
    flags, _ = _check([_cloud(rng, n, C) for n in (65, 0, 257)], _calibs(3), [SHAPES[0], SHAPES[1], SHAPES[1]])
    assert flags[0].any() and not flags[0].all()
    # every size at a wave's and a chunk's edge in one batch, the two image shapes alternating
    sizes = (1, 63, 64, 65, 255, 256, 257)
    flags, _ = _check([_cloud(rng, n, C) for n in sizes], _calibs(len(sizes)), [SHAPES[b % 2] for b in range(len(sizes))])
    assert sum(int(f.sum()) for f in flags) > 100
    # and each of them alone
    for b, n in enumerate(sizes):
        _check([_cloud(rng, n, C)], _calibs(1), [SHAPES[b % 2]])
    # two empty scenes side by side inside one chunk and an empty last scene, in the rows and in the box table
    sizes = (70, 0, 0, 130, 0)
    flags, cnt = _check([_cloud(rng, n, C) for n in sizes], _calibs(len(sizes)), [SHAPES[b % 2] for b in range(len(sizes))],
                        [_boxes_for(rng, m) for m in (2, 0, 0, 3, 0)])
    assert flags[0].any() and flags[3].any() and len(cnt) == 5


def test_a_scan_that_carries_across_more_than_1024_chunks():
    from dfu3d_amd import ingest_ops as ops
    rng = np.random.default_rng(1899)
    n = ops.CHUNK * 1024 + 300                         # 1026 chunks: the second pass of the one-workgroup scan
    flags, _ = _check([_cloud(rng, 700, 4), _cloud(rng, n, 4), _cloud(rng, 90, 4)], _calibs(3), [SHAPES[0], SHAPES[1], SHAPES[0]])
    assert 0.05 < flags[1][ops.CHUNK * 1024:].mean() and flags[1].sum() > ops.CHUNK * 64


def test_planted_points():
    rng = np.random.default_rng(1881)
    c0 = R.synthetic_calib(yaw=0.0)                    # rect z = x - float32(0.27), exactly
    shape = SHAPES[0]
    front = np.ascontiguousarray(np.stack([rng.uniform(6, 40, 300), rng.uniform(-1, 1, 300), rng.uniform(-0.5, 0.2, 300),
                                           rng.random(300)], 1), np.float32)
    behind = front.copy()
    behind[:, 0] = -front[:, 0]
    with np.errstate(all="ignore"):
        img, depth = c0.lidar_to_img(behind[:, :3])
    inside = (img[:, 0] >= 0) & (img[:, 0] < shape[1]) & (img[:, 1] >= 0) & (img[:, 1] < shape[0])
    assert inside.sum() > 100 and (depth[inside] < 0).all()        # behind the camera, yet u and v inside the image
    special = _cloud(rng, 40, 4)
    special[0, :3] = [np.float32(0.27), 0.5, 0.1]                   # rect z exactly 0
    special[1, :3] = [np.float32(0.27), 0.0, 0.0]
    special[2, 0] = np.nan
    special[3, 1] = np.nan
    special[4, 2] = np.nan
    special[5] = [10.0, 0.1, -0.2, np.nan]                          # a NaN that is no coordinate: kept, bit for bit
    special[6, :3] = [np.inf, 0.0, 0.0]
    special[7, :3] = [-0.0, 0.0, 0.0]
    assert c0.lidar_to_rect(special[:2, :3])[:, 2].tolist() == [0.0, 0.0]
    flags, _ = _check([front, behind, special], [c0, c0, c0], [shape, shape, shape])
    assert flags[0].all() and not flags[1].any()                    # a scene kept whole, a scene dropped whole
    assert not flags[2][2:5].any() and flags[2][5]
    # the same points under the other image shape in the same batch: the shapes are per scene
    wide = _cloud(rng, 400, 4)
    flags, _ = _check([wide, wide.copy()], [c0, c0], [SHAPES[0], SHAPES[1]])
    assert flags[0].sum() != flags[1].sum()


def _boxes_for(rng, m, heading=True):
    b = np.zeros((m, 7))
    b[:, 0], b[:, 1], b[:, 2] = rng.uniform(5, 35, m), rng.uniform(-8, 8, m), rng.uniform(-1.5, 0.5, m)
    b[:, 3:6] = rng.uniform(1.0, 6.0, (m, 3))
    b[:, 6] = rng.uniform(-4, 4, m) if heading else 0.0
    return b


def test_box_counts_and_modes():
    from dfu3d_amd import ingest_ops as ops
    rng = np.random.default_rng(1882)
    calibs = _calibs(4)
    shapes = [SHAPES[0], SHAPES[1], SHAPES[0], SHAPES[1]]
    scenes = [_cloud(rng, 6000, 4), _cloud(rng, 0, 4), _cloud(rng, 2500, 4), _cloud(rng, 257, 4)]
    overlap = np.array([[12.0, 0.0, -0.5, 8.0, 6.0, 4.0, 0.3], [13.0, 1.0, -0.5, 8.0, 6.0, 4.0, -0.4],      # share points
                        [20.0, 3.0, 40.0, 2.0, 2.0, 2.0, 0.0]])                                             # holds no point
    boxes = [overlap, _boxes_for(rng, 5), _boxes_for(rng, 100), np.zeros((0, 7))]      # scene 1: boxes and no points
    _, cnt = _check(scenes, calibs, shapes, boxes)
    assert cnt[0] > 10 and cnt[1] > 10 and cnt[2] == 0 and (cnt[3:8] == 0).all() and (cnt[8:] > 0).sum() > 20
    kept0 = scenes[0][R.fov_flag(scenes[0], calibs[0], shapes[0])]
    from oracle.gtdb_oracle import points_in_boxes_cpu
    assert (points_in_boxes_cpu(kept0, overlap[:2]).sum(0) == 2).sum() > 5
    # EMIT alone, COUNT alone, both: each gives what both give
    _check(scenes, calibs, shapes, boxes, mode=ops.EMIT)
    _check(scenes, calibs, shapes, boxes, mode=ops.COUNT)
    _check(scenes, calibs, shapes, boxes, mode=ops.EMIT | ops.COUNT)
    # no box at all
    _, cnt = _check(scenes, calibs, shapes, [np.zeros((0, 7))] * 4)
    assert cnt.shape == (0,)
    _check(scenes, calibs, shapes, [np.zeros((0, 7))] * 4, mode=ops.COUNT)
    # other point widths
    for C in (3, 5):
        _check([_cloud(rng, 900, C), _cloud(rng, 1, C)], calibs[:2], shapes[:2], [_boxes_for(rng, 7), _boxes_for(rng, 2)])


def test_the_frames_of_g18():
    G = K.golden()
    frames = K.golden_frames(G)
    boxes = [G['f%d_ann_gt_boxes_lidar' % i] for i in range(3)]
    flags, cnt = _check([f['points'] for f in frames], [K.calib_of(f) for f in frames], [f['shape'] for f in frames], boxes)
    for i in range(3):
        assert np.array_equal(flags[i], G['f%d_fov_flag' % i])                        # the reference's own flags
    want = np.concatenate([G['f%d_ann_num_points_in_gt' % i][:len(boxes[i])] for i in range(3)])
    assert np.array_equal(cnt, want) and len(want) == 9                              # and its hull counts


def test_one_launch_equals_six_and_runs_repeat():
    rng = np.random.default_rng(1883)
    sizes = (700, 0, 257, 1, 1300, 64)
    scenes = [_cloud(rng, n, 4) for n in sizes]
    calibs = _calibs(6)
    shapes = [SHAPES[b % 2] for b in range(6)]
    boxes = [_boxes_for(rng, m) for m in (4, 2, 0, 1, 9, 3)]
    rows, off, cnt = _run(scenes, calibs, shapes, boxes)
    rows2, off2, cnt2 = _run(scenes, calibs, shapes, boxes)
    assert rows.tobytes() == rows2.tobytes() and off.tobytes() == off2.tobytes() and cnt.tobytes() == cnt2.tobytes()
    single = [_run([scenes[b]], [calibs[b]], [shapes[b]], [boxes[b]]) for b in range(6)]
    assert b"".join(s[0].tobytes() for s in single) == rows.tobytes()
    assert np.concatenate([[0], np.cumsum([s[1][1] for s in single])]).astype(np.int64).tobytes() == off.tobytes()
    assert b"".join(s[2].tobytes() for s in single) == cnt.tobytes()


def test_status_bits_and_a_capacity_beyond_the_scenes():
    import torch
    from dfu3d_amd import ingest_ops as ops
    rng = np.random.default_rng(1884)
    pts = _cloud(rng, 600, 4)
    c = _calibs(2)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)           # noqa: E731
    rec = t(np.stack([x.record() for x in c]))
    # the array is longer than the scenes: rows at or beyond point_off[B] are never kept
    r = ops.fov_ingest(t(pts), t(np.array([0, 200, 450], np.int64)), rec, t(np.array([SHAPES[0], SHAPES[1]], np.int32)))
    want, off, _, _ = R.fov_ingest([pts[:200], pts[200:450]], c, [SHAPES[0], SHAPES[1]])
    assert int(r.status.item()) == 0 and r.out_off.cpu().numpy().tolist() == off.tolist()
    assert np.array_equal(r.points[:off[-1]].cpu().numpy(), want)
    # a negative image side: the scene keeps nothing, the other scene is as it was
    r = ops.fov_ingest(t(pts), t(np.array([0, 200, 600], np.int64)), rec, t(np.array([[-1, 1242], SHAPES[1]], np.int32)))
    want, off, _, _ = R.fov_ingest([pts[:0], pts[200:]], c[1:] * 2, [SHAPES[1], SHAPES[1]])
    assert int(r.status.item()) == ops.ST_SHAPE and r.out_off.cpu().numpy().tolist() == [0, 0, off[-1]]
    assert np.array_equal(r.points[:off[-1]].cpu().numpy(), want)
    # a table that does not ascend is flagged, into the caller's status word, ORed
    status = torch.full((1,), 8, dtype=torch.int32, device=DEV)
    r = ops.fov_ingest(t(pts), t(np.array([0, 400, 300], np.int64)), rec, t(np.array([SHAPES[0], SHAPES[1]], np.int32)),
                       status=status)
    assert r.status is status and int(status.item()) == 8 | ops.ST_OFFSETS
