"""Rotated / axis-aligned NMS (csrc/iou_stage.hip: k_suppress_mask, k_nms_reduce) on patterns whose keep list is written
down, not computed: axis-aligned boxes with heading 0 and power-of-two coordinates, so every area and IoU is exact in
float32.  The patterns put suppressions on the bit and word boundaries of the mask (bit 0 / 63 of a word, word 63 / 64 /
511 of a row, the 4096-box boundary of the walk's register slots) and pin the strict `>` of the threshold test.
Every pattern runs through dfu3d_nms_bev and dfu3d_nms_normal_bev, and through dfu3d_nms_bev once more with every box
turned by pi/2 and dx, dy swapped (the same footprints through another path of the clipper)."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
f32 = np.float32


def _site(k):
    """Centres of disjoint 4 m cells, away from the origin (the far-reach pattern keeps its actors there)."""
    k = np.asarray(k)
    return 8.0 + 4.0 * (k % 256), 8.0 + 4.0 * (k // 256)


def _disjoint(n, dx=2.0, dy=1.0):
    b = np.zeros((n, 7), f32)
    b[:, 0], b[:, 1] = _site(np.arange(n))
    b[:, 3], b[:, 4], b[:, 5] = dx, dy, 1.0
    return b


def _quarter_turned(b):
    q = b.copy()
    q[:, 3], q[:, 4] = b[:, 4], b[:, 3]
    q[:, 6] = f32(np.pi / 2)
    return q


def _raw(boxes, thresh, normal, mask_fill=None):
    """The C entry point on caller-made buffers: `keep` pre-filled with -1 (must stay so beyond num_keep), the mask
    workspace uninitialised or filled with a byte."""
    from dfu3d_amd import _lib, stages as st
    n = boxes.shape[0]
    tb = torch.from_numpy(np.ascontiguousarray(boxes, f32)).to(DEV) if n else torch.zeros((1, 7), dtype=torch.float32, device=DEV)
    words = max(n * ((n + 63) // 64), 1)
    mask = torch.empty(words, dtype=torch.int64, device=DEV)
    if mask_fill is not None:
        mask.view(torch.uint8).fill_(mask_fill)
    keep = torch.full((max(n, 1),), -1, dtype=torch.int64, device=DEV)
    num = torch.full((1,), -7, dtype=torch.int32, device=DEV)
    fn = _lib.lib().dfu3d_nms_normal_bev if normal else _lib.lib().dfu3d_nms_bev
    rc = fn(ctypes.c_void_p(tb.data_ptr()), n, ctypes.c_float(thresh), ctypes.c_void_p(mask.data_ptr()),
            ctypes.c_void_p(keep.data_ptr()), ctypes.c_void_p(num.data_ptr()), st._stream())
    torch.cuda.synchronize()
    assert rc == 0, rc
    k = int(num.item())
    keep = keep.cpu().numpy()
    assert 0 <= k <= n and (keep[k:] == -1).all()                 # nothing written beyond num_keep
    return keep[:k]


def _wrapped(boxes, thresh, normal):
    from dfu3d_amd import stages as st
    keep, k = st.nms_bev(torch.from_numpy(np.ascontiguousarray(boxes, f32)).to(DEV), float(thresh), normal=normal)
    return keep[:k].cpu().numpy()


def _all_paths(boxes, thresh, expected, quarter=True):
    expected = np.asarray(expected, np.int64)
    runs = [("rotated", boxes, False), ("normal", boxes, True)]
    if quarter:
        runs.append(("rotated, turned by pi/2", _quarter_turned(boxes), False))
    for what, b, normal in runs:
        got = _wrapped(b, thresh, normal)
        assert got.dtype == np.int64 and np.array_equal(got, expected), (what, len(got), len(expected),
                                                                         np.setxor1d(got, expected)[:16])


# ---- strict threshold ----------------------------------------------------------------------------------------------
# (A, B): B is the 1 x 1 box inside the 2 x 1 box A -> overlap 1, union 2, IoU exactly 0.5.  B's index sits at bit 0 and bit
# 63 of word 0, 63, 64 and 511 of A's row (index 0 has no predecessor, so word 0 has bit 1 in its place), once next to
# A and otherwise far from it.
STRICT_PAIRS = [(0, 1), (2, 63), (3, 63 * 64), (4, 63 * 64 + 63), (5, 64 * 64), (6, 64 * 64 + 63), (7, 511 * 64),
                (8, 511 * 64 + 63), (20000, 20031), (8191, 8192)]


def _strict_scene():
    n = 32768
    b = _disjoint(n)
    for i, j in STRICT_PAIRS:
        b[j] = b[i]
        b[j, 0] += f32(0.5)
        b[j, 3] = 1.0
    return b


def test_the_threshold_is_strict():
    b = _strict_scene()
    n = b.shape[0]
    # IoU == thresh does not suppress
    _all_paths(b, f32(0.5), np.arange(n), quarter=False)
    # one float32 below: every B goes, and nothing else
    below = np.nextafter(f32(0.5), f32(0))
    assert float(below) < 0.5
    expected = np.setdiff1d(np.arange(n), [j for _, j in STRICT_PAIRS])
    _all_paths(b, below, expected, quarter=False)      # sincosf(float32(pi/2)) is not (1, 0): no exact 0.5 when turned


# ---- chain ---------------------------------------------------------------------------------------------------------
def _chain(n):
    """2 x 1 boxes one metre apart along x: neighbours have IoU 1/3, second neighbours only touch."""
    b = np.zeros((n, 7), f32)
    b[:, 0] = np.arange(n)
    b[:, 3], b[:, 4], b[:, 5] = 2.0, 1.0, 1.0
    return b


@pytest.mark.parametrize("n", [64, 65, 4096, 4097, 32768])
def test_chain_keeps_every_other_box(n):
    """Every suppression was decided one step earlier, so it crosses each boundary of the walk's running set."""
    _all_paths(_chain(n), 0.25, np.arange(0, n, 2))


# ---- all identical / all disjoint ------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 64, 4097, 32768])
def test_all_identical_and_all_disjoint(n):
    same = np.repeat(_disjoint(1), n, 0)
    _all_paths(same, 0.5, [0])
    _all_paths(_disjoint(n), 0.5, np.arange(n))        # writes the whole keep array


# ---- far reach -------------------------------------------------------------------------------------------------------
def _far_reach(n):
    """Box 0 suppresses exactly the boxes j % 64 == 63 and box 4096; box 1 overlaps exactly those with j % 4096 == 0.
    The suppressed boxes are copies of their suppressor (they never act); box 4096 covers both box 0 and box 1."""
    b = _disjoint(n)
    b[0, :2] = (0.0, 0.0)                               # x in [-1, 1]
    b[1, :2] = (2.0, 0.0)                               # x in [1, 3]: touches box 0, no area in common
    j = np.arange(n)
    b[(j % 64 == 63)] = b[0]
    b[(j % 4096 == 0) & (j > 1)] = b[1]
    if n > 4096:
        b[4096] = b[0]
        b[4096, 0], b[4096, 3] = 1.0, 4.0              # 4 x 1 over both: IoU 0.5 with either
    expected = j[~((j % 64 == 63) | ((j % 4096 == 0) & (j > 1)))]
    return b, expected


@pytest.mark.parametrize("n", [4097, 32768])
def test_far_reach(n):
    b, expected = _far_reach(n)
    assert expected[0] == 0 and expected[1] == 1 and len(expected) == n - n // 64 - (n - 1) // 4096
    _all_paths(b, 0.25, expected)


# ---- workspace and outputs -------------------------------------------------------------------------------------------
def test_poisoned_workspace_and_untouched_tail():
    """k_suppress_mask leaves the words of blocks that end at or before box i unwritten (`cb * 64 + 63 <= i`); the walk
    reads such a word at most for bits of boxes it has already passed.  With the workspace full of 0xFF instead of
    whatever torch.empty holds, the result is the same; `keep` beyond num_keep stays as it was (checked in _raw)."""
    below = np.nextafter(f32(0.5), f32(0))
    strict = _strict_scene()
    for fill in (0xFF, 0x00, 0xA5):
        for normal in (False, True):
            for n in (64, 65, 4097):
                assert np.array_equal(_raw(_chain(n), 0.25, normal, fill), np.arange(0, n, 2)), (fill, normal, n)
            b, expected = _far_reach(8192 + 64)
            assert np.array_equal(_raw(b, 0.25, normal, fill), expected), (fill, normal)
            assert np.array_equal(_raw(np.repeat(_disjoint(1), 200, 0), 0.5, normal, fill), [0])
        assert np.array_equal(_raw(strict, below, False, fill),
                              np.setdiff1d(np.arange(len(strict)), [j for _, j in STRICT_PAIRS])), fill


def test_no_boxes():
    for normal in (False, True):
        assert _raw(np.zeros((0, 7), f32), 0.3, normal, 0xFF).size == 0       # num_keep == 0, keep untouched
