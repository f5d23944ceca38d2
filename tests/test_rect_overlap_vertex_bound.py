"""The polygon of `overlap_area` (dfu3d_amd/csrc/rect_overlap.hpp) has MAXV = 8 LDS slots per thread.  Eight is the bound
in exact arithmetic; in float32 near-coincident edges can flip signs of g, and nothing proves that a ninth vertex is
impossible, so the kernel saturates the slot.  This fuzz runs the float32 restatement
(tests/rect_overlap_ref.py) over the families on which clippers go wrong, both ways round, and asserts that the
unsaturated count never passes MAXV: the saturation is a guard that these inputs do not reach.  CPU only."""
import numpy as np

from tests import iou3d_cases as C
from tests import rect_overlap_ref as R


def test_vertex_count_stays_within_maxv_on_the_degenerate_families():
    rng = np.random.default_rng(20240)
    a, b, fam, names = C.family_pairs(rng, groups=400)
    assert len(a) >= 200000
    hist = np.zeros(2 * R.MAXV + 2, np.int64)
    worst = {}
    for x, y in ((a, b), (b, a)):
        area, reached = R.overlap_area(R.make_rect(x), R.make_rect(y))
        assert np.isfinite(area).all() and (area >= 0).all()
        hist += np.bincount(reached, minlength=len(hist))
        for k, name in enumerate(names):
            worst[name] = max(worst.get(name, 0), int(reached[fam == k].max()))
    print("vertices reached after any side -> pairs:", {k: int(v) for k, v in enumerate(hist) if v})
    print("most vertices per family:", worst)
    assert hist[R.MAXV + 1:].sum() == 0, hist
    assert hist[R.MAXV] > 0                      # the families do reach the last slot (exact arithmetic would give 4)


def test_vertex_count_through_the_fmt5_reading_and_under_a_rigid_motion():
    rng = np.random.default_rng(20241)
    a, b, _, _ = C.family_pairs(rng, groups=40)
    top = 0
    for shift, turn in (((70.0, -40.0), 0.37), ((-70.0, 40.0), np.pi / 2)):
        x, y = C.rigid_motion(a, shift, turn), C.rigid_motion(b, shift, turn)
        top = max(top, int(R.overlap_area(R.make_rect(x), R.make_rect(y))[1].max()))
    top = max(top, int(R.overlap_area(R.make_rect(C.to_fmt5(a), 5), R.make_rect(C.to_fmt5(b), 5))[1].max()))
    assert top <= R.MAXV, top
