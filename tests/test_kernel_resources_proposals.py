"""CPU-only guard on the proposal-stage kernels (proposal_stage.hip): the gfx950 code object hipcc makes with the
product's flags holds exactly the expected k_pr_* kernels, uses no scratch memory, spills no registers and uses the LDS
each is designed around:

  k_pr_order   256 digits x W waves of counts and the W wave totals of the scan, W = DFU3D_PROP_SORT_THREADS / 64
                                                                                            4 * (256 * 16 + 16) = 16 448 bytes
  k_pr_nms     the polygon planes of rect_overlap.hpp (4 planes x 8 vertices x 256 threads x 4 bytes = 32 768), the kept
               list (DFU3D_PROP_MAX_POST Rects), the block's DFU3D_PROP_BLOCK_ROWS candidates (Rect and point index) and
               as many diagonal words, the queue of the pairs to clip (DFU3D_PROP_QUEUE_PAIRS entries of 2 bytes), the
               word of the suppressed candidates and the queue's two counters (8 bytes each)                 = 65 536 bytes

The kernels' own sizes come from the header's constants; the plane layout and the Rect (six floats) are rect_overlap.hpp's,
which has no header of its own to read, as in the other tests of this kind."""
import os
import shutil

import pytest

from dfu3d_amd import _lib_prop
from tools import isa_mix as tools  # noqa: E402

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
SRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "dfu3d_amd", "csrc", "proposal_stage.hip")
FIELDS = ("vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size", "group_segment_fixed_size")
K = _lib_prop.CONSTANTS
MAX_POST, ROWS, PAIRS, WAVES = (K["DFU3D_PROP_MAX_POST"], K["DFU3D_PROP_BLOCK_ROWS"], K["DFU3D_PROP_QUEUE_PAIRS"],
                                K["DFU3D_PROP_SORT_THREADS"] // 64)
PLANES, RECT = 4 * 8 * 256 * 4, 6 * 4                    # rect_overlap.hpp: [4][MAXV * IB] floats; struct Rect
LDS = {"k_pr_order": 4 * (256 * WAVES + WAVES),
       "k_pr_nms": PLANES + MAX_POST * RECT + ROWS * (RECT + 4) + ROWS * 8 + PAIRS * 2 + 8 + 8}
assert LDS["k_pr_nms"] <= 64 * 1024


@pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which("hipcc")), reason="hipcc not available")
def test_proposal_kernels_no_scratch_no_spills_expected_lds():
    found = {}
    for name, (_, block) in tools.kernels(tools.assembly(SRC)).items():
        d = tools.demangle(name)
        short = d.split("(")[0].split("::")[-1].replace("void ", "").strip()
        if short.startswith("k_pr_"):
            found[short] = block
    assert set(found) == set(LDS), sorted(found)
    for k, block in found.items():
        res = {f: tools.field(block, f) for f in FIELDS}
        assert res["vgpr_spill_count"] == 0 and res["private_segment_fixed_size"] == 0, (k, res)
        assert res["sgpr_spill_count"] == 0 and res["group_segment_fixed_size"] == LDS[k], (k, res)
