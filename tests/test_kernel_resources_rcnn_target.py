"""CPU-only guard on PointRCNN's target-assignment kernels (rcnntarget_stage.hip): the gfx950 code object hipcc makes
with the product's flags holds exactly the expected k_tg_* kernels, uses no scratch memory, spills no registers and uses
the LDS each is designed around:

  k_tg_point_targets   one tile of 64 boxes: 5 floats and 6 doubles each                       64 * (20 + 48) =  4 352 bytes
  k_tg_roi_max_iou     the polygon planes of rect_overlap.hpp, 4 planes x 8 vertices x 256 threads x 4 bytes = 32 768 bytes
  k_tg_roi_sample      three index lists and the keys of DFU3D_TGT_MAX_ROIS ints, four wave totals  4 * 8 192 + 16 = 32 784"""
import os
import shutil

import pytest

from dfu3d_amd import _lib_tgt
from tools import isa_mix as tools  # noqa: E402

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
SRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "dfu3d_amd", "csrc", "rcnntarget_stage.hip")
FIELDS = ("vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size", "group_segment_fixed_size")
LDS = {"k_tg_point_targets": 64 * (5 * 4 + 6 * 8), "k_tg_roi_max_iou": 4 * 8 * 256 * 4,
       "k_tg_roi_sample": 4 * 4 * _lib_tgt.CONSTANTS["DFU3D_TGT_MAX_ROIS"] + 4 * 4}


@pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which("hipcc")), reason="hipcc not available")
def test_rcnn_target_kernels_no_scratch_no_spills_expected_lds():
    found = {}
    for name, (_, block) in tools.kernels(tools.assembly(SRC)).items():
        d = tools.demangle(name)
        short = d.split("(")[0].split("::")[-1].replace("void ", "").strip()
        if short.startswith("k_tg_"):
            found[short] = block
    assert set(found) == set(LDS), sorted(found)
    for k, block in found.items():
        res = {f: tools.field(block, f) for f in FIELDS}
        assert res["vgpr_spill_count"] == 0 and res["private_segment_fixed_size"] == 0, (k, res)
        assert res["sgpr_spill_count"] == 0 and res["group_segment_fixed_size"] == LDS[k], (k, res)
