"""CPU-only guard on the point-sampling kernels (pointsample_stage.hip): the gfx950 code object hipcc makes with the
product's flags holds exactly the expected k_smp_* kernels, uses no scratch memory, spills no registers and uses the LDS
each is designed around, W = DFU3D_SMP_SCENE_THREADS / 64 waves:

  k_smp_order   the sort of block_sort.hpp: 256 digits x W waves of counts and the W wave totals of the scan
                                                                                            4 * (256 * 16 + 16) = 16 448 bytes
  k_smp_list    the W 64-bit wave sums of the counts before the scene, block_select's 256-bucket histogram and its three
                64-bit hand-off words, the W wave totals of the scans, one flag word; rounded up to the 8 bytes the 64-bit
                words are aligned to                                          8 * 16 + 4 * 256 + 8 * 3 + 4 * 16 + 4 -> 1 248 bytes
  k_smp_gather  none
"""
import os
import shutil

import pytest

from dfu3d_amd import _lib_smp
from tools import isa_mix as tools  # noqa: E402

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
SRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "dfu3d_amd", "csrc", "pointsample_stage.hip")
FIELDS = ("vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size", "group_segment_fixed_size")
K = _lib_smp.CONSTANTS
WAVES = K["DFU3D_SMP_SCENE_THREADS"] // 64
LDS = {"k_smp_order": 4 * (256 * WAVES + WAVES),
       "k_smp_list": -(-(8 * WAVES + 4 * 256 + 8 * 3 + 4 * WAVES + 4) // 8) * 8,
       "k_smp_gather": 0}
assert K["DFU3D_SMP_SCENE_THREADS"] % 64 == 0 and K["DFU3D_SMP_GATHER_THREADS"] % 64 == 0 and len(LDS) == K["DFU3D_SMP_LAUNCHES"]


@pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which("hipcc")), reason="hipcc not available")
def test_sample_points_kernels_no_scratch_no_spills_expected_lds():
    found = {}
    for name, (_, block) in tools.kernels(tools.assembly(SRC)).items():
        d = tools.demangle(name)
        short = d.split("(")[0].split("::")[-1].replace("void ", "").strip()
        if short.startswith("k_smp_"):
            found[short] = block
    assert set(found) == set(LDS), sorted(found)
    for k, block in found.items():
        res = {f: tools.field(block, f) for f in FIELDS}
        assert res["vgpr_spill_count"] == 0 and res["private_segment_fixed_size"] == 0, (k, res)
        assert res["sgpr_spill_count"] == 0 and res["group_segment_fixed_size"] == LDS[k], (k, res)
