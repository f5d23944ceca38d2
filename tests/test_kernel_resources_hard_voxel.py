"""CPU-only guard on the hard-voxel kernels (hardvoxel_stage.hip): the gfx950 code object hipcc makes with the product's
flags holds exactly the expected k_hvox_* kernels, one per launch of a call, uses no scratch memory, spills no
registers and uses the LDS each is designed around, N = DFU3D_HVOX_ROW_THREADS threads, W = N / 64 waves:

  k_hvox_init     workgroup 0 sums the scenes' counts: one 64-bit partial sum per thread and one flag word, rounded up to
                  the 8 bytes the 64-bit words are aligned to                                   8 * 1024 + 4 -> 8 200 bytes
  k_hvox_insert   none: the table is in global memory
  k_hvox_count    the W wave sums of the workgroup sum                                                   4 * 16 = 64 bytes
  k_hvox_offsets  the W wave totals of the workgroup scans                                               4 * 16 = 64 bytes
  k_hvox_assign   the W wave totals of the workgroup scan                                                4 * 16 = 64 bytes
  k_hvox_place    none: the thinning of a wave's rows is done by ballot
  k_hvox_emit     none
"""
import os
import shutil

import pytest

from dfu3d_amd import _lib_hvox
from tools import isa_mix as tools  # noqa: E402

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
SRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "dfu3d_amd", "csrc", "hardvoxel_stage.hip")
FIELDS = ("vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size", "group_segment_fixed_size")
K = _lib_hvox.CONSTANTS
THREADS = K["DFU3D_HVOX_ROW_THREADS"]
WAVES = THREADS // 64
LDS = {"k_hvox_init": -(-(8 * THREADS + 4) // 8) * 8,
       "k_hvox_insert": 0,
       "k_hvox_count": 4 * WAVES,
       "k_hvox_offsets": 4 * WAVES,
       "k_hvox_assign": 4 * WAVES,
       "k_hvox_place": 0,
       "k_hvox_emit": 0}
assert THREADS % 64 == 0 and K["DFU3D_HVOX_OUT_THREADS"] % 64 == 0 and len(LDS) == K["DFU3D_HVOX_LAUNCHES"]


@pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which("hipcc")), reason="hipcc not available")
def test_hard_voxel_kernels_no_scratch_no_spills_expected_lds():
    found = {}
    for name, (_, block) in tools.kernels(tools.assembly(SRC)).items():
        d = tools.demangle(name)
        short = d.split("(")[0].split("::")[-1].replace("void ", "").strip()
        if short.startswith("k_hvox_"):
            found[short] = block
    assert set(found) == set(LDS), sorted(found)
    for k, block in found.items():
        res = {f: tools.field(block, f) for f in FIELDS}
        assert res["vgpr_spill_count"] == 0 and res["private_segment_fixed_size"] == 0, (k, res)
        assert res["sgpr_spill_count"] == 0 and res["group_segment_fixed_size"] == LDS[k], (k, res)
