"""CPU-only guard on the anchor target kernels (anchor_stage.hip): the gfx950 code object hipcc makes with the product's
flags holds exactly the expected k_anc_* kernels, one per launch of a call, uses no scratch memory, spills no registers
and uses the LDS each is designed around, M = DFU3D_ANC_MAX_BOXES, S = DFU3D_ANC_MAX_SETS, T = DFU3D_ANC_THREADS:

  k_anc_prep   the last live row of the sample and the M / 64 wave counts of the workgroup rank          4 + 4 * M / 64
  k_anc_top    the S + 1 list offsets, a rectangle (16 bytes) and the top IoU's bits per box        4 (S + 1) + 20 M
  k_anc_emit   the same with the box's class on top, and the 7 T target words of the workgroup on their way to whole
               lines                                                                        4 (S + 1) + 24 M + 28 T

The two streaming kernels must also stay within 64 vector registers, so that eight waves fit a SIMD.
"""
import os
import shutil

import pytest

from dfu3d_amd import _lib_anc
from tools import isa_mix as tools  # noqa: E402

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
SRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "dfu3d_amd", "csrc", "anchor_stage.hip")
FIELDS = ("vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size", "group_segment_fixed_size", "vgpr_count")
K = _lib_anc.CONSTANTS
M, S, T = K["DFU3D_ANC_MAX_BOXES"], K["DFU3D_ANC_MAX_SETS"], K["DFU3D_ANC_THREADS"]
LDS = {"k_anc_prep": 4 + 4 * (M // 64),
       "k_anc_top": 4 * (S + 1) + 20 * M,
       "k_anc_emit": 4 * (S + 1) + 24 * M + 28 * T}
STREAMING = ("k_anc_top", "k_anc_emit")
assert M % 64 == 0 and T % 64 == 0 and len(LDS) == K["DFU3D_ANC_LAUNCHES"] and max(LDS.values()) <= 32 * 1024


@pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which("hipcc")), reason="hipcc not available")
def test_anchor_target_kernels_no_scratch_no_spills_expected_lds():
    found = {}
    for name, (_, block) in tools.kernels(tools.assembly(SRC)).items():
        d = tools.demangle(name)
        short = d.split("(")[0].split("::")[-1].replace("void ", "").strip()
        if short.startswith("k_anc_"):
            found[short] = block
    assert set(found) == set(LDS), sorted(found)
    for k, block in found.items():
        res = {f: tools.field(block, f) for f in FIELDS}
        assert res["vgpr_spill_count"] == 0 and res["private_segment_fixed_size"] == 0, (k, res)
        assert res["sgpr_spill_count"] == 0 and res["group_segment_fixed_size"] == LDS[k], (k, res)
        if k in STREAMING:
            assert res["vgpr_count"] <= 64, (k, res)
