"""CPU-only guard on the CenterHead kernels (centerhead_stage.hip): the gfx950 code object hipcc makes with the product's
flags uses no scratch memory and spills no registers, and the LDS of every kernel fits a 64 KiB workgroup."""
import os
import shutil

import pytest

from tools import isa_mix as tools  # noqa: E402

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
SRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "dfu3d_amd", "csrc", "centerhead_stage.hip")


@pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which("hipcc")), reason="hipcc not available")
def test_center_head_kernels_no_scratch_no_spills():
    found = {tools.demangle(name).split("(")[0]: block for name, (_, block) in tools.kernels(tools.assembly(SRC)).items()}
    for k in ("k_ca_slots", "k_ca_draw", "k_cd_decode"):
        block = found[k]
        res = {f: tools.field(block, f) for f in ("vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size",
                                                   "group_segment_fixed_size")}
        assert res["vgpr_spill_count"] == 0 and res["private_segment_fixed_size"] == 0, (k, res)
        assert res["sgpr_spill_count"] == 0, (k, res)
        assert 0 < res["group_segment_fixed_size"] <= 65536, (k, res)
    res = {f: tools.field(found["k_ca_transc"], f) for f in ("vgpr_spill_count", "sgpr_spill_count",
                                                              "private_segment_fixed_size", "group_segment_fixed_size")}
    assert not any(res.values()), res                                        # no scratch, no spills, and it uses no LDS
