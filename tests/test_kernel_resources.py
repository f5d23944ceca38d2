"""CPU-only guard on the register budget of the binning pass (k_bp_bin): the gfx950 code object hipcc makes with the
product's flags must not use scratch memory or VGPR spills, must keep its SGPR spills at the two dwords left after
the uniform-state diet (47 before it), and must leave room for seven waves per SIMD."""
import os
import shutil

import pytest

from tools import isa_mix as tools  # noqa: E402

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
SRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "dfu3d_amd", "csrc", "pixel_stage.hip")


@pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which("hipcc")), reason="hipcc not available")
def test_k_bp_bin_register_budget():
    found = {tools.demangle(name).split("(")[0]: block for name, (_, block) in tools.kernels(tools.assembly(SRC)).items()}
    block = found["k_bp_bin"]
    res = {k: tools.field(block, k) for k in ("sgpr_spill_count", "vgpr_spill_count", "private_segment_fixed_size",
                                               "vgpr_count", "sgpr_count")}
    assert res["vgpr_spill_count"] == 0, res
    assert res["private_segment_fixed_size"] == 0, res
    assert 0 <= res["sgpr_spill_count"] <= 2, res
    assert 0 < res["vgpr_count"] <= 72, res            # 72 allocated VGPRs: seven waves per SIMD
    assert 0 < res["sgpr_count"] <= 96, res            # 82-96 SGPRs: seven 256-thread workgroups per CU
