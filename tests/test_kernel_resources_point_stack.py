"""CPU-only guard on the stacked set-abstraction kernels (pointstack_stage.hip): the gfx950 code object hipcc makes with
the product's flags holds exactly the expected k_stk_* kernels, uses no scratch memory and spills no registers, and the
LDS of every kernel fits a 64 KiB workgroup (the sampling kernels keep their points in registers; LDS carries one
exchange slot per wave and parity)."""
import os
import re
import shutil

import pytest

from tools import isa_mix as tools  # noqa: E402

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
SRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "dfu3d_amd", "csrc", "pointstack_stage.hip")
FIELDS = ("vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size", "group_segment_fixed_size")
WITH_LDS = {"k_stk_fps<256, 1>", "k_stk_fps<256, 4>", "k_stk_fps<1024, 2>", "k_stk_fps<1024, 4>", "k_stk_fps<1024, 8>",
            "k_stk_fps<1024, 16>", "k_stk_fps_big", "k_stk_starts"}
NO_LDS = {"k_stk_count", "k_stk_ball", "k_stk_group", "k_stk_gidx", "k_stk_bev"}


@pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which("hipcc")), reason="hipcc not available")
def test_point_stack_kernels_no_scratch_no_spills():
    found = {}
    for name, (_, block) in tools.kernels(tools.assembly(SRC)).items():
        d = tools.demangle(name)
        short = d.split("(")[0].split("::")[-1].replace("void ", "").strip()
        if "<" in short:                               # the integer template arguments, however the demangler spells them
            short = "%s<%s>" % (short.split("<")[0], ", ".join(re.findall(r"\d+", short.split("<", 1)[1])))
        if short.startswith("k_stk_"):
            found[short] = block
        assert not short.startswith("k_pn_"), short    # the batched kernels stay in pointnet2_stage.hip
    assert set(found) == WITH_LDS | NO_LDS, sorted(found)
    for k, block in found.items():
        res = {f: tools.field(block, f) for f in FIELDS}
        assert res["vgpr_spill_count"] == 0 and res["private_segment_fixed_size"] == 0, (k, res)
        assert res["sgpr_spill_count"] == 0, (k, res)
        if k in WITH_LDS:
            assert 0 < res["group_segment_fixed_size"] <= 65536, (k, res)
        else:
            assert res["group_segment_fixed_size"] == 0, (k, res)
