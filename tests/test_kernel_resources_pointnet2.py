"""CPU-only guard on the PointNet++ kernels (pointnet2_stage.hip): the gfx950 code object hipcc makes with the product's
flags holds exactly the expected k_pn_* kernels, uses no scratch memory and spills no registers, and the LDS of every
kernel fits a 64 KiB workgroup (the sampling kernels keep their points in registers; LDS carries one exchange slot per
wave and parity)."""
import os
import re
import shutil

import pytest

from tools import isa_mix as tools  # noqa: E402

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
SRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "dfu3d_amd", "csrc", "pointnet2_stage.hip")
FIELDS = ("vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size", "group_segment_fixed_size")
WITH_LDS = {"k_pn_fps<256, 1>", "k_pn_fps<256, 4>", "k_pn_fps<1024, 2>", "k_pn_fps<1024, 4>", "k_pn_fps<1024, 8>",
            "k_pn_fps<1024, 16>", "k_pn_fps_big", "k_pn_three_nn", "k_pn_offsets"}
NO_LDS = {"k_pn_ball", "k_pn_group", "k_pn_interp", "k_pn_count", "k_pn_place", "k_pn_order", "k_pn_gather_bwd",
          "k_pn_check_batch"}


@pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which("hipcc")), reason="hipcc not available")
def test_pointnet2_kernels_no_scratch_no_spills():
    found = {}
    for name, (_, block) in tools.kernels(tools.assembly(SRC)).items():
        d = tools.demangle(name)
        short = d.split("(")[0].split("::")[-1].replace("void ", "").strip()
        if "<" in short:                               # the integer template arguments, however the demangler spells them
            short = "%s<%s>" % (short.split("<")[0], ", ".join(re.findall(r"\d+", short.split("<", 1)[1])))
        if short.startswith("k_pn_"):
            found[short] = block
    assert set(found) == WITH_LDS | NO_LDS, sorted(found)
    for k, block in found.items():
        res = {f: tools.field(block, f) for f in FIELDS}
        assert res["vgpr_spill_count"] == 0 and res["private_segment_fixed_size"] == 0, (k, res)
        assert res["sgpr_spill_count"] == 0, (k, res)
        if k in WITH_LDS:
            assert 0 < res["group_segment_fixed_size"] <= 65536, (k, res)
        else:
            assert res["group_segment_fixed_size"] == 0, (k, res)
