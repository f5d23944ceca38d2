"""CPU-only guard on the RoI-point pooling kernels (roipoint_stage.hip): the gfx950 code object hipcc makes with the
product's flags holds exactly the expected k_rp_* kernels, uses no scratch memory, spills no registers and uses no LDS
(the search keeps its count in registers and its hits in pooled_idx; the gather moves rows through registers)."""
import os
import re
import shutil

import pytest

from tools import isa_mix as tools  # noqa: E402

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
SRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "dfu3d_amd", "csrc", "roipoint_stage.hip")
FIELDS = ("vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size", "group_segment_fixed_size")
KERNELS = {"k_rp_search", "k_rp_gather<0>", "k_rp_gather<1>"}


@pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which("hipcc")), reason="hipcc not available")
def test_roipoint_kernels_no_scratch_no_spills_no_lds():
    found = {}
    for name, (_, block) in tools.kernels(tools.assembly(SRC)).items():
        d = tools.demangle(name)
        short = d.split("(")[0].split("::")[-1].replace("void ", "").strip()
        if "<" in short:                               # the integer template arguments, however the demangler spells them
            short = "%s<%s>" % (short.split("<")[0], ", ".join(re.findall(r"\d+", short.split("<", 1)[1])))
        if short.startswith("k_rp_"):
            found[short] = block
    assert set(found) == KERNELS, sorted(found)
    for k, block in found.items():
        res = {f: tools.field(block, f) for f in FIELDS}
        assert res["vgpr_spill_count"] == 0 and res["private_segment_fixed_size"] == 0, (k, res)
        assert res["sgpr_spill_count"] == 0 and res["group_segment_fixed_size"] == 0, (k, res)
