"""CPU-only guard on the pillar-scatter kernels (bevscatter_stage.hip): the gfx950 code object hipcc makes with the
product's flags uses no scratch memory and spills no registers, and the LDS of every kernel fits a 64 KiB workgroup."""
import os
import shutil

import pytest

from tools import isa_mix as tools  # noqa: E402

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
SRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "dfu3d_amd", "csrc", "bevscatter_stage.hip")
FIELDS = ("vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size", "group_segment_fixed_size")
KERNELS = ["k_bs_clear", "k_bs_gather", "k_bs_mark", "k_bs_write"]
WITH_LDS = {"k_bs_gather", "k_bs_write"}             # the transposing tile: 64 x 65 words and the run's owners


@pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which("hipcc")), reason="hipcc not available")
def test_pillar_scatter_kernels_no_scratch_no_spills():
    found = {}
    for name, (_, block) in tools.kernels(tools.assembly(SRC)).items():
        d = tools.demangle(name)
        short = d.split("(")[0].split("::")[-1].replace("void ", "").strip()
        if short.startswith("k_bs_"):
            found[short] = block
    assert sorted(found) == KERNELS, sorted(found)
    for k, block in found.items():
        res = {f: tools.field(block, f) for f in FIELDS}
        assert res["vgpr_spill_count"] == 0 and res["private_segment_fixed_size"] == 0, (k, res)
        assert res["sgpr_spill_count"] == 0, (k, res)
        assert res["group_segment_fixed_size"] <= 65536, (k, res)
        assert (res["group_segment_fixed_size"] >= 64 * 65 * 4 + 64 * 4) == (k in WITH_LDS), (k, res)
