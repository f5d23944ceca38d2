"""CPU-only guard on the optimiser kernels (optim_stage.hip): the gfx950 code object hipcc makes with the product's flags
has exactly the three kernels of the stage, uses no scratch memory, spills no registers, and needs no LDS beyond the wave
sums of the workgroup reduction."""
import os
import shutil

import pytest

from tools import isa_mix as tools  # noqa: E402

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
SRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "dfu3d_amd", "csrc", "optim_stage.hip")
FIELDS = ("vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size", "group_segment_fixed_size")
KERNELS = ["k_opt_step", "k_opt_sumsq", "k_opt_total"]
LDS = {"k_opt_sumsq": 4 * 8}                         # one double per wave


@pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which("hipcc")), reason="hipcc not available")
def test_optimizer_kernels_no_scratch_no_spills():
    found = {}
    for name, (_, block) in tools.kernels(tools.assembly(SRC)).items():
        d = tools.demangle(name)
        short = d.split("(")[0].split("::")[-1].replace("void ", "").strip()
        if short.startswith("k_opt_"):
            found[short] = block
    assert sorted(found) == KERNELS, sorted(found)
    from dfu3d_amd import _lib_opt
    assert _lib_opt.CONSTANTS["DFU3D_OPT_LAUNCHES"] == len(KERNELS)
    for k, block in found.items():
        res = {f: tools.field(block, f) for f in FIELDS}
        assert res["vgpr_spill_count"] == 0 and res["private_segment_fixed_size"] == 0, (k, res)
        assert res["sgpr_spill_count"] == 0, (k, res)
        assert res["group_segment_fixed_size"] == LDS.get(k, 0), (k, res)
