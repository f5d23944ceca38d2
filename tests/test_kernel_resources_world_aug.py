"""CPU-only guard on the world-augmentation kernels (worldaug_stage.hip): the gfx950 code object hipcc makes with the
product's flags uses no scratch memory and spills no registers, and the LDS of every kernel fits a 64 KiB workgroup."""
import os
import shutil

import pytest

from tools import isa_mix as tools  # noqa: E402

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
SRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "dfu3d_amd", "csrc", "worldaug_stage.hip")
FIELDS = ("vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size", "group_segment_fixed_size")
KERNELS = ["k_wa_boxes", "k_wa_boxes", "k_wa_count", "k_wa_scan", "k_wa_write"]      # k_wa_boxes: float32 and float64


@pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which("hipcc")), reason="hipcc not available")
def test_world_aug_kernels_no_scratch_no_spills():
    found = {}
    for name, (_, block) in tools.kernels(tools.assembly(SRC)).items():
        d = tools.demangle(name)
        short = d.split("(")[0].split("::")[-1].replace("void ", "").strip()
        if short.startswith("k_wa_"):
            found[short] = block
    assert sorted(k.split("<")[0] for k in found) == KERNELS, sorted(found)
    for k, block in found.items():
        res = {f: tools.field(block, f) for f in FIELDS}
        assert res["vgpr_spill_count"] == 0 and res["private_segment_fixed_size"] == 0, (k, res)
        assert res["sgpr_spill_count"] == 0, (k, res)
        assert 0 < res["group_segment_fixed_size"] <= 65536, (k, res)
