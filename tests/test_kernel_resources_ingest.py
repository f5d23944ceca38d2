"""CPU-only guard on the FOV-ingest kernels (ingest_stage.hip): the gfx950 code object hipcc makes with the product's
flags has exactly the kernels DFU3D_ING_LAUNCHES counts, uses no scratch memory, spills no registers, and needs no LDS
beyond the wave totals of the workgroup scan and sums."""
import os
import shutil

import pytest

from tools import isa_mix as tools  # noqa: E402

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
SRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "dfu3d_amd", "csrc", "ingest_stage.hip")
FIELDS = ("vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size", "group_segment_fixed_size")
KERNELS = ["k_ing_boxes", "k_ing_flag", "k_ing_scan", "k_ing_write"]


@pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which("hipcc")), reason="hipcc not available")
def test_ingest_kernels_no_scratch_no_spills():
    from dfu3d_amd import _lib_ingest
    C = _lib_ingest.CONSTANTS
    waves = C["DFU3D_ING_CHUNK"] // 64
    lds = {"k_ing_flag": 4 * waves, "k_ing_write": 4 * waves, "k_ing_boxes": 4 * waves,     # one int per wave
           "k_ing_scan": 4 * (1024 // 64)}                                                    # the scan's 16 wave totals
    found = {}
    for name, (_, block) in tools.kernels(tools.assembly(SRC)).items():
        d = tools.demangle(name)
        short = d.split("(")[0].split("::")[-1].replace("void ", "").strip()
        if short.startswith("k_ing_"):
            assert short not in found, short
            found[short] = block
    assert sorted(found) == KERNELS, sorted(found)
    assert C["DFU3D_ING_LAUNCHES"] == len(KERNELS)
    for k, block in found.items():
        res = {f: tools.field(block, f) for f in FIELDS}
        assert res["vgpr_spill_count"] == 0 and res["private_segment_fixed_size"] == 0, (k, res)
        assert res["sgpr_spill_count"] == 0, (k, res)
        assert res["group_segment_fixed_size"] == lds[k], (k, res)
