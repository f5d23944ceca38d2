"""CPU-only guard on the sparse-convolution kernels (sparseconv_stage.hip): the gfx950 code object hipcc makes with the
product's flags holds exactly the expected k_spc_* kernels, uses no scratch memory, spills no registers and uses the LDS
each is designed around.  N = DFU3D_SPC_ROW_THREADS threads, W = N / 64 waves, TK = DFU3D_SPC_TILE_K, KV = DFU3D_SPC_MAX_KV.

  k_spc_fill, k_spc_insert, k_spc_cand, k_spc_tables   none: the tables are in global memory
  k_spc_count, k_spc_offsets, k_spc_assign             the W wave sums / totals of the workgroup sum and scans: 4 * 16 = 64
  k_spc_gemm<WN, TR>   a tile of TM = 128 / WN rows by TN = 32 * WN channels: the tile's part of the table (TM * KV ints),
                       the gathered rows (TM x (TK + 1) floats: the pad column keeps a column read off one bank), the
                       weight slice ((TK + 1) x TN floats forward, TK x (TN + 1) transposed) and the mask of present offsets
                       WN = 1: 13 824 + 16 896 + 4 224 + 4 = 34 948;  WN = 2: 6 912 + 8 448 + 8 448 (8 320) + 4
  k_spc_wgrad, k_spc_wsum                              none: both operands come straight from global memory

Registers as built (recorded, not asserted beyond the spill counts): k_spc_gemm 48 .. 52 VGPRs with the 16 accumulators
among them, k_spc_wgrad 28, the index kernels 8 .. 43: registers never limit the occupancy (the product kernel's LDS
allows four workgroups of four waves per compute unit with WN = 1, six with WN = 2)."""
import os
import shutil

import pytest

from dfu3d_amd import _lib_spc
from tools import isa_mix as tools  # noqa: E402

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
SRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "dfu3d_amd", "csrc", "sparseconv_stage.hip")
FIELDS = ("vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size", "group_segment_fixed_size", "vgpr_count")
K = _lib_spc.CONSTANTS
WAVES = K["DFU3D_SPC_ROW_THREADS"] // 64
TK, KV = K["DFU3D_SPC_TILE_K"], K["DFU3D_SPC_MAX_KV"]


def gemm_lds(wn, transposed):
    tm, tn = 32 * (4 // wn), 32 * wn
    return 4 * (tm * KV + tm * (TK + 1) + (TK * (tn + 1) if transposed else tn * (TK + 1)) + 1)


LDS = {"k_spc_fill": 0, "k_spc_insert": 0, "k_spc_cand": 0, "k_spc_count": 4 * WAVES, "k_spc_offsets": 4 * WAVES,
       "k_spc_assign": 4 * WAVES, "k_spc_tables": 0, "k_spc_wgrad": 0, "k_spc_wsum": 0,
       # (the template arguments as the tool's demangler leaves them: <int WN, bool TR>)
       "k_spc_gemm<Li1ELb0>": gemm_lds(1, False), "k_spc_gemm<Li2ELb0>": gemm_lds(2, False),
       "k_spc_gemm<Li1ELb1>": gemm_lds(1, True), "k_spc_gemm<Li2ELb1>": gemm_lds(2, True)}
assert K["DFU3D_SPC_GEMM_THREADS"] == 256 and K["DFU3D_SPC_WGRAD_THREADS"] == 64 and gemm_lds(1, False) == 34948


@pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which("hipcc")), reason="hipcc not available")
def test_sparse_conv_kernels_no_scratch_no_spills_expected_lds():
    found = {}
    for name, (_, block) in tools.kernels(tools.assembly(SRC)).items():
        d = tools.demangle(name)
        short = d.split("(")[0].split("::")[-1].replace("void ", "").strip()
        if short.startswith("k_spc_"):
            found[short] = block
    assert set(found) == set(LDS), sorted(found)
    for k, block in found.items():
        res = {f: tools.field(block, f) for f in FIELDS}
        print(k, res)
        assert res["vgpr_spill_count"] == 0 and res["private_segment_fixed_size"] == 0, (k, res)
        assert res["sgpr_spill_count"] == 0 and res["group_segment_fixed_size"] == LDS[k], (k, res)
        assert res["vgpr_count"] <= 64, (k, res)                  # eight waves per SIMD as far as registers go
