"""CPU-only: the C-ABI library builds/loads and exports exactly what
include/dfu3d.h declares (no compute calls without a GPU)."""
import ctypes

import numpy as np
import pytest

from dfu3d_amd import _header, _lib

STAGE = {k[len("DFU3D_STAGE_"):]: v for k, v in _lib.CONSTANTS.items() if k.startswith("DFU3D_STAGE_")}


def test_library_exports_every_header_symbol():
    L = _lib.lib()
    declared = _lib.header_symbols()
    assert len(declared) >= 15
    for name in declared:
        assert hasattr(L, name), "libdfu3d_hip.so does not export %s" % name
        assert name in _lib.SIGNATURES, "no ctypes signature for %s" % name
    assert set(_lib.SIGNATURES) == set(declared)


def test_version_and_strerror():
    L = _lib.lib()
    assert L.dfu3d_version() == 150 == _lib.header_version()
    assert L.dfu3d_strerror(0) == b"ok"
    assert b"invalid" in L.dfu3d_strerror(-1)


def test_argument_validation_without_gpu():
    """Null pointers / bad sizes are rejected on the host before any launch."""
    L = _lib.lib()
    assert L.dfu3d_fov_filter(None, None, None, None, 1, 900, 1600, 10, None, None, None) == -1
    assert L.dfu3d_range_cluster(None, None, None, None, 0, 3.0, 0.001, None, None, None, None, 8, None) == -1


def test_bin_table_geometry_covers_reachable_bins():
    from dfu3d_amd.params import Params
    p = Params()
    g = _lib.BinGeom()
    g.vsize_r, g.vsize_t, g.vsize_p = p.vsize
    g.rmin_r, g.rmin_t, g.rmin_p = p.vrange_min
    g.grid_r, g.grid_t, g.grid_p = p.vgrid
    g.max_points_per_voxel, g.max_voxels = 100, 1000000
    g.theta_min, g.z_max, g.depth_min = p.theta_min, p.z_max, p.depth_min
    n = _lib.lib().dfu3d_bin_table_geometry(ctypes.byref(g))
    assert n == g.t_n * g.p_n and 1_000_000 < n < 1_500_000
    th = np.array([np.nextafter(1.5, 2), np.pi])
    ph = np.array([-np.pi / 2, np.pi / 2])
    tb = np.floor((th + 5.0) / p.vsize[1])
    pb = np.floor((ph + 5.0) / p.vsize[2])
    assert g.t_lo <= tb.min() and tb.max() < g.t_lo + g.t_n
    assert g.p_lo <= pb.min() and pb.max() < g.p_lo + g.p_n


def test_struct_layouts_match_the_header(tmp_path):
    """sizeof / offsetof of dfu3d_bin_geom and dfu3d_chain_cfg as a C compiler sees include/dfu3d.h == the ctypes
    mirrors in dfu3d_amd/_lib.py (a silent drift would corrupt every dfu3d_pseudo_boxes call)."""
    import ctypes
    import os
    import subprocess
    from dfu3d_amd import _build, _lib
    fields_geom = [f[0] for f in _lib.BinGeom._fields_]
    fields_cfg = [f[0] for f in _lib.ChainCfg._fields_]
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "dfu3d.h"', 'int main(void) {',
           'printf("%zu\\n", sizeof(dfu3d_bin_geom));', 'printf("%zu\\n", sizeof(dfu3d_chain_cfg));']
    src += ['printf("%%zu\\n", offsetof(dfu3d_bin_geom, %s));' % f for f in fields_geom]
    src += ['printf("%%zu\\n", offsetof(dfu3d_chain_cfg, %s));' % f for f in fields_cfg]
    src += ['return 0; }']
    c = tmp_path / "layout.c"
    c.write_text("\n".join(src))
    exe = str(tmp_path / "layout")
    subprocess.check_call(["gcc", "-I", _build.INCLUDE, str(c), "-o", exe])
    vals = [int(v) for v in subprocess.check_output([exe]).decode().split()]
    assert vals[0] == ctypes.sizeof(_lib.BinGeom) and vals[1] == ctypes.sizeof(_lib.ChainCfg)
    k = 2
    for f in fields_geom:
        assert vals[k] == getattr(_lib.BinGeom, f).offset, f
        k += 1
    for f in fields_cfg:
        assert vals[k] == getattr(_lib.ChainCfg, f).offset, f
        k += 1


def test_sizes_struct_layout_and_workspace_bytes(tmp_path):
    """dfu3d_sizes mirrors the header; dfu3d_workspace_bytes answers for every stage and its PSEUDO_BOXES figure is
    the chain workspace of the same configuration."""
    import subprocess
    from dfu3d_amd import _build
    fields = [f[0] for f in _lib.Sizes._fields_]
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "dfu3d.h"', 'int main(void) {',
           'printf("%zu\\n", sizeof(dfu3d_sizes));']
    src += ['printf("%%zu\\n", offsetof(dfu3d_sizes, %s));' % f for f in fields] + ['return 0; }']
    c = tmp_path / "sz.c"
    c.write_text("\n".join(src))
    exe = str(tmp_path / "sz")
    subprocess.check_call(["gcc", "-I", _build.INCLUDE, str(c), "-o", exe])
    vals = [int(v) for v in subprocess.check_output([exe]).decode().split()]
    assert vals[0] == ctypes.sizeof(_lib.Sizes)
    for k, f in enumerate(fields):
        assert vals[1 + k] == getattr(_lib.Sizes, f).offset, f
    L = _lib.lib()
    z = _lib.Sizes()
    z.V, z.H, z.W, z.max_inst, z.cap_n, z.cap_vox, z.cap_rows, z.max_points_per_voxel = 96, 900, 1600, 8, 34720, 1 << 18, 6144, 100
    z.pool_cap, z.table_entries, z.dense, z.stat_filter = 96 << 17, 824 * 1573, 1, 0
    assert sorted(STAGE.values()) == list(range(12))
    got = [L.dfu3d_workspace_bytes(s, ctypes.byref(z)) for s in range(len(STAGE))]
    assert got[STAGE["FOV_FILTER"]] == 0 and all(g > 0 for i, g in enumerate(got) if i != STAGE["FOV_FILTER"])
    assert all(g % 256 == 0 for g in got)
    assert got[STAGE["RADIUS_FILTER"]] >= 16 * z.pool_cap + z.pool_cap + 4 * z.pool_cap            # shadow (+ boxes) + flags + queue
    assert got[STAGE["VOXEL_DOWN_SAMPLE"]] == L.dfu3d_voxel_down_sample_scratch_bytes(z.pool_cap) == 80 * z.pool_cap
    assert L.dfu3d_workspace_bytes(len(STAGE), ctypes.byref(z)) == -1
    assert L.dfu3d_workspace_bytes(STAGE["RADIUS_FILTER"], None) == -1
    # == dfu3d_chain_workspace_bytes of the same configuration
    c = _lib.ChainCfg()
    c.V, c.H, c.W, c.max_inst, c.cap_n, c.cap_vox, c.cap_rows = 96, 900, 1600, 8, 34720, 1 << 18, 6144
    c.dense, c.pool_cap, c.bounds_h, c.bounds_w, c.n_theta = 1, 96 << 17, 900, 1600, 89
    c.geom.max_points_per_voxel, c.geom.t_n, c.geom.p_n = 100, 824, 1573
    assert got[STAGE["PSEUDO_BOXES"]] == L.dfu3d_chain_workspace_bytes(ctypes.byref(c))
    assert got[STAGE["PSEUDO_BOXES"]] > got[STAGE["BACKPROJECT_BIN"]]      # the chain holds the back-projection scratch and more


def test_signatures_are_read_from_the_header():
    """One signature per declared symbol, and a few of them typed by hand HERE (and nowhere else): what the reader
    makes of include/dfu3d.h is what a person reading the header would write."""
    from ctypes import POINTER, c_char_p, c_float, c_int32, c_int64, c_uint64, c_void_p
    S = _lib.SIGNATURES
    assert len(S) == len(_lib.header_symbols()) == 46
    assert set(S) == set(_lib.header_symbols())
    assert S["dfu3d_lshape_fit_ws_doubles"] == (c_int64, [c_int64, c_int32])
    assert S["dfu3d_nms_bev"][1][2] is c_float
    assert S["dfu3d_nms_bev"] == (c_int32, [c_void_p, c_int32, c_float, c_void_p, c_void_p, c_void_p, c_void_p])
    assert S["dfu3d_plane_ransac"][1][10] is c_uint64                      # seed
    assert S["dfu3d_pseudo_boxes"][1][0] is POINTER(_lib.ChainCfg) and len(S["dfu3d_pseudo_boxes"][1]) == 21
    assert S["dfu3d_pseudo_boxes"][1][1:] == [c_void_p] * 20
    assert S["dfu3d_strerror"] == (c_char_p, [c_int32])
    assert S["dfu3d_version"] == (c_int32, [])
    assert S["dfu3d_workspace_bytes"] == (c_int64, [c_int32, POINTER(_lib.Sizes)])
    assert S["dfu3d_eval_match_scores"][1][17] is POINTER(_lib.EvalCombo)
    assert S["dfu3d_eval_match_stats"][1][17] is POINTER(_lib.EvalCombo)
    assert S["dfu3d_selftest_classify"][1][3] is POINTER(_lib.BinGeom)
    assert ctypes.sizeof(_lib.EvalCombo) == 16
    assert _lib.EvalCombo._fields_ == [("cls", c_int32), ("difficulty", c_int32), ("min_overlap", ctypes.c_double)]
    assert dict(_lib.ChainCfg._fields_)["geom"] is _lib.BinGeom and _lib.ChainCfg._fields_[-1][0] == "geom"


def test_reader_raises_on_what_it_does_not_know():
    """An unknown type is an error that names the prototype -- never a default."""
    ok = "typedef struct dfu3d_t { int32_t a, b; double c; } dfu3d_t;\nint dfu3d_x(const dfu3d_t *t, float *p, void *stream);"
    structs, sigs, _ = _header.parse(ok)
    assert sigs == {"dfu3d_x": (ctypes.c_int32, [ctypes.POINTER(structs["dfu3d_t"]), ctypes.c_void_p, ctypes.c_void_p])}
    for bad in ("int dfu3d_x(size_t n);", "int dfu3d_x(int32_t a, long b);", "int dfu3d_x(foo_t *p);",
                "int dfu3d_x(const dfu3d_nosuch *p);", "int dfu3d_x(const char *s);", "short dfu3d_x(void);",
                "int dfu3d_x(unsigned int n);", "typedef struct dfu3d_t { size_t n; } dfu3d_t;", "int other_name(void);"):
        with pytest.raises(ValueError, match="dfu3d_x|dfu3d_t|other_name"):
            _header.parse(bad)


def test_reader_takes_integer_macros_only_and_evaluates_nothing_else():
    import sys
    text = """#ifndef DFU3D_H
#define DFU3D_H
#define DFU3D_A 7          /* comment 9 */
#define DFU3D_B (-3)
#define DFU3D_C 16u
#define DFU3D_D (128 + 16 * (65536 + 16384))
#define DFU3D_E 2 * 3 - 4 * (1 - 2)
#define DFU3D_FN(x) (2 * (x))
#define DFU3D_FLOAT 1.5
#define DFU3D_OCTAL 010
#define DFU3D_HEX 0x10
#define DFU3D_CAST ((int64_t)4)
#define DFU3D_NAME DFU3D_A
#define DFU3D_DIV (8 / 2)
#define DFU3D_CODE __import__("sys").modules.__setitem__("dfu3d_macro_was_evaluated", 1)
#define OTHER 5
#endif
"""
    assert _header.parse(text)[2] == {"DFU3D_A": 7, "DFU3D_B": -3, "DFU3D_C": 16, "DFU3D_D": 1310848, "DFU3D_E": 10}
    assert "dfu3d_macro_was_evaluated" not in sys.modules
    with pytest.raises(ValueError, match="DFU3D_BROKEN"):
        _header.parse("#define DFU3D_BROKEN (1 + ")
    C = _lib.CONSTANTS
    assert "DFU3D_H" not in C and "DFU3D_SHADOW_BYTES" not in C and "DFU3D_RF_QUEUE_INTS" not in C
    assert C["DFU3D_VERSION"] == 150 and C["DFU3D_EINVAL"] == -1 and C["DFU3D_ST_CENTER_OVERFLOW"] == 128


# Every constant dfu3d_amd/stages.py exported when its values were still typed by hand, with those values: the record that
# deriving them from the header moved none.
STAGES_CONSTANTS = {
    "CALIB_FLOATS": 48, "ROW_DOUBLES": 24, "MAX_INST": 32, "TABLE_ENTRY_BYTES": 28, "MASK_BYTES": 0,
    "BP_BIN": 1, "BP_AMB": 2, "BP_MARK": 4, "BP_VOX": 8, "BP_REPAIR": 16, "BP_ALL": 31,
    "RF_SHADOW": 1, "RF_FLAGS": 2, "RF_RESOLVE": 4, "RF_COMPACT": 8, "RF_ALL": 15,
    "ST_POOL_OVERFLOW": 1, "ST_VOX_OVERFLOW": 2, "ST_ROW_OVERFLOW": 4, "ST_BIN_RANGE": 8, "ST_VOX_PTS_OVERFLOW": 16,
    "ST_VOXEL_RANGE": 32, "ST_BOX_RANGE": 64, "ST_CENTER_OVERFLOW": 128,
    "EVAL_MAX_DET": 2048, "GT_SAMPLE_MAX_BOXES": 512, "CENTER_MAX_K": 1024, "SELFTEST_SCRATCH_BYTES": 1310848,
}


def test_stages_constants_kept_their_values():
    from dfu3d_amd import stages
    for name, value in STAGES_CONSTANTS.items():
        assert getattr(stages, name) == value and type(getattr(stages, name)) is int, name
    assert sorted(stages.STATUS_TEXT) == [1, 2, 4, 8, 16, 32, 128]
    assert stages.status_message(4 | 128) == stages.STATUS_TEXT[4] + "; " + stages.STATUS_TEXT[128]
    assert stages.status_message(0) == stages.status_message(64) == "ok"      # ST_BOX_RANGE has no text: as before
