"""Record what every scratch-size function of the C ABI returns, over a fixed grid, from a BUILT library of a given
commit (CPU only: the size functions are host code).  tests/test_scratch_sizes.py replays the calls against the
library of the working tree and asserts equality, so a refactor of a layout cannot move a size unnoticed.

    python tests/golden/capture_scratch_sizes.py <libdfu3d_hip.so> <libdfu3d_hip_keybits14.so> <commit> > tests/golden/scratch_sizes.json

The expected values must come from the commit whose sizes are to be kept (a checkout of it, built with
dfu3d_amd/_build.py), never from the code under test.
"""
import ctypes
import itertools
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

BENCH_E = 824 * 1573                 # table entries per view of the product's geometry (tests/test_abi.py)
POOLS = [1, 511, 512, 513, 2047, 2048, 2049, 131071, 131072, 131073, 5 << 17, 96 << 17, 0, -1]
SIZES_FIELDS = ["V", "H", "W", "max_inst", "cap_n", "cap_vox", "cap_rows", "max_points_per_voxel", "pool_cap",
                "table_entries", "dense", "stat_filter"]


def bp_grid():
    """(V, H, W, cap_vox, max_points, table_entries)"""
    g = []
    for V in (1, 3, 12, 96):
        for H, W in ((900, 1600), (180, 320), (225, 400), (16, 4), (370, 1224), (901, 1601)):   # 400, 1224, 1601: no multiple of the 64-pixel tile
            for cap_vox, mp in ((1 << 18, 100), (1 << 17, 100), (1 << 16, 1), (7, 3)):
                for E in (BENCH_E, 1, 63, 64, 65, 257):
                    g.append((V, H, W, cap_vox, mp, E))
    g += [(0, 900, 1600, 1 << 18, 100, BENCH_E), (96, 0, 1600, 1 << 18, 100, BENCH_E), (96, 900, -1, 1 << 18, 100, BENCH_E),
          (96, 900, 1600, 0, 100, BENCH_E), (96, 900, 1600, 1 << 18, 0, BENCH_E), (96, 900, 1600, 1 << 18, 100, 0),
          (-1, -1, -1, -1, -1, -1)]
    return g


def sizes_grid():
    """dfu3d_sizes records: the bench configuration, the small shapes of the chain tests, V = 1, odd widths, invalid ones"""
    g = []
    shapes = [(96, 900, 1600, 8, 34720, 1 << 18, 6144, 100, BENCH_E), (12, 180, 320, 5, 4096, 1 << 17, 6144, 100, BENCH_E),
              (1, 225, 400, 6, 1000, 1 << 16, 64, 100, 4099), (3, 370, 1224, 32, 20000, 1 << 16, 512, 7, 65)]
    for (V, H, W, M, cap_n, cap_vox, cap_rows, mp, E), dense, stat in itertools.product(shapes, (0, 1), (0, 1)):
        for P in (V << 17, 1, 511, 512, 513):
            g.append([V, H, W, M, cap_n, cap_vox, cap_rows, mp, P, E, dense, stat])
    ok = [96, 900, 1600, 8, 34720, 1 << 18, 6144, 100, 96 << 17, BENCH_E, 1, 0]
    for k, bad in ((0, 0), (0, -3), (1, 0), (2, 0), (3, 0), (3, 33), (4, 0), (5, 0), (6, 0), (7, 0), (8, 0), (8, -1),
                   (9, 0), (9, 1 << 31), (9, -5)):
        for dense in (0, 1):
            r = list(ok)
            r[10] = dense
            r[k] = bad
            g.append(r)
    return g


def capture(lib_path, kb14_path, commit):
    from dfu3d_amd import _lib
    libs = {"product": _lib.bind(ctypes.CDLL(lib_path)), "keybits14": _lib.bind(ctypes.CDLL(kb14_path))}
    L = libs["product"]
    out = {"commit": commit}
    for name, lib in libs.items():
        rows = []
        for a in bp_grid():
            pw, bw = ctypes.c_int64(-7), ctypes.c_int64(-7)
            rc = lib.dfu3d_backproject_scratch_words(*a, ctypes.byref(pw), ctypes.byref(bw))
            rows.append([list(a), [rc, pw.value, bw.value]])
        out["backproject_scratch_words/" + name] = rows
    caps = (1, 255, 256, 257, 4096, 34720, 1 << 16, 1 << 18, 0, -1)
    out["segments_scratch_words"] = [[[V, a, b], L.dfu3d_segments_scratch_words(V, a, b)]
                                     for V in (1, 12, 96, 0) for a in caps for b in caps]
    out["rf_shadow_bytes"] = [[[P], L.dfu3d_rf_shadow_bytes(P)] for P in POOLS]
    out["rf_queue_ints"] = [[[P], L.dfu3d_rf_queue_ints(P)] for P in POOLS]
    out["voxel_down_sample_scratch_bytes"] = [[[P], L.dfu3d_voxel_down_sample_scratch_bytes(P)] for P in POOLS]
    out["lshape_fit_ws_doubles"] = [[[P, r], L.dfu3d_lshape_fit_ws_doubles(P, r)] for P in POOLS for r in (1, 64, 6144, 0, -1)]
    ws, chain = [], []
    for r in sizes_grid():
        z = _lib.Sizes(*r)
        ws.append([r, [L.dfu3d_workspace_bytes(s, ctypes.byref(z)) for s in range(-1, 13)]])
        c = _lib.ChainCfg()
        c.V, c.H, c.W, c.max_inst, c.cap_n, c.cap_vox, c.cap_rows = r[:7]
        c.geom.max_points_per_voxel, c.pool_cap, c.dense, c.stat_filter = r[7], r[8], r[10], r[11]
        c.bounds_h, c.bounds_w, c.n_theta, c.stat_voxel, c.stat_nb_neighbors = r[1], r[2], 89, 0.1, 20
        if 0 < r[9] < (1 << 31):
            c.geom.t_n, c.geom.p_n = (824, 1573) if r[9] == BENCH_E else (1, r[9])
        chain.append([r, L.dfu3d_chain_workspace_bytes(ctypes.byref(c))])
    out["workspace_bytes[stage -1..12]"] = ws
    out["chain_workspace_bytes"] = chain
    return out


if __name__ == "__main__":
    table = capture(sys.argv[1], sys.argv[2], sys.argv[3])
    print("{")
    keys = list(table)
    for i, k in enumerate(keys):
        v = table[k]
        end = "," if i + 1 < len(keys) else ""
        if isinstance(v, str):
            print(' %s: %s%s' % (json.dumps(k), json.dumps(v), end))
        else:
            print(' %s: [\n  %s\n ]%s' % (json.dumps(k), ",\n  ".join(json.dumps(row, separators=(",", ":")) for row in v), end))
    print("}")
