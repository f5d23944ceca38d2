"""The chain path (dfu3d_pseudo_boxes) without the work its result does not need: edge tables kept across calls,
lean voxel records, fewer launches.  Every test compares against something that does not share the code under test:
the stage-by-stage path where its kernels and launch sequence differ from the chain's (the exact repair does not:
both paths launch k_bp_repair, so there the independent references are the product build and the CPU oracle),
a fresh workspace, or the CPU oracle."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import penet_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# launches of ONE dfu3d_pseudo_boxes call on a chunk of the bench workload (dense, joint radius filter, FOV filter,
# RANSAC planes), counted on the host in the `count` build.  The parent commit issues 45.
CHAIN_LAUNCHES = 37
CHAIN_LAUNCHES_PARENT = 45


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _oracle_rows(scenes, p):
    """[(view, inst, cluster, BoxRow)] of dense scenes, oracle RANSAC keyed by view index (as tests/test_gpu_engine.py)."""
    op = O.Params(**{k: getattr(p, k) for k in O.Params.__dataclass_fields__ if hasattr(p, k)})
    out, v = [], 0
    for s in scenes:
        pts = s.points.numpy()
        for c, cal in enumerate(s.calibs):
            oc = O.Calibration({"P2": cal.P2, "R0": cal.R0, "Tr_velo2cam": cal.V2C})
            lid, _ = O.fov_filter(pts, oc, p.fov_hw)
            n = int(s.n_inst[c])
            res = O.depth2pointsrgbpm(s.depth[c].numpy().copy()[:, :, None], None, oc, lid, O.NUSC_CLASSES,
                                      s.masks[c][:n].numpy().astype(np.float32), s.inst_class[c][:n].numpy(),
                                      s.inst_box[c][:n].numpy(), op, plane=None, plane_key=v, want_points=False)
            for r in res.rows:
                out.append((v, r.inst, r.cluster, r))
            v += 1
    return out


def _compare(rows_gpu, exp, tol=1e-6):
    R = rows_gpu.cpu().numpy()
    assert R.shape[0] == len(exp), (R.shape[0], len(exp))
    for got, (v, j, k, r) in zip(R, exp):
        assert (int(got[0]), int(got[1]), int(got[2]), int(got[3])) == (v, j, k, r.cls)
        np.testing.assert_allclose(got[4:16], r.as_vector(), rtol=tol, atol=tol)


def _bench_scenes(seeds, device=None):
    from dfu3d_amd import synth
    kw = {} if device is None else {"device": device}
    return [synth.make_scene(s, H=900, W=1600, M=8, cams=6, dense=True, k_min=30, k_max=40, **kw) for s in seeds]


def test_tables_are_rebuilt_when_the_geometry_changes():
    """One chain workspace, calls with geometry A, B, A, B (B: the theta / phi origins moved by a third of a bin -- the
    same table size, other edges): every call gives the rows of an engine of its own with that geometry.  The step
    A -> B is the call that finds A's tag next to the tables while it is handed B, and must rebuild; the repeats
    (A, A and B, B) take the kept tables."""
    _need_gpu()
    from dfu3d_amd import synth
    from dfu3d_amd.engine import PseudoBoxEngine
    from dfu3d_amd.params import Params
    H, W, M, cams = 180, 320, 5, 3
    pa = Params(bounds_hw=(H, W), fov_hw=(H, W))
    pb = Params(bounds_hw=(H, W), fov_hw=(H, W), vrange_min=(-100.0, -5.0007, -5.0007))
    scenes = [synth.make_scene(70 + f, H=H, W=W, M=M, cams=cams, dense=True, k_min=12, k_max=18) for f in range(4)]
    b = synth.to_view_batch(scenes, pa, DEV, dense=True)
    cap_n = max(s.points.shape[0] for s in scenes)
    kw = dict(views_per_chunk=cams * 4, dense=True, cap_vox=1 << 17, chain=True)
    fresh = {}
    for name, p in (("A", pa), ("B", pb)):
        e = PseudoBoxEngine(p, H, W, M, cap_n, **kw)
        fresh[name], st_ = e.run(b)
        assert st_ == 0 and fresh[name].shape[0] > 3
        geom = e.lanes[0].geom
        fresh[name + "_geom"] = type(geom).from_buffer_copy(geom)
        del e
    ga, gb = fresh["A_geom"], fresh["B_geom"]
    assert ga.t_n * ga.p_n == gb.t_n * gb.p_n and (ga.t_lo, ga.p_lo) != (gb.t_lo, gb.p_lo)
    assert not (fresh["A"].shape == fresh["B"].shape and torch.equal(fresh["A"], fresh["B"])), "B must change the result"
    eng = PseudoBoxEngine(pa, H, W, M, cap_n, **kw)
    for name in ("A", "B", "A", "A", "B", "B", "A"):
        eng.lanes[0].chain_cfg.geom = fresh[name + "_geom"]
        rows, st_ = eng.run(b)
        assert st_ == 0
        assert rows.shape == fresh[name].shape and torch.equal(rows, fresh[name]), name


_PRODUCT_144 = {}


def _run_144(chain):
    """24 bench frames, ONE chunk of 144 views, under whatever library _lib._LIB is."""
    from dfu3d_amd import synth
    from dfu3d_amd.engine import PseudoBoxEngine
    from dfu3d_amd.params import Params
    p = Params()
    if "batch" not in _PRODUCT_144:
        # (made on the host, as the oracle reads them: the generator's draws differ between devices)
        scenes = _bench_scenes([11 + f for f in range(24)])
        b = synth.to_view_batch(scenes, p, DEV, dense=True)
        b.pack_masks()
        _PRODUCT_144["scenes"], _PRODUCT_144["batch"] = scenes, b
    scenes, b = _PRODUCT_144["scenes"], _PRODUCT_144["batch"]
    cap_n = max(s.points.shape[0] for s in scenes)
    eng = PseudoBoxEngine(p, 900, 1600, 8, cap_n, views_per_chunk=144, dense=True, cap_vox=1 << 18, pool_per_view=1 << 17,
                          chain=chain)
    rows, st_ = eng.run(b)
    vox = None
    if not chain:
        n_vox, pix, xyz, st2 = eng.virtual_points(b)
        assert st2 == 0
        vox = (n_vox.cpu(), pix.cpu(), xyz.cpu())
    del eng
    torch.cuda.empty_cache()
    return rows, st_, vox


@pytest.mark.parametrize("variant", ["keybits14", "no_mid"])
def test_fused_repair_equals_the_stage_by_stage_repair_at_144_views(variant, monkeypatch):
    """The test builds that force the exact repair (keybits14: a large share of the voxels is queued; no_mid: the full fp64
    classification) at 24 bench frames in one launch: the chain gives the rows of the stage-by-stage path of the same build
    and of the product build, bit for bit; the voxels of dfu3d_backproject_bin of the test build equal the product's; and
    the rows equal the oracle's on all 24 frames.  Both paths run the repair as k_bp_repair, one launch and one workgroup
    per view (the chain with lean records, the stage path with the record of every voxel), so the two paths of one build
    are no check of the repair against each other: the independent references are the product build's rows and voxels,
    where practically nothing is queued, and the CPU oracle."""
    _need_gpu()
    from dfu3d_amd import _lib
    from dfu3d_amd.params import Params
    if "rows" not in _PRODUCT_144:
        _PRODUCT_144["rows"], st0, _PRODUCT_144["vox"] = _run_144(chain=False)
        assert st0 == 0 and _PRODUCT_144["rows"].shape[0] > 500
        exp = _oracle_rows(_PRODUCT_144["scenes"], Params())
        assert len(exp) > 500
        _PRODUCT_144["oracle"] = exp
    monkeypatch.setattr(_lib, "_LIB", _lib.load_variant(variant))
    rows_s, st_s, vox_s = _run_144(chain=False)
    rows_c, st_c, _ = _run_144(chain=True)
    assert st_s == 0 and st_c == 0
    ref = _PRODUCT_144["rows"]
    assert rows_s.shape == ref.shape and torch.equal(rows_s, ref)
    assert rows_c.shape == ref.shape and torch.equal(rows_c, ref)
    n0, pix0, xyz0 = _PRODUCT_144["vox"]
    n1, pix1, xyz1 = vox_s
    assert torch.equal(n0, n1)
    for v in range(n0.numel()):
        n = int(n0[v])
        assert torch.equal(pix0[v, :n], pix1[v, :n]) and torch.equal(xyz0[v, :n], xyz1[v, :n]), v
    exp = _PRODUCT_144["oracle"]
    _compare(rows_c, exp)


def test_stale_voxel_records_are_never_read():
    """The chain stores pixel and coordinates only for voxels under an instance mask, so the slots of the others keep
    what an earlier pass (or nobody) left there.  Batch X, then batch Y in the same workspace; Y in a workspace filled
    with NaN (all bits set) before its initialisation: bit-equal rows, equal to the oracle's (the four frames of the
    timed-layout parity test, in its layout: packed masks, 12 views per chunk, two lanes)."""
    _need_gpu()
    from dfu3d_amd import _lib, stages as st, synth
    from dfu3d_amd.engine import PseudoBoxEngine
    from dfu3d_amd.params import Params
    p = Params()
    sx = _bench_scenes([300 + f for f in range(4)])
    sy = _bench_scenes([11 + f for f in range(4)])
    bx, by = synth.to_view_batch(sx, p, DEV, dense=True), synth.to_view_batch(sy, p, DEV, dense=True)
    bx.pack_masks()
    by.pack_masks()
    cap_n = max(s.points.shape[0] for s in sx + sy)
    kw = dict(views_per_chunk=12, dense=True, cap_vox=1 << 18, pool_per_view=1 << 17, lanes=2, chain=True)
    eng = PseudoBoxEngine(p, 900, 1600, 8, cap_n, **kw)
    rows_x, st_x = eng.run(bx)
    rows_y, st_y = eng.run(by)
    assert st_x == 0 and st_y == 0 and rows_x.shape[0] > 60
    del eng
    torch.cuda.empty_cache()
    eng2 = PseudoBoxEngine(p, 900, 1600, 8, cap_n, **kw)
    torch.cuda.synchronize()
    for L in eng2.lanes:
        with torch.cuda.stream(L.stream):
            L.chain_ws.fill_(0xFF)                              # every fp64 a NaN, every counter and index -1
            st._lib.check(_lib.lib().dfu3d_chain_workspace_init(L.chain_cfg, L.chain_ws.data_ptr(), st._stream()),
                          "dfu3d_chain_workspace_init")
    torch.cuda.synchronize()
    rows_p, st_p = eng2.run(by)
    assert st_p == 0
    assert rows_p.shape == rows_y.shape and torch.equal(rows_p, rows_y)
    exp = _oracle_rows(sy, p)
    assert len(exp) >= 60
    _compare(rows_y, exp)


def test_chain_launch_count(monkeypatch):
    """One chunk of the bench workload through one dfu3d_pseudo_boxes call, in the build that counts every kernel launch
    of the library on the host: at most CHAIN_LAUNCHES (the parent: CHAIN_LAUNCHES_PARENT)."""
    _need_gpu()
    from dfu3d_amd import _lib, synth
    from dfu3d_amd.engine import PseudoBoxEngine
    from dfu3d_amd.params import Params
    L = _lib.load_variant("count")
    L.dfu3d_debug_launch_count.restype = ctypes.c_longlong
    L.dfu3d_debug_launch_count.argtypes = [ctypes.c_int]
    monkeypatch.setattr(_lib, "_LIB", L)
    p = Params()
    scenes = _bench_scenes([7, 8])
    b = synth.to_view_batch(scenes, p, DEV, dense=True)
    b.pack_masks()
    cap_n = max(s.points.shape[0] for s in scenes)
    eng = PseudoBoxEngine(p, 900, 1600, 8, cap_n, views_per_chunk=12, dense=True, cap_vox=1 << 18, pool_per_view=1 << 17,
                          chain=True)
    rows, st_ = eng.run(b)
    assert st_ == 0 and rows.shape[0] > 20
    L.dfu3d_debug_launch_count(1)
    rows2, _ = eng.run(b)
    n = int(L.dfu3d_debug_launch_count(1))
    print("launches of one chain call: %d" % n)
    assert torch.equal(rows, rows2)
    assert 0 < n <= CHAIN_LAUNCHES < CHAIN_LAUNCHES_PARENT, n
