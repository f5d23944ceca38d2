"""Guard bands and poisoned scratch (tests/guarded_alloc.py) around the HIP stages.

Every family runs twice, under Guarded(0xFF) and under Guarded(0x00): inputs are uploaded, scratch and outputs allocated
and the op run under the mode, so that every buffer the op sees sits between two 64 KB bands and every `empty` buffer
arrives full of the poison.  After each run: the specified outputs equal the family's existing reference (bit for bit
where the family's own test asserts equality, with that test's tolerance otherwise), every band is intact, and the two
runs' specified outputs are bit-equal.  Rows beyond a returned count are unspecified and not compared.  An access more
than 64 KB outside a buffer, and the sub-buffers inside a library-carved workspace, are out of reach.

Scratch and outputs are torch.empty (poisoned); torch.zeros only where the C header makes the caller zero: status words,
pool_cursor, n_vox, n_rows.

Where a family's own checking helper asserts bit equality with its reference, the helper is run as it is under each
poison (under_both): both runs then equal the same bits, and what the helper returns is compared on top.

Entry points run, per family (every one of them could be driven under the mode):
  detector      as_strided self-test on the device (front and back band); a tensor made on autograd's device thread is
                guarded and counted, so the backwards below go through .backward().
  core stages   through dfu3d_amd.stages, called one by one with the runners of tests/test_gpu_stages.py and
                tests/test_gpu_radius_filter.py (alloc = torch.empty): fov_filter, plane_ransac, project_label;
                bin_table_init + backproject_bin (V = 3 at 225 x 400, dense depth with both key axes and sparse depth,
                max_points 1 and 100, two passes each); segments_build with shadow and joint table; radius_filter
                (nb_points 1 and 4); ballquery_fuse plain, masked (behind radius_filter without its compaction) and joint;
                stat_filter (segments of 0, 1, 2, 31, 400, 1300 points, nb_neighbors 30 and 64) alone and behind
                voxel_down_sample; range_cluster (the cases up to 3000 points, four radius pairs, with its sx / sy / si
                scratch handed in); range_cluster + lshape_fit.
  engine        PseudoBoxEngine constructed and run under the mode, so _make_lane's buffers are guarded (12 views of
                180 x 320, two lanes, two passes): stage by stage and chain=True, dense and sparse, byte and packed
                masks, stat_filter off and on, against the oracle's rows as tests/test_gpu_engine.py compares them; and
                cap_vox = 257, which raises ST_VOX_OVERFLOW (status bit and guards only).  The chain's single workspace is
                carved inside the library: only its two outer ends are guarded.  graphs=True is out of scope.
  pointnet2     fps (N = 700 and FPS_BIG: both sides of FPS_ONCHIP), ball_query (BALL_N x BALL_M, one and two scales per
                launch), group (C = 0 too), three_nn (m < 3 too), three_interpolate, invert / inverse_of, gather_backward
                through grouping, query_group and interpolate on BWD_CASES.
  point_stack   in tests/test_gpu_point_stack_edges.py, one family per test: counts (float and int columns) and starts; fps at
                300, 5000 and [16500, 90] rows (both sides of FPS_ONCHIP: the memory form's scratch arrives poisoned);
                ball_query on grid_case (two scales per launch, and one); group (C = 0, C = 17, the plain form);
                query_group through .backward(); bev_sample.
  roipoint      pool and pool_fused on every case of tests/roipoint_ref.py, and feature rows off 16 bytes.
  rcnn_target   point_targets, roi_max_iou (by class and not), roi_subsample on every shape of their test.
  proposals     proposal_ops.proposals: N = 1, 63, 64, 65, 129, 200 and 2500 candidates of 3000.
  pillar / bev  pillar_group (n = 1, 63, 64, 65, 257, both layouts; pillars of 1, 64, 65, 129, 200, 1500 points; more than
                65535 pillars), pillar_max and pillar_max_concat with their backwards; pillar_scatter and its backward.
  center head   assign_targets, decode_bbox_from_heatmap (K = 1024 and 1), center_loss forward and backward (H * W = 1, 63,
                64, 65, 4097, empty heads, 1024 slots on one cell), nms_bev_segments (0 .. 1024 boxes, both kinds, cuts).
  iou / nms     boxes_bev (tile edges of the matrix kernel), boxes_bev_paired (255, 256, 257), rotate_iou_eval (four
                criteria), nms_bev and nms_normal_bev through the wrapper and on caller-made buffers (64, 65, 4097).
  data path     fov_ingest (sizes around the wave and the chunk, empty scenes, box counts, the three modes, 1025 chunks),
                world_aug_collate (every configuration, all scenes in one CSR, 1025 chunks), DataBaseSampler.sample_batch
                (gt_sample_collide + gt_sample_paste; 1026 slots), points_in_boxes_mask, gt_database (1030 boxes),
                la_sampling_batch (objects of 1, 4, 5, 64, 256, 257, 1500 points).
  eval          eval_overlaps, eval_match_scores and eval_match_stats through _Evaluator / eval_class, three metrics.
  optim_ops     FusedAdamStep.step: three steps over four lists of lengths, on tensors carved with sentinel words.
"""
import numpy as np
import pytest
import torch

from tests.guarded_alloc import Guarded

pytestmark = pytest.mark.gpu

POISONS = (0xFF, 0x00)


def cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(x):
    """Tensors (nested in tuples / lists / dicts) -> NumPy arrays."""
    if isinstance(x, torch.Tensor):
        return x.detach().cpu().numpy()
    if isinstance(x, dict):
        return {k: host(v) for k, v in x.items()}
    if isinstance(x, (tuple, list)):
        return [host(v) for v in x]
    return x


def bits_equal(a, b, path="out"):
    """Bit equality of two nested results (NaNs with equal bits are equal)."""
    if isinstance(a, dict):
        assert a.keys() == b.keys(), path
        for k in a:
            bits_equal(a[k], b[k], "%s[%r]" % (path, k))
    elif isinstance(a, (tuple, list)):
        assert len(a) == len(b), path
        for i, (x, y) in enumerate(zip(a, b)):
            bits_equal(x, y, "%s[%d]" % (path, i))
    elif isinstance(a, np.ndarray):
        assert a.dtype == b.dtype and a.shape == b.shape, (path, a.dtype, b.dtype, a.shape, b.shape)
        assert a.tobytes() == b.tobytes(), "%s differs between the two poisons" % path
    else:
        assert a == b, (path, a, b)


def both_poisons(run, verify=None, count=None, min_count=1):
    """run() under each poison -> its specified outputs (tensors); verify(outputs as NumPy) compares with the reference.
    count / min_count: the number of guarded allocations, where it is known / a lower bound of it."""
    outs = []
    for poison in POISONS:
        with Guarded(poison) as g:
            out = run()
            torch.cuda.synchronize()
            g.check()
        assert g.count >= min_count > 0, "%d guarded allocations, at least %d expected" % (g.count, min_count)
        if count is not None:
            assert g.count == count, (g.count, count)
        out = host(out)
        if verify is not None:
            verify(out)
        outs.append(out)
    bits_equal(outs[0], outs[1])
    return outs[0]


# ---- the detector itself, on the device -------------------------------------------------------------------------------
def test_detector_on_the_gpu():
    n = 37
    with Guarded() as g:
        t = torch.empty(n, dtype=torch.float32, device="cuda")
        up = cu(np.arange(5, dtype=np.int16))
        z = torch.zeros(3, dtype=torch.float64, device="cuda")
        assert torch.isnan(t).all() and up.tolist() == [0, 1, 2, 3, 4] and z.tolist() == [0.0] * 3
        assert t.data_ptr() % 512 == 0 and up.data_ptr() % 512 == 0
        g.check()
        torch.as_strided(t, (n + 1,), (1,))[n] = 1.0          # inside the storage the mode owns
        with pytest.raises(AssertionError, match=r"BEHIND aten\.empty\.memory_format -> float32\[37\]") as e:
            g.check()
        assert "first damaged offset 148" in str(e.value) and "test_detector_on_the_gpu" in str(e.value)
        front = torch.as_strided(up, (6,), (1,), up.storage_offset() - 1)
        front[0] = 3
        with pytest.raises(AssertionError, match=r"FRONT of aten\._to_copy\.default -> int16\[5\]"):
            g.check()
    assert g.count == 3

    class Twice(torch.autograd.Function):                      # backward runs on autograd's device thread
        @staticmethod
        def forward(ctx, x):
            return x * 2.0

        @staticmethod
        def backward(ctx, go):
            gi = torch.empty_like(go)
            torch.mul(go, 2.0, out=gi)
            return gi
    x = torch.arange(6, dtype=torch.float32, device="cuda").requires_grad_(True)
    go = torch.ones(6, device="cuda")
    with Guarded() as g:
        Twice.apply(x).backward(go)
        torch.cuda.synchronize()
        g.check()
    assert g.count == 1 and g.records[0].op.startswith("aten.empty_like") and x.grad.tolist() == [2.0] * 6


# ---- pointnet2_ops ---------------------------------------------------------------------------------------------------
from tests import pointnet2_ref as PR  # noqa: E402


@pytest.mark.parametrize("case", [(2, 700, 64), PR.FPS_BIG], ids=str)
def test_pointnet2_fps(case):
    from dfu3d_amd import pointnet2_ops as ops
    B, N, npoint = case
    assert (N > ops.FPS_ONCHIP) == (case == PR.FPS_BIG)
    xyz = PR.cloud(1900 + N, B, N)
    want_idx, want_xyz = PR.fps(xyz, npoint)

    def run():
        st = torch.zeros(1, dtype=torch.int32, device="cuda")
        with ops.status_scope(st):
            idx, new_xyz = ops.fps(cu(xyz), npoint)
        return idx, new_xyz, st

    def verify(out):
        assert np.array_equal(out[0], want_idx) and np.array_equal(out[1], want_xyz) and out[2].tolist() == [0]
    both_poisons(run, verify)


def test_pointnet2_ball_query():
    from dfu3d_amd import pointnet2_ops as ops
    scales = [(0.9, 7), (1.7, 16), (1e3, PR.BALL_NSAMPLE_ALL[-1])]
    for N in PR.BALL_N:
        for M in PR.BALL_M:
            xyz = PR.cloud(10 + N, 2, N, scale=1.0)
            ctr = PR.cloud(20 + M, 2, M, scale=1.0)
            ctr[:, 0] = xyz[:, N // 2]
            want = [PR.ball_query(xyz, ctr, *s) for s in scales]

            def run():
                t_xyz, t_ctr = cu(xyz), cu(ctr)
                two = ops.ball_query(t_xyz, t_ctr, [scales[0][0], scales[1][0]], [scales[0][1], scales[1][1]])
                one = ops.ball_query(t_xyz, t_ctr, [scales[2][0]], [scales[2][1]])
                return list(two) + list(one)

            def verify(out):
                for got, w in zip(out, want):
                    assert np.array_equal(got, w), (N, M)
            both_poisons(run, verify, count=5)


@pytest.mark.parametrize("C", PR.GROUP_C + [0])
def test_pointnet2_group(C):
    from dfu3d_amd import pointnet2_ops as ops
    B, N, M, ns = 2, 301, 37, 5
    rng = np.random.default_rng(30 + C)
    xyz, ctr = PR.cloud(31, B, N), PR.cloud(32, B, M)
    feat = rng.normal(0, 1, (B, C, N)).astype(np.float32) if C else None
    idx = rng.integers(0, N, (B, M, ns)).astype(np.int32)
    modes = (True, False) if C else (True,)

    def run():
        st = torch.zeros(1, dtype=torch.int32, device="cuda")
        t_feat = cu(feat) if C else None
        with ops.status_scope(st):
            return [ops.group(cu(xyz), cu(ctr), t_feat, cu(idx), u) for u in modes] + [st]

    def verify(out):
        for got, u in zip(out, modes):
            assert np.array_equal(got, PR.group(xyz, ctr, feat, idx, u))
        assert out[-1].tolist() == [0]
    both_poisons(run, verify)


@pytest.mark.parametrize("m", PR.NN_M)
def test_pointnet2_three_nn_and_interpolate(m):
    from dfu3d_amd import pointnet2_ops as ops
    B, n = 2, 263
    rng = np.random.default_rng(40 + m)
    unknown, known = PR.cloud(41, B, n), PR.cloud(42 + m, B, m)
    if m >= 3:
        known[:, m // 2:] = known[:, :m - m // 2]
    unknown[:, 0] = known[:, 0]
    want_d, want_i = PR.three_nn(unknown, known)
    feats = [rng.normal(0, 1, (B, C, m)).astype(np.float32) for C in PR.GROUP_C]
    w = rng.uniform(0, 1, (B, n, 3)).astype(np.float32)

    def run():
        dist, idx = ops.three_nn(cu(unknown), cu(known))
        t_w = cu(w)
        return [dist, idx] + [ops.three_interpolate(cu(f), idx, t_w) for f in feats]

    def verify(out):
        assert np.array_equal(out[0], want_d) and np.array_equal(out[1], want_i)
        for got, f in zip(out[2:], feats):
            assert np.array_equal(got, PR.three_interpolate(f, want_i, w))
    both_poisons(run, verify)


def test_pointnet2_inverse_and_ordered_backwards():
    from dfu3d_amd import pointnet2_ops as ops
    from tests.test_gpu_pointnet2 import BWD_CASES
    for name in sorted(BWD_CASES):
        rng = np.random.default_rng(50)
        idx = BWD_CASES[name](rng).astype(np.int32)
        idx[idx == 13] = 14
        B, M, ns = idx.shape
        N, C = 97, 19
        feat = rng.normal(0, 1, (B, C, N)).astype(np.float32)
        go = rng.normal(0, 1, (B, C, M, ns)).astype(np.float32)
        go5 = rng.normal(0, 1, (B, 3 + C, M, ns)).astype(np.float32)
        xyz, ctr = PR.cloud(51, B, N), PR.cloud(52, B, M)

        def run():
            t_idx = cu(idx)
            inv = ops.inverse_of(t_idx, N)
            f1 = cu(feat).requires_grad_(True)
            ops.grouping(f1, t_idx).backward(cu(go))
            f2 = cu(feat).requires_grad_(True)
            ops.query_group(cu(xyz), cu(ctr), f2, t_idx, True).backward(cu(go5))
            return inv.csr, inv.list, f1.grad, f2.grad

        def verify(out):
            for b in range(B):
                w_csr, w_lst = PR.invert(idx[b].reshape(-1), N)
                assert np.array_equal(out[0][b], w_csr) and np.array_equal(out[1][b], w_lst), name
            assert np.array_equal(out[2].view(np.uint32), PR.gather_backward(go, idx, N).view(np.uint32)), name
            assert np.array_equal(out[3].view(np.uint32), PR.gather_backward(go5[:, 3:], idx, N).view(np.uint32)), name
        both_poisons(run, verify)
    for m in (1, 40):                                                       # the weighted form
        rng = np.random.default_rng(60 + m)
        B, C, n = 2, 21, 333
        idx = rng.integers(0, m, (B, n, 3)).astype(np.int32)
        if m > 20:
            idx[idx == 7] = 8
        w = rng.uniform(0, 1, (B, n, 3)).astype(np.float32)
        feat = rng.normal(0, 1, (B, C, m)).astype(np.float32)
        go = rng.normal(0, 1, (B, C, n)).astype(np.float32)
        want = PR.gather_backward(go, idx, m, weight=w, k=3)

        def run():
            f = cu(feat).requires_grad_(True)
            ops.interpolate(f, cu(idx), cu(w)).backward(cu(go))
            return f.grad
        both_poisons(run, lambda out: np.testing.assert_array_equal(out.view(np.uint32), want.view(np.uint32)))


# ---- PseudoBoxEngine -------------------------------------------------------------------------------------------------
ENG_H, ENG_W, ENG_M, ENG_CAMS, ENG_FRAMES = 180, 320, 5, 3, 4


@pytest.fixture(scope="module")
def engine_cases():
    """(dense, stat_filter) -> (params, scenes, oracle rows), each computed once."""
    from dfu3d_amd import synth
    from dfu3d_amd.params import Params
    from tests.test_gpu_engine import _oracle_rows
    done = {}

    def get(dense, stat):
        if (dense, stat) not in done:
            p = Params(bounds_hw=(ENG_H, ENG_W), fov_hw=(ENG_H, ENG_W), stat_filter=stat)
            scenes = [synth.make_scene(70 + f, H=ENG_H, W=ENG_W, M=ENG_M, cams=ENG_CAMS, dense=dense, k_min=12, k_max=18)
                      for f in range(ENG_FRAMES)]
            exp, _ = _oracle_rows(scenes, p, dense)
            assert len(exp) > 3
            done[dense, stat] = (p, scenes, exp)
        return done[dense, stat]
    return get


def _engine_run(p, scenes, dense, chain, packed, cap_vox=1 << 17):
    from dfu3d_amd import synth
    from dfu3d_amd.engine import PseudoBoxEngine
    b = synth.to_view_batch(scenes, p, "cuda:0", dense=dense)
    if packed:
        b.pack_masks()
    cap_n = max(s.points.shape[0] for s in scenes)
    eng = PseudoBoxEngine(p, ENG_H, ENG_W, ENG_M, cap_n, views_per_chunk=ENG_CAMS * 2, dense=dense, cap_vox=cap_vox,
                          lanes=2, chain=chain)
    rows, status = eng.run(b)
    rows2, status2 = eng.run(b)                                # the lanes' buffers as the first pass left them
    assert status2 == status and torch.equal(rows, rows2)
    return rows, status


@pytest.mark.parametrize("stat", [False, True], ids=["plain", "stat_filter"])
@pytest.mark.parametrize("packed", [False, True], ids=["byte_masks", "packed_masks"])
@pytest.mark.parametrize("dense", [True, False], ids=["dense", "sparse"])
@pytest.mark.parametrize("chain", [False, True], ids=["stages", "chain"])
def test_engine_under_guards(engine_cases, chain, dense, packed, stat):
    from tests.test_gpu_engine import _compare
    p, scenes, exp = engine_cases(dense, stat)

    def run():
        rows, status = _engine_run(p, scenes, dense, chain, packed)
        assert status == 0
        _compare(rows, exp)                                    # as tests/test_gpu_engine.py compares: 1e-6
        return rows
    both_poisons(run, min_count=2 * 49)                        # _make_lane makes at least 49 buffers per lane


@pytest.mark.parametrize("chain", [False, True], ids=["stages", "chain"])
def test_engine_voxel_overflow_under_guards(engine_cases, chain):
    """cap_vox far below the voxels of a view: ST_VOX_OVERFLOW is raised and nothing is written past vox_pix, it_bits,
    it_x/y/z (V * cap_vox each).  The rows are unspecified."""
    from dfu3d_amd import stages as st
    p, scenes, _ = engine_cases(True, False)
    for poison in POISONS:
        with Guarded(poison) as g:
            _, status = _engine_run_once(p, scenes, chain, cap_vox=257)
            torch.cuda.synchronize()
            g.check()
        assert g.count > 0 and status & st.ST_VOX_OVERFLOW


def _engine_run_once(p, scenes, chain, cap_vox):
    from dfu3d_amd import synth
    from dfu3d_amd.engine import PseudoBoxEngine
    b = synth.to_view_batch(scenes, p, "cuda:0", dense=True)
    cap_n = max(s.points.shape[0] for s in scenes)
    eng = PseudoBoxEngine(p, ENG_H, ENG_W, ENG_M, cap_n, views_per_chunk=ENG_CAMS * 2, dense=True, cap_vox=cap_vox,
                          lanes=2, chain=chain)
    return eng.run(b)


def under_both(fn, *args, **kw):
    """A checking helper of another test module (it uploads, runs and asserts against its reference itself) under each
    poison.  Where that helper asserts bit equality with the reference, the two runs are bit-equal to each other through
    it; what it returns is compared bit for bit on top."""
    return both_poisons(lambda: fn(*args, **kw))


# ---- pillar_ops and bev_ops ------------------------------------------------------------------------------------------
def _group_fields(g):
    return {k: getattr(g, k) for k in ('kept_idx', 'unq_inv', 'unq_cnt', 'coords', 'offsets', 'plist', 'features')}


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_pillar_group_small_sizes(n):
    from tests import pillar_vfe_ref as VR
    from tests import test_gpu_pillar_vfe as T
    for layout in (VR.LAYOUT_PILLAR, VR.LAYOUT_SIMPLE2D):
        pts = T.random_points(np.random.default_rng(100 + n), n, 3, cols=6)
        both_poisons(lambda: _group_fields(T.check_group(pts, 3, layout=layout, abs_xyz=(n % 2 == 1), dist=(n != 64))[0]))


def test_pillar_group_max_and_backward_on_long_pillars():
    """Pillars of 1, 64, 65, 129, 200 and 1500 points: pillar_group, pillar_max and pillar_max_concat with their backwards
    (check_max goes through .backward())."""
    from tests import test_gpu_pillar_vfe as T
    pts = T.long_pillar_points(np.random.default_rng(21), sizes=(1, 64, 65, 1500, 129, 200), extra=500)

    def run():
        g, ref, _ = T.check_group(pts, 2, dist=True)
        assert {1, 64, 65, 129, 200, 1500} <= set(ref['unq_cnt'].tolist())
        rng = np.random.default_rng(30)
        for C in (1, 32, 100):
            T.check_max(rng.normal(size=(g.n_kept, C)).astype(np.float32), g, ref['unq_inv'], rng, "random C=%d" % C)
        x = np.maximum(rng.normal(size=(g.n_kept, 64)), 0).astype(np.float32)
        x[:, ::3] = 0.0
        T.check_max(x, g, ref['unq_inv'], rng, "relu")
        return _group_fields(g)
    both_poisons(run)


@pytest.mark.parametrize("name", ["smallest", "ragged_tiles_empty_sample", "c_above_64", "scatter3d"])
def test_bev_pillar_scatter_forward_and_backward(name):
    from tests import pillar_scatter_ref as SR
    from tests import test_gpu_pillar_scatter as T
    from dfu3d_amd import bev_ops
    case = [c for c in T.CASES if c[0] == name][0]
    _, B, C, nz, ny, nx, P, _ = case
    f, coords = T._inputs(case)
    want, want_map, status = SR.scatter(f, coords, B, (nx, ny, nz))
    gc = np.random.default_rng(len(name)).standard_normal(want.shape).astype(np.float32)
    want_grad = SR.scatter_backward(gc, coords, B, (nx, ny, nz), want_map, P)
    assert status == 0

    def run():
        ft = T._dev(f).requires_grad_(True)
        info = bev_ops.ScatterInfo()
        canvas = bev_ops.pillar_scatter(ft, T._dev(coords), B, (nx, ny, nz), info=info)
        canvas.backward(T._dev(gc))
        return canvas, info.cell_map, info.status, ft.grad

    def verify(out):
        assert SR.same_bits(out[0], want) and np.array_equal(out[1], want_map) and not out[2].any()
        assert SR.same_bits(out[3], want_grad)
    both_poisons(run, verify)


# ---- roipoint_ops, rcnn_target_ops, proposal_ops ---------------------------------------------------------------------
def test_roipoint_pool_plain_and_fused():
    from tests import roipoint_ref as RR
    from tests import test_gpu_roipoint as T
    for name in sorted(T._cases()):
        c = T._cases()[name]
        for fused in (False, True):
            exp = T._expected(name, fused)

            def verify(out):
                assert RR.same_bits(out[2], exp[2]) and RR.same_bits(out[1], exp[1]) and RR.same_bits(out[0], exp[0]), name
            both_poisons(lambda: T._run(c, fused), verify)
    c = T._cases()['extra']                                     # feature rows one float off 16 bytes: the dword path
    under_both(T._run, c, True, misalign=True)


def test_rcnn_target_point_targets_max_iou_and_subsample():
    from dfu3d_amd import rcnn_target_ops as ops
    from dfu3d_amd.pcdet_kitti import iou3d_nms_utils
    from tests import rcnn_target_ref as TR
    from tests import test_gpu_rcnn_target as T
    for name in T.POINT_SHAPES + ['faces']:
        exp = T.point_expected(name, 3, True)

        def verify(out):
            assert np.array_equal(out[0], exp[0]) and TR.same_bits(out[1], exp[1]) and np.array_equal(out[2], exp[2]), name
        both_poisons(lambda: T.run_points(name, 3, True), verify)
    for shape in T.IOU_SHAPES:
        rois, labels, gt = T.iou_case(*shape)
        full = np.stack([iou3d_nms_utils.boxes_iou3d_gpu(T.t(rois[b]), T.t(gt[b, :, :7])).cpu().numpy() for b in range(3)])
        for by_class in (True, False):
            rov, rasg = TR.max_iou(full, labels, gt, by_class)

            def verify(out):
                assert TR.same_bits(out[0], rov) and np.array_equal(out[1], rasg), (shape, by_class)
            both_poisons(lambda: ops.roi_max_iou(T.t(rois), T.t(labels), T.t(gt), by_class), verify)
    for M, R_ in T.SAMPLE_SHAPES:
        cfg = dict(TR.SAMPLER, ROI_PER_IMAGE=R_)
        ov = T.sample_rows(M)
        rng = np.random.default_rng(7 * M + R_)
        key = rng.integers(0, max(M // 3, 2), ov.shape).astype(np.int32)
        u = rng.uniform(0, 1, (len(ov), R_)).astype(np.float32)
        u[:, 0], u[:, -1] = 0.0, np.nextafter(np.float32(1), np.float32(0))
        exp, exp_status, _ = TR.subsample(ov, cfg, key, u)

        def verify(out):
            assert np.array_equal(out[0], exp) and out[1].reshape(-1).tolist() == [exp_status], (M, R_)
        both_poisons(lambda: ops.roi_subsample(T.t(ov), cfg, T.t(key), T.t(u)), verify)


@pytest.mark.parametrize("N", [1, 63, 64, 65, 129, 200])
def test_proposals_block_edges(N):
    from tests import proposal_ref as P
    from tests import test_gpu_proposals as T
    rng = np.random.default_rng(1000 * N + 7)
    scores, boxes, labels = P.distinct_scores(rng, 3, N), P.clustered_boxes(rng, 3, N), T.labels_for(rng, (3, N))
    kept = P.walk_ref(scores, boxes, 0.3, N)                   # (the reference walks with the NMS kernel: outside the mode)
    for post in sorted({max(min(len(k) for k in kept) // 2, 1), max(len(k) for k in kept) + 3}):
        exp = P.pad_ref(kept, scores, labels, boxes, post)
        both_poisons(lambda: T.run(scores, labels, boxes, 0.3, N, post), lambda out: T.check(out, exp, "post %d" % post))


def test_proposals_beyond_the_segmented_cap():
    from tests import proposal_ref as P
    from tests import test_gpu_proposals as T
    B, N, pre, post = 2, 3000, 2500, 512
    rng = np.random.default_rng(41)
    scores, labels = P.distinct_scores(rng, B, N), T.labels_for(rng, (B, N))
    boxes = P.clustered_boxes(rng, B, N, centres=40, jitter=0.06)
    exp = P.pad_ref(P.walk_ref(scores, boxes, 0.8, pre), scores, labels, boxes, post)
    both_poisons(lambda: T.run(scores, labels, boxes, 0.8, pre, post), lambda out: T.check(out, exp, "tight"))


# ---- CenterHead: targets, decode, loss, segmented NMS ----------------------------------------------------------------
def test_center_head_targets_and_decode():
    from tests import center_head_ref as CR
    from tests import test_gpu_center_head as T
    cfg = T.CFGS["A"]
    gt = T.random_boxes(np.random.default_rng(61), cfg, 4, 512, 500)
    gt[1] = T.random_boxes(np.random.default_rng(62), dict(cfg, class_names=['Car']), 1, 512, 500, n_exact=500)[0]
    want = CR.assign_targets(gt, cfg)

    def assign():
        head = T.make_head(cfg)
        ret = head.assign_targets(torch.from_numpy(gt).cuda(), feature_map_size=list(cfg['map_hw']), check=True)
        return {k: ret[k] for k in ('heatmaps', 'target_boxes', 'inds', 'masks', 'target_boxes_src')}
    both_poisons(assign, lambda out: T.compare_assign(out, want, "A, B = 4"))
    cfg2 = dict(CR.CFG_A, point_cloud_range=[-54.0, -54.0, -5.0, 54.0, 54.0, 3.0], voxel_size=[0.075, 0.075, 0.2], stride=8)
    lim = [-50.0, -50.0, -9.0, 50.0, 50.0, 9.0]
    for K, n_cls, B in ((1024, 3, 3), (1, 1, 2)):
        d = CR.decode_inputs(77 + K, B, n_cls, 180, 180, True, True)
        want_d = CR.decode_bbox_from_heatmap(d['heatmap'], d['rot_cos'], d['rot_sin'], d['center'], d['center_z'], d['dim'],
                                             cfg2['point_cloud_range'], cfg2['voxel_size'], cfg2['stride'], vel=d['vel'],
                                             iou=d['iou'], K=K, score_thresh=0.5, post_center_limit_range=lim)
        both_poisons(lambda: T.run_decode(d, K, 0.5, lim, cfg2), lambda out: T.compare_decode(out, want_d))


@pytest.mark.parametrize("edge", [dict(hw=(1, 1)), dict(hw=(7, 9)), dict(hw=(8, 8)), dict(hw=(5, 13)), dict(hw=(17, 241)),
                                  dict(hw=(8, 8), empty=True), dict(hw=(7, 9), full_same_ind=True, n_max=1024)],
                         ids=lambda e: "-".join("%s%s" % kv for kv in e.items()))
def test_center_loss_forward_and_backward(edge):
    from dfu3d_amd import center_loss_ops
    from tests import center_loss_ref as LR
    from tests import test_gpu_center_loss as T
    H, W = edge['hw']
    targets, preds, order = T.random_case(H * W + 1, [1, 3], 1, H, W, edge.get('n_max', 6),
                                          edge.get('full_same_ind', False), edge.get('empty', False))
    weights = dict(cls_weight=0.5, loc_weight=0.25, code_weights=[1.0, 1.0, 0.5, 2.0, 2.0, 2.0, 0.25, 0.25])
    fwd = LR.forward(preds, targets, order, weights)
    up = np.zeros(5, np.float32)
    up[-1] = 1.0
    hm64, reg = LR.backward(preds, targets, order, weights, fwd, grad_losses=up)

    def run():
        dev, tg = T.to_dev(preds), T.targets_dev(targets)
        losses, _ = center_loss_ops.center_loss([d['hm'] for d in dev], tg['heatmaps'], [[d[k] for k in order] for d in dev],
                                                tg['target_boxes'], tg['inds'], tg['masks'], **weights)
        losses[-1].backward()
        return [losses] + [{k: v.grad for k, v in d.items()} for d in dev]

    def verify(out):
        assert np.isfinite(out[0]).all() and T.within(out[0], fwd['losses'])
        for h in range(2):
            assert T.within(out[1 + h]['hm'], hm64[h].astype(np.float32)), h
            for key in order:
                assert np.array_equal(out[1 + h][key].view(np.uint32), np.ascontiguousarray(reg[h][key]).view(np.uint32)), (h, key)
    both_poisons(run, verify)


def test_nms_segments():
    """Segments of 0, 1, 63, 64, 65, 500, 1000 and 1024 boxes, rotated and axis-aligned, C = 7 and 9, with cuts."""
    from oracle import iou3d_oracle as oracle
    from tests import test_gpu_center_postprocess as T
    from tests.iou3d_cases import random_boxes
    rng = np.random.default_rng(T.SCENE_SEED)
    lists = [random_boxes(rng, n, T._spread(n)) for n in T.COUNTS]
    for normal in (False, True):
        pairs = [oracle.pair_ious(b, normal=normal) for b in lists]
        thresh, half = oracle.widest_gap_threshold(np.concatenate([p[2] for p in pairs]), 0.2)
        assert half > T.MARGIN
        keeps = [oracle.nms_sparse(b, -np.arange(len(b), dtype=np.float64), thresh, normal=normal, pairs=p)[0]
                 for b, p in zip(lists, pairs)]
        for C, pre, post in ((7, None, None), (9, 300, 40)):
            want = keeps if pre is None else \
                [oracle.nms_sparse(b, -np.arange(len(b), dtype=np.float64), float(np.float32(thresh)), normal=normal,
                                   pre_maxsize=pre)[0][:post] for b in lists]
            blk = T._block(lists, C=C, fill="nan")
            both_poisons(lambda: T._run(blk, T.COUNTS, np.float32(thresh), pre_max=pre, post_max=post, normal=normal),
                         lambda out: T._check(out[0], out[1], want, "C=%d normal=%s" % (C, normal)))


# ---- rotated IoU / NMS -----------------------------------------------------------------------------------------------
def test_rotated_iou_and_nms():
    from tests import iou3d_cases as C
    from tests import test_gpu_iou3d as T3
    from tests import test_gpu_iou3d_edges as TE
    from tests import test_gpu_nms_patterns as TN
    rng = np.random.default_rng(47)
    for n, m in [(1, 1), (7, 31), (8, 32), (9, 33), (9, 65), (1, 700)]:
        a, b = C.random_boxes(rng, n, 4.0), C.random_boxes(rng, m, 4.0)
        a[-1], b[-1] = a[0], a[0]
        under_both(TE._check_matrix, a, b)
    from dfu3d_amd import stages as st
    from dfu3d_amd.pcdet_kitti.rotate_iou import rotate_iou_gpu_eval
    for n in (1, 255, 256, 257):
        under_both(TE.test_paired_entry_point, n)              # against the checker, with that test's tolerances
        a, b = C.random_boxes(rng, n, 3.0), C.random_boxes(rng, n, 3.0)
        both_poisons(lambda: [st.boxes_bev_paired(cu(a), cu(b), iou=i) for i in (False, True)])     # and the same bits twice
    q, r = np.zeros((77, 5), np.float32), np.zeros((130, 5), np.float32)
    for x in (q, r):
        x[:, :2], x[:, 2:4], x[:, 4] = rng.uniform(-12, 12, (len(x), 2)), rng.uniform(0.5, 5, (len(x), 2)), rng.uniform(-3.2, 3.2, len(x))
    for criterion in (-1, 0, 1, 2):
        under_both(T3.test_rotate_iou_eval_mirror, criterion)
        both_poisons(lambda: rotate_iou_gpu_eval(q, r, criterion))
    for normal in (False, True):
        for n in (64, 65, 4097):
            both_poisons(lambda: TN._wrapped(TN._chain(n), 0.25, normal),
                         lambda out: np.testing.assert_array_equal(out, np.arange(0, n, 2)))
            both_poisons(lambda: TN._raw(TN._chain(n), 0.25, normal),          # caller-made mask, keep and count
                         lambda out: np.testing.assert_array_equal(out, np.arange(0, n, 2)))
        b, expected = TN._far_reach(4097)
        both_poisons(lambda: TN._wrapped(b, 0.25, normal), lambda out: np.testing.assert_array_equal(out, expected))


# ---- ingest, world augmentation, ground-truth sampling, points in boxes, la_sampling ---------------------------------
@pytest.mark.parametrize("C", [3, 4, 5])
def test_ingest_sizes_around_the_wave_and_the_chunk(C):
    from tests import test_gpu_ingest as T
    rng = np.random.default_rng(180 + C)
    sizes = (1, 63, 64, 65, 255, 256, 257)
    scenes = [T._cloud(rng, n, C) for n in sizes]
    shapes = [T.SHAPES[b % 2] for b in range(len(sizes))]
    under_both(T._check, scenes, T._calibs(len(sizes)), shapes)
    both_poisons(lambda: T._run(scenes, T._calibs(len(sizes)), shapes)[:2])
    under_both(T._check, [T._cloud(rng, 0, C)], T._calibs(1), [T.SHAPES[0]])
    sizes = (70, 0, 0, 130, 0)
    under_both(T._check, [T._cloud(rng, n, C) for n in sizes], T._calibs(5), [T.SHAPES[b % 2] for b in range(5)],
               [T._boxes_for(rng, m) for m in (2, 0, 0, 3, 0)])


def test_ingest_second_pass_of_the_scan_and_box_counts():
    from dfu3d_amd import ingest_ops as ops
    from tests import test_gpu_ingest as T
    rng = np.random.default_rng(1899)
    n = ops.CHUNK * 1024 + 1                                   # 1025 chunks: the smallest scene that takes the second pass
    under_both(T._check, [T._cloud(rng, 70, 4), T._cloud(rng, n, 4), T._cloud(rng, 90, 4)], T._calibs(3),
               [T.SHAPES[0], T.SHAPES[1], T.SHAPES[0]])
    scenes = [T._cloud(rng, 6000, 4), T._cloud(rng, 0, 4), T._cloud(rng, 2500, 4), T._cloud(rng, 257, 4)]
    boxes = [T._boxes_for(rng, 3), T._boxes_for(rng, 5), T._boxes_for(rng, 100), np.zeros((0, 7))]
    shapes = [T.SHAPES[0], T.SHAPES[1], T.SHAPES[0], T.SHAPES[1]]
    for mode in (ops.EMIT, ops.COUNT, ops.EMIT | ops.COUNT):
        under_both(T._check, scenes, T._calibs(4), shapes, boxes, mode=mode)


from tests import world_aug_cases as W  # noqa: E402


@pytest.mark.parametrize("ci", range(W.N_CFG))
def test_world_aug_collate(ci):
    """Scene sizes 0, 1, 63, 64, 1023, 1024, 1025, 3000 and the planted ones in one CSR, and empty scenes side by side."""
    from tests import test_gpu_world_aug as T
    from tests import world_aug_ref as WR
    for pick in (list(range(W.n_scenes())), [2, 0, 0, 3, 8, 0]):
        ops = T._ops(ci, pick)
        want = WR.batch(ops, W.pc_range(ci), mask_boxes=W.training(ci))
        n_rows = sum(len(o[0]) for o in ops)
        both_poisons(lambda: T._run(ops, W.pc_range(ci), W.training(ci), want_aug=True, want_keep=True),
                     lambda out: T._check_against_restatement(out, want, n_rows))


def test_gt_sample_paste(tmp_path):
    """DataBaseSampler.sample_batch (dfu3d_gt_sample_collide + dfu3d_gt_sample_paste) over 40 scenes: no scene points, every
    candidate colliding, groups with n <= 0, against the restatement."""
    from dfu3d_amd.pcdet_kitti.database_sampler import DataBaseSampler
    from tests import gt_sampling_ref as GR
    from tests import test_gpu_gt_sampling as T
    rng = np.random.default_rng(3)
    boxes = [[rng.uniform(-40, 40), rng.uniform(-40, 40), -1.0, 4.0, 1.8, 1.5, rng.uniform(-3, 3)] for _ in range(40)]
    T._planted_db(tmp_path, boxes, [['Car', 'Pedestrian'][k % 2] for k in range(40)], npts=30)
    cfg = T._cfg(['Car:3', 'Pedestrian:2'], width=(0.2, 0.2, 0.0), limit=True)
    scenes = []
    for s in range(40):
        n = 0 if s % 17 == 0 else int(rng.choice([1, 63, 64, 65, 1023, 1024, 1025, 2500]))
        p = np.zeros((n, 4), np.float32)
        p[:, :2], p[:, 2], p[:, 3] = rng.uniform(-45, 45, (n, 2)), rng.uniform(-2, 0, n), rng.random(n)
        if s % 13 == 0:
            gb, gn = np.array([[0, 0, -1, 300, 300, 3, 0]], np.float32), np.array(['Van'])
        elif s % 11 == 0:
            gb = np.array([[60 + 6 * k, 60, -1, 4, 1.8, 1.5, 0] for k in range(5)], np.float32)
            gn = np.array(['Car', 'Car', 'Car', 'Pedestrian', 'Pedestrian'])
        else:
            gb, gn = np.zeros((0, 7), np.float32), np.array([], '<U10')
        scenes.append({'points': p, 'gt_boxes': gb, 'gt_names': gn, 'gt_boxes_mask': np.ones(len(gn), bool)})
    copy = lambda: [{k: v.copy() for k, v in d.items()} for d in scenes]        # noqa: E731
    ref = GR.RefSampler(tmp_path, cfg, ['Car', 'Pedestrian'])
    np.random.seed(9)
    exp = [ref(d)[0] for d in copy()]

    def run():
        smp = DataBaseSampler(tmp_path, cfg, ['Car', 'Pedestrian'], device="cuda:0")
        np.random.seed(9)
        batch = smp.sample_batch(copy())
        got = batch.split()
        for s in range(len(scenes)):
            T._same(got[s], exp[s]["points"], exp[s]["gt_boxes"], exp[s]["gt_names"], s)
        return batch.points[:int(batch.point_off[-1])]
    both_poisons(run)


def test_gtdb_points_in_boxes_and_database():
    from dfu3d_amd.pcdet_kitti.roiaware_pool3d_utils import points_in_boxes_cpu
    from oracle import gtdb_oracle as G
    from tests import test_gpu_gtdb as T
    rng = np.random.default_rng(5)
    for n, nb in ((1, 1), (63, 3), (65, 2), (5000, 17)):
        pts, boxes = T._scene(rng, max(n, 1), max(nb, 1))
        pts, boxes = pts[:n], boxes[:nb]
        exp = G.points_in_boxes_cpu(pts, boxes)
        both_poisons(lambda: points_in_boxes_cpu(pts[:, :3].copy(), boxes),
                     lambda out: np.testing.assert_array_equal(out, exp))
    frames = [T._scene(rng, n, nb) for n, nb in ((3000, 9), (1, 2), (500, 0), (800, 5))]
    both_poisons(lambda: T._database_matches_oracle(frames)[1])
    frames = [T._scene(np.random.default_rng(16), n, nb, size=(0.5, 2.5)) for n, nb in ((400, 700), (300, 330))]
    cnt = both_poisons(lambda: T._database_matches_oracle(frames)[1])          # 1030 boxes: the second pass of the scan
    assert len(cnt) > 1024 and cnt[1024:].any()


def test_la_sampling_batch():
    """Objects of 4, 5, 256, 257 and 1500 points (and 1, 64): the restatement's rows, bit for bit, unless an angle sits on a
    bin edge (tests/test_gpu_la_sampling.py's rule)."""
    from dfu3d_amd.pcdet_kitti.database_sampler_virtual import la_sampling_batch
    from oracle import la_sampling_oracle as LA
    from tests import test_gpu_la_sampling as T
    rng = np.random.default_rng(7)
    objs = []
    for n in (4, 5, 256, 257, 1500, 1, 64, 4, 5, 256, 257, 1500):
        d, a = rng.uniform(4, 60), rng.uniform(-np.pi, np.pi)
        objs.append(T._object(rng, n, np.array([d * np.cos(a), d * np.sin(a), rng.uniform(-1.5, 0.5)])))
    objs.append(np.zeros((7, 8), np.float32))
    exp = [LA.la_sampling(o, 0.006, 0.003) for o in objs]

    def verify(out):
        for o, g, e in zip(objs, out, exp):
            same = g.shape == e.shape and np.array_equal(g.view(np.uint32), e.view(np.uint32))
            assert same or T._near_tie(o, 0.006, 0.003)
    both_poisons(lambda: la_sampling_batch(objs, 0.006, 0.003), verify)


# ---- the eval stage and the optimiser --------------------------------------------------------------------------------
def test_eval_stage():
    from dfu3d_amd.pcdet_kitti import eval as E
    from oracle import kitti_eval_oracle as KO
    from tests import test_gpu_kitti_eval as T
    classes = ['Car', 'Pedestrian']
    cls = [KO.CLASS_NAMES.index(c) for c in classes]
    mo = np.stack([np.full((3, 2), 0.7), np.full((3, 2), 0.5), np.full((3, 2), 0.3)], 0)
    gts, dts = T.eval_cases.make_annos(77, 20, max_gt=12, extra_dt=10, classes=tuple(classes))
    for metric in (0, 1, 2):
        want = KO.eval_class(gts, dts, cls, (0, 1, 2), metric, mo, metric == 0)

        def run():
            ev, safe = T.check_overlaps(E, gts, dts, metric, mo[:, metric, :])
            r = E.eval_class(gts, dts, cls, (0, 1, 2), metric, mo, metric == 0, _evaluator=ev)
            if safe:
                for key, tol in (('recall', 1e-12), ('precision', 1e-12), ('orientation', 1e-9)):
                    np.testing.assert_allclose(r[key], want[key], rtol=0, atol=tol, equal_nan=True)
            return {k: np.asarray(r[k]) for k in ('recall', 'precision', 'orientation')}
        both_poisons(run)


@pytest.mark.parametrize("lengths", [[1], [5], [4095, 4096, 4097], [1, 1, 2, 64, 4097, 8199]], ids=str)
def test_optim_fused_adam_steps(lengths):
    from tests import test_gpu_optimizer as T
    out = [None, None]
    for k, poison in enumerate(POISONS):
        with Guarded(poison) as g:
            out[k] = T.run_three_steps(lengths, 1)             # asserts every step's bits and the sentinel words itself
            torch.cuda.synchronize()
            g.check()
        assert g.count > 0
    assert np.array_equal(out[0][0], out[1][0]) and all(np.array_equal(a, b) for a, b in zip(out[0][1], out[1][1]))


# ---- the core stages through stages.py, one by one -------------------------------------------------------------------
from tests import test_gpu_stages as TS  # noqa: E402


def _empty(n, dtype):
    """Scratch and outputs: poisoned under the mode."""
    return torch.empty(n, dtype=dtype, device="cuda")


@pytest.fixture(scope="module")
def st():
    from dfu3d_amd import stages
    return stages


def test_core_fov_plane_label(st):
    from dfu3d_amd import synth
    scenes, p = TS._lidar_setup(20)
    cap_n = max(s.points.shape[0] for s in scenes)
    planes_o = TS._oracle_planes(scenes, p)

    def run():
        b = synth.to_view_batch(scenes, p, TS.DEV)
        fov_idx, n_fov, plane = TS._fov_plane_run(st, b, p, cap_n, alloc=_empty)
        out = TS._project_label_run(st, b, p, cap_n, planes_o, fov_idx, n_fov, alloc=_empty)
        np.testing.assert_allclose(plane.cpu().numpy().reshape(-1, 4), planes_o, rtol=1e-9, atol=1e-9)
        TS._fov_label_verify(scenes, p, cap_n, planes_o, fov_idx, n_fov, *out)
        return plane, n_fov, out[0], out[1]                    # rows beyond the counts are unspecified
    both_poisons(run)


@pytest.fixture(scope="module")
def bp_scene():
    """V = 3 at 225 x 400, dense and sparse depth, with rows of constant depth and a patch that lands in a few bins; the
    oracle's answers per (sparse, max_points, key_axis), computed once."""
    from dfu3d_amd import synth
    out = {}
    for sparse in (False, True):
        s = synth.make_scene(31, H=225, W=400, M=4, cams=3, dense=not sparse, k_min=10, k_max=14)
        depth = s.depth.numpy().copy()
        depth[0, 100:110, :] = 7.5
        depth[1, 60:90, 100:200] = 0.02
        out[sparse] = (depth, s.calibs, s.masks.numpy())
    expected = {}

    def oracle(sparse, max_points, key_axis):
        key = (sparse, max_points, key_axis)
        if key not in expected:
            depth, cal, masks = out[sparse]
            expected[key] = [TS._bp_oracle(depth[v], cal[v], masks[v], max_points, 1000000, key_axis) for v in range(3)]
        return expected[key]
    return out, oracle


@pytest.mark.parametrize("sparse,max_points,key_axis", [(False, 1, 1), (False, 100, 1), (False, 1, 2), (False, 100, 2),
                                                        (True, 1, 1), (True, 100, 1)])
def test_core_backproject(st, bp_scene, sparse, max_points, key_axis):
    scenes, oracle = bp_scene
    depth, cal, masks = scenes[sparse]
    want = oracle(sparse, max_points, key_axis)

    def run():
        got = TS._bp_run(st, depth, cal, masks, max_points, 1000000, key_axis, alloc=_empty)
        TS._bp_assert_oracle(got, want)                        # bit for bit up to n_vox, status 0
        return got[0]
    both_poisons(run)


def test_core_segments_build(st):
    c = TS._segments_case()

    def run():
        o = TS._segments_run(st, c, alloc=_empty)
        TS._segments_verify(c, o)
        return [o[k] for k in ("cursor", "base_a", "cnt_a", "base_b", "cnt_b", "base_ab", "cnt_ab")]
    both_poisons(run)


def test_core_radius_filter(st):
    segs, radius = TS._radius_filter_cases()
    for nb in (1, 4):
        def run():
            base, out_cnt, X = TS._radius_filter_run(st, segs, radius, nb, alloc=_empty)
            TS._radius_filter_verify(segs, radius, nb, base, out_cnt, X)
            return out_cnt
        both_poisons(run)


def test_core_ballquery_fuse_plain_masked_joint(st):
    from tests import test_gpu_radius_filter as TR
    segsA, segsB = TS._fuse_segments(12, TS.FUSE_CASES)

    def plain():
        base_a, ncb, nbase, X = TS._ballquery_fuse_run(st, segsA, segsB, alloc=_empty)
        TS._ballquery_fuse_verify(segsA, segsB, base_a, ncb, nbase, X)
        return ncb, nbase
    both_poisons(plain)
    mA, mB = TS._fuse_segments(121, TS.MASKED_FUSE_CASES, far=True)

    def masked():
        base_a, ncb, nbase, X = TS._ballquery_fuse_run(st, mA, mB, radius=TS.MASKED_FUSE_RADIUS, alloc=_empty)
        TS._masked_fuse_verify(mA, mB, TS.MASKED_FUSE_RADIUS, base_a, ncb, X)
        return ncb, nbase
    both_poisons(masked)
    ra = np.array([3.0, 3.0, 3.0, -1.0, 0.6, 0.0])             # the joint pass: radius -1 empties a LiDAR list, 0 keeps it
    rb = np.array([0.6, 3.0, 0.6, 3.0, 0.6, 3.0])
    under_both(TR._joint_filter_then_fuse_equals_oracle, st, mA, mB, ra, rb, alloc=_empty)


@pytest.mark.parametrize("nb_neighbors", [30, 64])
def test_core_voxel_down_sample_and_stat_filter(st, nb_neighbors):
    """Segments of 0, 1, 2, 31, 400 and 1300 points: the statistical filter alone (nb_neighbors 30 and 64, the kernel's KMAX),
    and the voxel down-sample followed by it, as the engine runs the pair."""
    from oracle import penet_oracle as O
    rng = np.random.default_rng(11)
    segs = [TS._clustered_points(rng, n, 0.5, 0.1) for n in TS.STAT_SIZES]
    S = len(segs)
    enable = np.ones(S, np.int32)
    enable[3] = 0

    def alone():
        base, out, X = TS._stat_filter_run(st, segs, enable, nb_neighbors, 0.3, alloc=_empty)
        TS._stat_filter_verify(segs, enable, nb_neighbors, 0.3, base, out, X)
        return out
    both_poisons(alone)
    runs = [np.cumsum(rng.normal(0, 0.015, (n, 3)), 0) + rng.uniform(-30, 30, 3) for n in TS.STAT_SIZES]
    down = [O.voxel_down_sample(r, 0.05) for r in runs]
    P, base, cnt, cap = TS._pool_from_segments(runs)
    ones = np.ones(S, np.int32)

    def pair():
        px, py, pz = TS._t(P[:, 0]), TS._t(P[:, 1]), TS._t(P[:, 2])
        tb, tc, te = TS._t(base), TS._t(cnt), TS._t(ones)
        status = torch.zeros(1, dtype=torch.int32, device="cuda")
        st.voxel_down_sample(px, py, pz, tb, tc, te, 0.05, S, cap,
                             _empty(st.voxel_down_sample_scratch_bytes(cap), torch.uint8), status)
        torch.cuda.synchronize()
        n_down, X = tc.cpu().numpy().copy(), torch.stack([px, py, pz], 1).cpu().numpy()
        for s in range(S):
            assert n_down[s] == len(down[s]) and np.array_equal(X[base[s]:base[s] + n_down[s]], down[s]), s
        st.stat_filter(px, py, pz, tb, tc, te, nb_neighbors, 0.3, S, cap, _empty(S + 1, torch.int32),
                       _empty(cap, torch.uint8), _empty(cap, torch.float64))
        torch.cuda.synchronize()
        out, X = tc.cpu().numpy(), torch.stack([px, py, pz], 1).cpu().numpy()
        TS._stat_filter_verify(down, ones, nb_neighbors, 0.3, base, out, X)
        assert int(status.item()) == 0
        return n_down, out
    both_poisons(pair)


@pytest.mark.parametrize("R0,Rd", [(3.0, 0.001), (3.0, 0.0), (3.0, 0.05), (0.6, 0.001)])
def test_core_range_cluster(st, R0, Rd):
    cases = [c for c in TS._cluster_cases(np.random.default_rng(13)) if len(c) <= 3000]
    assert len(cases) >= 10 and max(len(c) for c in cases) == 2500

    def run():
        base, lab = TS._range_cluster_run(st, cases, R0, Rd, alloc=_empty)
        TS._range_cluster_verify(cases, R0, Rd, base, lab)
        return [lab[base[s]:base[s] + len(c)] for s, c in enumerate(cases)]
    both_poisons(run)


def test_core_lshape_fit(st):
    from dfu3d_amd.params import Params
    from oracle import penet_oracle as O
    from tests import fit_cases as F
    p = Params()
    n_theta, dtheta = p.thetas()
    segs, M, cals, classes, iscar, boxes, scores = TS._lshape_case()
    exp, _ = F.expected_rows(segs, M, classes, iscar, boxes, scores, [TS._oracle_calib(c) for c in cals], O.Params())

    def run():
        status, R = TS._lshape_fit_run(st, segs, M, cals, classes, iscar, boxes, scores, p, n_theta, dtheta, alloc=_empty)
        assert status == 0 and len(R) == len(exp)
        F.assert_rows_match(R, exp, dtheta)
        return F.sort_rows(R)                                  # the stage emits its rows in any order (the engine sorts them)
    both_poisons(run)


# ---- second passes of the one-workgroup scans, at the smallest size that takes them ----------------------------------
def test_world_aug_second_pass_of_the_chunk_scan():
    """1024 x 1024 + 1 rows in three scenes: 1025 chunks of 1024 rows, the smallest count whose scan carries into a
    second pass."""
    from tests import test_gpu_world_aug as T
    from tests import world_aug_ref as WR
    rng = np.random.default_rng(41)
    sizes = [400000, 300000, 1024 * 1024 + 1 - 700000]
    assert (sum(sizes) + 1023) // 1024 == 1025
    box = np.array([[1.0, 2.0, -1.0, 4.0, 2.0, 1.5, 0.3]], np.float32)
    ops = []
    for b, n in enumerate(sizes):
        p = np.empty((n, 4), np.float32)
        p[:, :2], p[:, 2], p[:, 3] = rng.uniform(-50, 50, (n, 2)), rng.uniform(-3, 1, n), rng.random(n)
        drawn = {'flips': [('x', b == 1), ('y', b == 2)], 'noise_rot': 0.3 - 0.25 * b, 'noise_scale': 0.95 + 0.05 * b,
                 'noise_translate': np.array([[0.5, -0.25, 0.1]], np.float32) * b}
        ops.append((p, box, np.ones(1, np.int32), drawn))
    pc_range = np.array([-40.0, -40.0, -3.0, 40.0, 40.0, 1.0], np.float32)
    want = WR.batch(ops, pc_range)
    assert want[2][-1] > 0
    both_poisons(lambda: T._run(ops, pc_range), lambda out: T._check_against_restatement(out, want, sum(sizes)))


def test_gt_sample_second_pass_of_the_slot_scan(tmp_path):
    """342 scenes of three slots each (the pasted objects and two chunks of 1024 points: one scene has 1025 points) are
    1026 slots: the scan of the slot counts carries into a second pass."""
    from dfu3d_amd.pcdet_kitti.database_sampler import DataBaseSampler
    from tests import gt_sampling_ref as GR
    from tests import test_gpu_gt_sampling as T
    rng = np.random.default_rng(23)
    boxes = [[rng.uniform(-40, 40), rng.uniform(-40, 40), -1.0, 4.0, 1.8, 1.5, rng.uniform(-3, 3)] for _ in range(40)]
    T._planted_db(tmp_path, boxes, [['Car', 'Pedestrian'][k % 2] for k in range(40)], npts=30)
    cfg = T._cfg(['Car:3', 'Pedestrian:2'], width=(0.2, 0.2, 0.0))
    scenes = []
    for s in range(342):
        n = 1025 if s == 7 else int(rng.integers(40, 200))
        p = np.zeros((n, 4), np.float32)
        p[:, :2], p[:, 2], p[:, 3] = rng.uniform(-45, 45, (n, 2)), rng.uniform(-2, 0, n), rng.random(n)
        scenes.append({'points': p, 'gt_boxes': np.zeros((0, 7), np.float32), 'gt_names': np.array([], '<U10'),
                       'gt_boxes_mask': np.ones(0, bool)})
    slots = 1 + (max(len(d['points']) for d in scenes) + 1023) // 1024
    assert slots == 3 and len(scenes) * slots > 1024
    copy = lambda: [{k: v.copy() for k, v in d.items()} for d in scenes]        # noqa: E731
    ref = GR.RefSampler(tmp_path, cfg, ['Car', 'Pedestrian'])
    np.random.seed(4)
    exp = [ref(d)[0] for d in copy()]
    assert len(exp[-1]["gt_names"]) > 0                                        # an object is pasted behind the boundary

    def run():
        smp = DataBaseSampler(tmp_path, cfg, ['Car', 'Pedestrian'], device="cuda:0")
        np.random.seed(4)
        batch = smp.sample_batch(copy())
        got = batch.split()
        for s in range(len(scenes)):
            T._same(got[s], exp[s]["points"], exp[s]["gt_boxes"], exp[s]["gt_names"], s)
        return batch.points[:int(batch.point_off[-1])]
    both_poisons(run)


def test_pillar_group_more_than_65535_pillars():
    from tests import test_gpu_pillar_vfe as T
    geo = dict(point_cloud_range=[0.0, -64.0, -3.0, 128.0, 64.0, 1.0], voxel_size=[0.25, 0.25, 4.0], grid_size=[512, 512, 1])
    pts = T.random_points(np.random.default_rng(12), 90000, 2, geo)

    def run():
        g = T.check_group(pts, 2, geo)[0]
        assert g.P > 65535
        return _group_fields(g)
    both_poisons(run)
