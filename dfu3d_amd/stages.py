"""Shape-checked Python wrappers over the C ABI (one per entry point of
include/dfu3d.h).  PyTorch is used for device memory and streams only; every
operand's dtype, device, contiguity and size is verified on the host before a
hand-written kernel is launched (a faulting kernel can reset the whole node).
"""
import ctypes
import math

import numpy as np
from dataclasses import dataclass

import torch

from . import _lib, _lib_aug, _lib_post
from ._lib import BinGeom, Dfu3dError

# Every integer macro DFU3D_<NAME> of include/dfu3d.h is <NAME> here, with the header's value (read by _header.py, never
# typed again): CALIB_FLOATS, ROW_DOUBLES, MAX_INST, TABLE_ENTRY_BYTES, MASK_BYTES, BP_*, RF_*, ST_*, STAGE_*, EVAL_MAX_DET,
# GT_SAMPLE_MAX_BOXES, CENTER_MAX_K, SELFTEST_SCRATCH_BYTES, ...
globals().update({name[len("DFU3D_"):]: value for name, value in _lib.CONSTANTS.items()})

STATUS_TEXT = {
    ST_POOL_OVERFLOW: "instance point pool too small (raise pool_cap)",
    ST_VOX_OVERFLOW: "more voxels than cap_vox in a view (raise cap_vox; bin table must be re-initialised)",
    ST_ROW_OVERFLOW: "more box rows than cap_rows",
    ST_BIN_RANGE: "a spherical bin fell outside the bin table",
    ST_VOX_PTS_OVERFLOW: "overflow-bin pixel list too small",
    ST_VOXEL_RANGE: "voxel_down_sample: a segment is wider than 2^21 voxels along an axis",
    ST_CENTER_OVERFLOW: "center_assign: more than num_max_objs boxes of one head in one sample",
}


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _chk(t, name, dtype, numel=None, min_numel=None):
    if not isinstance(t, torch.Tensor):
        raise Dfu3dError("%s: expected a torch.Tensor" % name)
    if not t.is_cuda:
        raise Dfu3dError("%s: must live on the GPU (got %s)" % (name, t.device))
    if t.dtype != dtype:
        raise Dfu3dError("%s: dtype %s, expected %s" % (name, t.dtype, dtype))
    if not t.is_contiguous():
        raise Dfu3dError("%s: must be contiguous" % name)
    if numel is not None and t.numel() != numel:
        raise Dfu3dError("%s: %d elements, expected %d" % (name, t.numel(), numel))
    if min_numel is not None and t.numel() < min_numel:
        raise Dfu3dError("%s: %d elements, need at least %d" % (name, t.numel(), min_numel))
    return ctypes.c_void_p(t.data_ptr())


def make_geom(depth_min=0.001, z_max=1.0, theta_min=1.5,
              vsize=(200.0, 0.0020000000949949026, 0.0020000000949949026),
              vrange_min=(-100.0, -5.0, -5.0), vgrid=(1, 5000, 5000),
              max_points_per_voxel=100, max_voxels=1000000):
    g = BinGeom()
    g.vsize_r, g.vsize_t, g.vsize_p = vsize
    g.rmin_r, g.rmin_t, g.rmin_p = vrange_min
    g.grid_r, g.grid_t, g.grid_p = vgrid
    g.max_points_per_voxel = int(max_points_per_voxel)
    g.max_voxels = int(max_voxels)
    g.theta_min, g.z_max, g.depth_min = theta_min, z_max, depth_min
    n = _lib.lib().dfu3d_bin_table_geometry(ctypes.byref(g))
    if n <= 0:
        raise Dfu3dError("invalid voxel geometry")
    return g, int(n)


def backproject_scratch_words(V, H, W, cap_vox, max_points, geom):
    """geom: the dfu3d_bin_geom of make_geom (its table decides the size of the segment lists)."""
    a, b = ctypes.c_int64(0), ctypes.c_int64(0)
    rc = _lib.lib().dfu3d_backproject_scratch_words(V, H, W, cap_vox, max_points, int(geom.t_n) * int(geom.p_n),
                                                    ctypes.byref(a), ctypes.byref(b))
    if rc != 0:
        raise Dfu3dError("dfu3d_backproject_scratch_words: invalid sizes")
    return a.value, b.value


def bin_table_init(table, entries_total):
    p = _chk(table, "table", torch.uint8, min_numel=entries_total * TABLE_ENTRY_BYTES)
    if table.data_ptr() % 8:
        raise Dfu3dError("table: must be 8-byte aligned")
    _lib.check(_lib.lib().dfu3d_bin_table_init(p, entries_total, _stream()), "bin_table_init")


def _check_frames(points, pt_off, view_frame, V, cap_n, host_pt_off=None, host_view_frame=None):
    """host_* are CPU copies used for bounds validation (no device sync)."""
    if points.dim() != 2 or points.shape[1] != 4:
        raise Dfu3dError("points: expected (N,4)")
    if host_pt_off is not None:
        off = [int(x) for x in host_pt_off]
        if off[0] < 0 or off[-1] > points.shape[0] or any(b < a for a, b in zip(off, off[1:])):
            raise Dfu3dError("pt_off: not a monotone partition of points")
        if max(b - a for a, b in zip(off, off[1:])) > cap_n:
            raise Dfu3dError("cap_n smaller than the largest frame")
        if host_view_frame is not None:
            vf = [int(x) for x in host_view_frame]
            if len(vf) != V or min(vf) < 0 or max(vf) >= len(off) - 1:
                raise Dfu3dError("view_frame: frame index out of range")


def fov_filter(points, pt_off, view_frame, calib, V, fov_hw, cap_n, fov_idx, n_fov,
               host_pt_off=None, host_view_frame=None):
    _check_frames(points, pt_off, view_frame, V, cap_n, host_pt_off, host_view_frame)
    rc = _lib.lib().dfu3d_fov_filter(
        _chk(points, "points", torch.float32), _chk(pt_off, "pt_off", torch.int32, min_numel=2),
        _chk(view_frame, "view_frame", torch.int32, numel=V),
        _chk(calib, "calib", torch.float32, numel=V * CALIB_FLOATS), V, int(fov_hw[0]),
        int(fov_hw[1]), cap_n, _chk(fov_idx, "fov_idx", torch.int32, numel=V * cap_n),
        _chk(n_fov, "n_fov", torch.int32, numel=V), _stream())
    _lib.check(rc, "dfu3d_fov_filter")


def plane_ransac(points, pt_off, view_frame, fov_idx, n_fov, V, cap_n, max_hs, xy_range,
                 trials, seed, key, cand_idx, plane):
    rc = _lib.lib().dfu3d_plane_ransac(
        _chk(points, "points", torch.float32), _chk(pt_off, "pt_off", torch.int32, min_numel=2),
        _chk(view_frame, "view_frame", torch.int32, numel=V),
        _chk(fov_idx, "fov_idx", torch.int32, numel=V * cap_n),
        _chk(n_fov, "n_fov", torch.int32, numel=V), V, cap_n, float(max_hs), float(xy_range),
        int(trials), ctypes.c_uint64(int(seed) & ((1 << 64) - 1)),
        _chk(key, "key", torch.int64, numel=V),
        _chk(cand_idx, "cand_idx", torch.int32, numel=V * cap_n),
        _chk(plane, "plane", torch.float64, numel=V * 4), _stream())
    _lib.check(rc, "dfu3d_plane_ransac")


def mask_word_bytes(max_inst):
    """Smallest packed mask word (bytes) that holds max_inst instance bits."""
    return 1 if max_inst <= 8 else (2 if max_inst <= 16 else 4)


_WORD_DTYPE = {1: torch.uint8, 2: torch.int16, 4: torch.int32}


def _chk_masks(masks, mask_format, V, max_inst, H, W):
    """masks: uint8 planes (V,max_inst,H,W) for MASK_BYTES, else packed words (V,H,W) of mask_format bytes."""
    if max_inst < 1 or max_inst > MAX_INST:
        raise Dfu3dError("max_inst must be in [1, %d]" % MAX_INST)
    if mask_format == MASK_BYTES:
        return _chk(masks, "masks", torch.uint8, numel=V * max_inst * H * W)
    if mask_format not in _WORD_DTYPE or mask_word_bytes(max_inst) > mask_format:
        raise Dfu3dError("mask_format %r cannot hold %d instance bits" % (mask_format, max_inst))
    if masks.data_ptr() % mask_format:
        raise Dfu3dError("masks: misaligned for %d-byte words" % mask_format)
    return _chk(masks, "masks (packed)", _WORD_DTYPE[mask_format], numel=V * H * W)


def pack_masks(masks, n_inst, V, max_inst, H, W, out=None, word_bytes=None):
    """uint8 planes (V,max_inst,H,W) -> packed words (V,H,W), bit j = plane j > 0 (dfu3d_pack_masks)."""
    wb = word_bytes or mask_word_bytes(max_inst)
    if out is None:
        out = torch.empty((V, H, W), dtype=_WORD_DTYPE[wb], device=masks.device)
    rc = _lib.lib().dfu3d_pack_masks(_chk(masks, "masks", torch.uint8, numel=V * max_inst * H * W),
                                     _chk(n_inst, "n_inst", torch.int32, numel=V), V, max_inst, H, W,
                                     _chk(out, "out", _WORD_DTYPE[wb], numel=V * H * W), wb, _stream())
    _lib.check(rc, "dfu3d_pack_masks")
    return out


def project_label(points, pt_off, view_frame, calib, plane, fov_idx, n_fov, masks, n_inst, V,
                  max_inst, H, W, cap_n, plane_offset, xy_range, ag_pt, ib_pix, n_ag, K,
                  it_bits, it_x, it_y, it_z, mask_format=MASK_BYTES, bounds_hw=None):
    """H, W: mask canvas; bounds_hw: the in-bounds test of my_loader.py:526 (default: the canvas)."""
    bh, bw = (H, W) if bounds_hw is None else (int(bounds_hw[0]), int(bounds_hw[1]))
    if bh > H or bw > W or bh < 1 or bw < 1:
        raise Dfu3dError("bounds %s must lie inside the mask canvas (%d,%d)" % ((bh, bw), H, W))
    rc = _lib.lib().dfu3d_project_label(
        _chk(points, "points", torch.float32), _chk(pt_off, "pt_off", torch.int32, min_numel=2),
        _chk(view_frame, "view_frame", torch.int32, numel=V),
        _chk(calib, "calib", torch.float32, numel=V * CALIB_FLOATS),
        _chk(plane, "plane", torch.float64, numel=V * 4),
        _chk(fov_idx, "fov_idx", torch.int32, numel=V * cap_n),
        _chk(n_fov, "n_fov", torch.int32, numel=V),
        _chk_masks(masks, mask_format, V, max_inst, H, W), int(mask_format),
        _chk(n_inst, "n_inst", torch.int32, numel=V), V, max_inst, H, W, bh, bw, cap_n,
        float(plane_offset), float(xy_range),
        _chk(ag_pt, "ag_pt", torch.int32, numel=V * cap_n),
        _chk(ib_pix, "ib_pix", torch.int32, numel=V * cap_n),
        _chk(n_ag, "n_ag", torch.int32, numel=V), _chk(K, "K", torch.int32, numel=V),
        _chk(it_bits, "it_bits", torch.int32, numel=V * cap_n),
        _chk(it_x, "it_x", torch.float64, numel=V * cap_n),
        _chk(it_y, "it_y", torch.float64, numel=V * cap_n),
        _chk(it_z, "it_z", torch.float64, numel=V * cap_n), _stream())
    _lib.check(rc, "dfu3d_project_label")


def backproject_bin(depth, calib, masks, n_inst, V, max_inst, H, W, geom, table_entries,
                    key_axis, table, pix_bin, blk_cnt, cap_vox, n_vox, vox_pix, it_bits, it_x,
                    it_y, it_z, status, phases=BP_ALL, mask_format=MASK_BYTES):
    pw, bw = backproject_scratch_words(V, H, W, cap_vox, geom.max_points_per_voxel, geom)
    if table.data_ptr() % 8 or blk_cnt.data_ptr() % 8:
        raise Dfu3dError("table / blk_cnt: must be 8-byte aligned")
    if depth.data_ptr() % 16:
        raise Dfu3dError("depth: must be 16-byte aligned")
    if W % 4:
        raise Dfu3dError("W must be a multiple of 4 (float4 depth loads)")
    mp = _chk_masks(masks, mask_format, V, max_inst, H, W) if masks is not None else None
    ni = _chk(n_inst, "n_inst", torch.int32, numel=V) if n_inst is not None else None
    rc = _lib.lib().dfu3d_backproject_bin(
        _chk(depth, "depth", torch.float32, numel=V * H * W),
        _chk(calib, "calib", torch.float32, numel=V * CALIB_FLOATS), mp, int(mask_format), ni, V, max_inst, H, W,
        ctypes.byref(geom), int(key_axis),
        _chk(table, "table", torch.uint8, min_numel=V * table_entries * TABLE_ENTRY_BYTES),
        _chk(pix_bin, "pix_bin", torch.int32, min_numel=pw),
        _chk(blk_cnt, "blk_cnt", torch.int32, min_numel=bw), cap_vox,
        _chk(n_vox, "n_vox", torch.int32, numel=V),
        _chk(vox_pix, "vox_pix", torch.int32, numel=V * cap_vox),
        _chk(it_bits, "it_bits", torch.int32, numel=V * cap_vox),
        _chk(it_x, "it_x", torch.float64, numel=V * cap_vox),
        _chk(it_y, "it_y", torch.float64, numel=V * cap_vox),
        _chk(it_z, "it_z", torch.float64, numel=V * cap_vox),
        _chk(status, "status", torch.int32, min_numel=1), int(phases), _stream())
    _lib.check(rc, "dfu3d_backproject_bin")


def shadow_floats(pool_cap):
    """float32 elements of the radius filter's shadow scratch (dfu3d_rf_shadow_bytes / 4)."""
    n = int(_lib.lib().dfu3d_rf_shadow_bytes(int(pool_cap)))
    if n < 0:
        raise Dfu3dError("dfu3d_rf_shadow_bytes: invalid pool_cap %r" % (pool_cap,))
    return n // 4


def rf_queue_ints(pool_cap):
    """int32 elements of the radius filter's queue scratch (dfu3d_rf_queue_ints)."""
    n = int(_lib.lib().dfu3d_rf_queue_ints(int(pool_cap)))
    if n < 0:
        raise Dfu3dError("dfu3d_rf_queue_ints: invalid pool_cap %r" % (pool_cap,))
    return n


def segments_build(a_bits, a_x, a_y, a_z, a_n, a_cap, b_bits, b_x, b_y, b_z, b_n, b_cap, V,
                   max_inst, pool_cap, pool_cursor, px, py, pz, base_a, cnt_a, base_b, cnt_b,
                   status, rad_a=None, rad_b=None, shadow=None, base_ab=None, cnt_ab=None, rad_ab=None, chunk_cnt=None):
    """rad_a / rad_b + shadow (+ the joint 2S segment table): everything the one-pass radius filter needs."""
    S = V * max_inst
    nw = int(_lib.lib().dfu3d_segments_scratch_words(V, a_cap, b_cap))
    if chunk_cnt is None:
        chunk_cnt = torch.empty(nw, dtype=torch.int32, device=px.device)
    opt = lambda t, name, dt, n: None if t is None else _chk(t, name, dt, numel=n)
    if shadow is not None and shadow.data_ptr() % 16:
        raise Dfu3dError("shadow: must be 16-byte aligned")
    rc = _lib.lib().dfu3d_segments_build(
        _chk(a_bits, "a_bits", torch.int32, numel=V * a_cap),
        _chk(a_x, "a_x", torch.float64, numel=V * a_cap),
        _chk(a_y, "a_y", torch.float64, numel=V * a_cap),
        _chk(a_z, "a_z", torch.float64, numel=V * a_cap), _chk(a_n, "a_n", torch.int32, numel=V),
        a_cap, _chk(b_bits, "b_bits", torch.int32, numel=V * b_cap),
        _chk(b_x, "b_x", torch.float64, numel=V * b_cap),
        _chk(b_y, "b_y", torch.float64, numel=V * b_cap),
        _chk(b_z, "b_z", torch.float64, numel=V * b_cap), _chk(b_n, "b_n", torch.int32, numel=V),
        b_cap, V, max_inst, pool_cap, _chk(pool_cursor, "pool_cursor", torch.int64, numel=1),
        _chk(px, "px", torch.float64, numel=pool_cap), _chk(py, "py", torch.float64, numel=pool_cap),
        _chk(pz, "pz", torch.float64, numel=pool_cap),
        _chk(base_a, "base_a", torch.int64, numel=S), _chk(cnt_a, "cnt_a", torch.int32, numel=S),
        _chk(base_b, "base_b", torch.int64, numel=S), _chk(cnt_b, "cnt_b", torch.int32, numel=S),
        _chk(status, "status", torch.int32, min_numel=1),
        opt(rad_a, "rad_a", torch.float64, S), opt(rad_b, "rad_b", torch.float64, S),
        opt(shadow, "shadow", torch.float32, shadow_floats(pool_cap)), opt(base_ab, "base_ab", torch.int64, 2 * S),
        opt(cnt_ab, "cnt_ab", torch.int32, 2 * S), opt(rad_ab, "rad_ab", torch.float64, 2 * S),
        _chk(chunk_cnt, "chunk_cnt", torch.int32, min_numel=nw), _stream())
    _lib.check(rc, "dfu3d_segments_build")


def radius_filter(px, py, pz, seg_base, seg_cnt, radius, nb_points, S, pool_cap, tile_off, flags,
                  queue, phases=RF_ALL, shadow=None, n_used=None):
    """shadow: float32 (4*pool_cap) scratch (allocated here when omitted); n_used: device int64 (1,) or None."""
    if shadow is None:
        shadow = torch.empty(shadow_floats(pool_cap), dtype=torch.float32, device=px.device)
    if shadow.data_ptr() % 16:
        raise Dfu3dError("shadow: must be 16-byte aligned")
    rc = _lib.lib().dfu3d_radius_filter(
        _chk(px, "px", torch.float64, numel=pool_cap), _chk(py, "py", torch.float64, numel=pool_cap),
        _chk(pz, "pz", torch.float64, numel=pool_cap),
        _chk(seg_base, "seg_base", torch.int64, numel=S),
        _chk(seg_cnt, "seg_cnt", torch.int32, numel=S),
        _chk(radius, "radius", torch.float64, numel=S), int(nb_points), S, pool_cap,
        None if n_used is None else _chk(n_used, "n_used", torch.int64, numel=1),
        _chk(shadow, "shadow", torch.float32, numel=shadow_floats(pool_cap)),
        _chk(tile_off, "tile_off", torch.int32, min_numel=S + 1),
        _chk(flags, "flags", torch.uint8, numel=pool_cap),
        _chk(queue, "queue", torch.int32, min_numel=rf_queue_ints(pool_cap)), int(phases), _stream())
    _lib.check(rc, "dfu3d_radius_filter")


def voxel_down_sample_scratch_bytes(pool_cap):
    return int(_lib.lib().dfu3d_voxel_down_sample_scratch_bytes(int(pool_cap)))


def voxel_down_sample(px, py, pz, seg_base, seg_cnt, enable, voxel_size, S, pool_cap, scratch, status):
    """Open3D voxel_down_sample per enabled segment, in place, centroids in first-seen voxel order (include/dfu3d.h)."""
    rc = _lib.lib().dfu3d_voxel_down_sample(
        _chk(px, "px", torch.float64, numel=pool_cap), _chk(py, "py", torch.float64, numel=pool_cap),
        _chk(pz, "pz", torch.float64, numel=pool_cap), _chk(seg_base, "seg_base", torch.int64, numel=S),
        _chk(seg_cnt, "seg_cnt", torch.int32, numel=S), _chk(enable, "enable", torch.int32, numel=S),
        float(voxel_size), S, pool_cap,
        _chk(scratch, "scratch", torch.uint8, min_numel=voxel_down_sample_scratch_bytes(pool_cap)),
        _chk(status, "status", torch.int32, min_numel=1), _stream())
    _lib.check(rc, "dfu3d_voxel_down_sample")


def stat_filter(px, py, pz, seg_base, seg_cnt, enable, nb_neighbors, std_ratio, S, pool_cap,
                tile_off, flags, mean_d):
    rc = _lib.lib().dfu3d_stat_filter(
        _chk(px, "px", torch.float64, numel=pool_cap), _chk(py, "py", torch.float64, numel=pool_cap),
        _chk(pz, "pz", torch.float64, numel=pool_cap),
        _chk(seg_base, "seg_base", torch.int64, numel=S),
        _chk(seg_cnt, "seg_cnt", torch.int32, numel=S),
        _chk(enable, "enable", torch.int32, numel=S), int(nb_neighbors), float(std_ratio), S,
        pool_cap, _chk(tile_off, "tile_off", torch.int32, min_numel=S + 1),
        _chk(flags, "flags", torch.uint8, numel=pool_cap),
        _chk(mean_d, "mean_d", torch.float64, numel=pool_cap), None, _stream())
    _lib.check(rc, "dfu3d_stat_filter")


def ballquery_fuse(px, py, pz, base_a, cnt_a, base_b, cnt_b, C, S, pool_cap, tile_off, flags, masked=False):
    """masked=True: `flags` holds the keep mask of a radius_filter call over the B lists made without RF_COMPACT;
    masked="joint": of a joint call over the A and B lists (cnt_a is updated: A is compacted here too)."""
    L = _lib.lib()
    fn = L.dfu3d_ballquery_fuse_joint if masked == "joint" else (L.dfu3d_ballquery_fuse_masked if masked else L.dfu3d_ballquery_fuse)
    rc = fn(
        _chk(px, "px", torch.float64, numel=pool_cap), _chk(py, "py", torch.float64, numel=pool_cap),
        _chk(pz, "pz", torch.float64, numel=pool_cap),
        _chk(base_a, "base_a", torch.int64, numel=S), _chk(cnt_a, "cnt_a", torch.int32, numel=S),
        _chk(base_b, "base_b", torch.int64, numel=S), _chk(cnt_b, "cnt_b", torch.int32, numel=S),
        float(C), S, pool_cap, _chk(tile_off, "tile_off", torch.int32, min_numel=2 * S + 2),
        _chk(flags, "flags", torch.uint8, numel=pool_cap), _stream())
    _lib.check(rc, "dfu3d_ballquery_fuse")


def points_in_boxes_mask(points, boxes):
    """points (n,3|4) float32 CUDA, boxes (B,7) float64 CUDA -> int32 (B,n)
    (roiaware_pool3d_utils.points_in_boxes_cpu, pcdet/ops/roiaware_pool3d/roiaware_pool3d_utils.py:9-25)."""
    if points.dim() != 2 or points.shape[1] not in (3, 4) or boxes.dim() != 2 or boxes.shape[1] != 7:
        raise Dfu3dError("points must be (n,3|4), boxes (B,7)")
    n, B = int(points.shape[0]), int(boxes.shape[0])
    out = torch.zeros((B, n), dtype=torch.int32, device=points.device)
    rc = _lib.lib().dfu3d_points_in_boxes_mask(
        _chk(points, "points", torch.float32, numel=n * points.shape[1]), n, int(points.shape[1]),
        _chk(boxes, "boxes", torch.float64, numel=B * 7), B, _chk(out, "out", torch.int32, numel=B * n),
        _stream())
    _lib.check(rc, "dfu3d_points_in_boxes_mask")
    return out


def gt_database(points, pt_off, box_frame, boxes, cap_out, host_pt_off=None):
    """Many frames at once -> (box_cnt (Bt,), box_off (Bt+1,), idx (cap_out,), gt_pts (cap_out,4), status)."""
    Bt = int(boxes.shape[0])
    dev = points.device
    if Bt == 0:
        raise Dfu3dError("no boxes")
    if points.dim() != 2 or points.shape[1] != 4:
        raise Dfu3dError("points must be (N,4) float32")
    if host_pt_off is not None:
        hp = np.asarray(host_pt_off)
        if hp[0] != 0 or np.any(np.diff(hp) < 0) or hp[-1] > points.shape[0]:
            raise Dfu3dError("pt_off must be non-decreasing within the point tensor")
    cnt = torch.zeros(Bt, dtype=torch.int32, device=dev)
    off = torch.zeros(Bt + 1, dtype=torch.int64, device=dev)
    idx = torch.empty(cap_out, dtype=torch.int32, device=dev)
    gt = torch.empty((cap_out, 4), dtype=torch.float32, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    rc = _lib.lib().dfu3d_gt_database(
        _chk(points, "points", torch.float32, numel=points.shape[0] * 4),
        _chk(pt_off, "pt_off", torch.int32, min_numel=2),
        _chk(box_frame, "box_frame", torch.int32, numel=Bt),
        _chk(boxes, "boxes", torch.float64, numel=Bt * 7), Bt,
        _chk(cnt, "cnt", torch.int32, numel=Bt), _chk(off, "off", torch.int64, numel=Bt + 1), int(cap_out),
        _chk(idx, "idx", torch.int32, numel=cap_out), _chk(gt, "gt", torch.float32, numel=cap_out * 4),
        _chk(status, "status", torch.int32, numel=1), _stream())
    _lib.check(rc, "dfu3d_gt_database")
    return cnt, off, idx, gt, status


def boxes_bev(boxes_a, boxes_b, iou=True):
    """(N,7),(M,7) float32 CUDA -> (N,M) float32 BEV IoU (iou=True) or overlap area."""
    n, m = int(boxes_a.shape[0]), int(boxes_b.shape[0])
    out = torch.zeros((n, m), dtype=torch.float32, device=boxes_a.device)
    if n == 0 or m == 0:
        return out
    rc = _lib.lib().dfu3d_boxes_bev(_chk(boxes_a, "boxes_a", torch.float32, numel=n * 7), n,
                                    _chk(boxes_b, "boxes_b", torch.float32, numel=m * 7), m,
                                    _chk(out, "out", torch.float32, numel=n * m), 1 if iou else 0, _stream())
    _lib.check(rc, "dfu3d_boxes_bev")
    return out


def boxes_bev_paired(boxes_a, boxes_b, iou=True):
    """(N,7),(N,7) -> (N,) overlap area / BEV IoU of row i with row i."""
    n = int(boxes_a.shape[0])
    if int(boxes_b.shape[0]) != n:
        raise Dfu3dError("paired overlap needs as many boxes on both sides")
    out = torch.zeros((n,), dtype=torch.float32, device=boxes_a.device)
    if n:
        rc = _lib.lib().dfu3d_boxes_bev_paired(_chk(boxes_a, "boxes_a", torch.float32, numel=n * 7),
                                               _chk(boxes_b, "boxes_b", torch.float32, numel=n * 7), n,
                                               _chk(out, "out", torch.float32, numel=n), 1 if iou else 0, _stream())
        _lib.check(rc, "dfu3d_boxes_bev_paired")
    return out


def rotate_iou_eval(boxes, query_boxes, criterion=-1):
    """(N,5),(K,5) float32 CUDA [cx cy w h angle] -> (N,K): the AP evaluator's rotated IoU (dfu3d_rotate_iou_eval)."""
    n, k = int(boxes.shape[0]), int(query_boxes.shape[0])
    out = torch.zeros((n, k), dtype=torch.float32, device=boxes.device)
    if n and k:
        rc = _lib.lib().dfu3d_rotate_iou_eval(_chk(boxes, "boxes", torch.float32, numel=n * 5), n,
                                              _chk(query_boxes, "query_boxes", torch.float32, numel=k * 5), k,
                                              _chk(out, "out", torch.float32, numel=n * k), int(criterion), _stream())
        _lib.check(rc, "dfu3d_rotate_iou_eval")
    return out


class EvalFrames:
    """All frames of an evaluation as flat CUDA tensors (see include/dfu3d.h, "f-3, AP evaluation"): offsets int64
    (F+1), per-box float64 bbox (.,4), cam (.,7), alpha, score, truncated and int32 code, dontcare, occluded."""

    FIELDS_GT = ("gt_code", "gt_dontcare", "gt_bbox", "gt_alpha", "gt_occluded", "gt_truncated")
    FIELDS_DT = ("dt_code", "dt_bbox", "dt_alpha", "dt_score")

    def __init__(self, **t):
        self.__dict__.update(t)
        self.F = int(self.gt_off.numel()) - 1
        self.n_gt, self.n_dt = int(self.gt_code.numel()), int(self.dt_code.numel())

    def _box_args(self):
        G, D = self.n_gt, self.n_dt
        f64, i32 = torch.float64, torch.int32
        return [_chk(self.gt_code, "gt_code", i32, numel=G), _chk(self.gt_dontcare, "gt_dontcare", i32, numel=G),
                _chk(self.gt_bbox, "gt_bbox", f64, numel=4 * G), _chk(self.gt_alpha, "gt_alpha", f64, numel=G),
                _chk(self.gt_occluded, "gt_occluded", i32, numel=G), _chk(self.gt_truncated, "gt_truncated", f64, numel=G),
                _chk(self.dt_code, "dt_code", i32, numel=D), _chk(self.dt_bbox, "dt_bbox", f64, numel=4 * D),
                _chk(self.dt_alpha, "dt_alpha", f64, numel=D), _chk(self.dt_score, "dt_score", f64, numel=D)]

    def _off_args(self):
        F = self.F
        return [_chk(self.gt_off, "gt_off", torch.int64, numel=F + 1), _chk(self.dt_off, "dt_off", torch.int64, numel=F + 1),
                _chk(self.ov_off, "ov_off", torch.int64, numel=F + 1)]


def eval_overlaps(fr: EvalFrames, metric):
    """-> float64 (n_pairs): overlap of detection j with ground truth i of frame f at ov_off[f] + i * D_f + j."""
    ov = torch.zeros(max(fr.n_pairs, 1), dtype=torch.float64, device=fr.gt_off.device)
    if fr.n_pairs:
        rc = _lib.lib().dfu3d_eval_overlaps(
            int(metric), fr.F, *fr._off_args(), _chk(fr.gt_bbox, "gt_bbox", torch.float64, numel=4 * fr.n_gt),
            _chk(fr.dt_bbox, "dt_bbox", torch.float64, numel=4 * fr.n_dt),
            _chk(fr.gt_cam, "gt_cam", torch.float64, numel=7 * fr.n_gt),
            _chk(fr.dt_cam, "dt_cam", torch.float64, numel=7 * fr.n_dt), _chk(ov, "ov", torch.float64, numel=fr.n_pairs),
            fr.n_pairs, _stream())
        _lib.check(rc, "dfu3d_eval_overlaps")
    return ov


def _combo_tensor(combos, device):
    """[(class index, difficulty, min_overlap)] -> the dfu3d_eval_combo array as a CUDA byte tensor."""
    arr = (_lib.EvalCombo * len(combos))()
    for k, (c, d, mo) in enumerate(combos):
        if int(d) < 0:
            raise Dfu3dError("difficulty must be >= 0")
        arr[k].cls, arr[k].difficulty, arr[k].min_overlap = int(c), int(d), float(mo)
    host = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8)
    return host.to(device)


_COMBO_P = ctypes.POINTER(_lib.EvalCombo)     # the header's type of `combos`; what is passed is a DEVICE array, hence the casts


def eval_match_scores(fr: EvalFrames, ov, metric, combos):
    """First pass of eval_class for every cell of `combos` -> (matched float64 (n_combo, n_gt) NaN-padded per frame,
    n_valid int32 (n_combo, F))."""
    dev = fr.gt_off.device
    C = len(combos)
    matched = torch.full((C, max(fr.n_gt, 1)), float("nan"), dtype=torch.float64, device=dev)
    n_valid = torch.zeros((C, fr.F), dtype=torch.int32, device=dev)
    cb = _combo_tensor(combos, dev)
    rc = _lib.lib().dfu3d_eval_match_scores(
        int(metric), fr.F, fr.max_dt, *fr._off_args(), _chk(ov, "ov", torch.float64, min_numel=max(fr.n_pairs, 1)),
        *fr._box_args(), ctypes.cast(_chk(cb, "combos", torch.uint8, numel=ctypes.sizeof(_lib.EvalCombo) * C), _COMBO_P), C, fr.n_gt,
        _chk(matched, "matched", torch.float64, min_numel=C * fr.n_gt), _chk(n_valid, "n_valid", torch.int32, numel=C * fr.F),
        _stream())
    _lib.check(rc, "dfu3d_eval_match_scores")
    return matched[:, :fr.n_gt], n_valid


def eval_match_stats(fr: EvalFrames, ov, metric, combos, thresholds, n_thresh, compute_aos=False):
    """Second pass: thresholds float64 (n_combo, T), n_thresh int32 (n_combo) -> (pr int64 (n_combo, T, 3) = tp, fp, fn
    over all frames, sim float64 (n_combo, F, T) or None)."""
    dev = fr.gt_off.device
    C, T = int(thresholds.shape[0]), int(thresholds.shape[1])
    if C != len(combos) or T < 1:
        raise Dfu3dError("thresholds must be (n_combo, T >= 1)")
    pr = torch.zeros((C, T, 3), dtype=torch.int64, device=dev)
    sim = torch.zeros((C, fr.F, T), dtype=torch.float64, device=dev) if compute_aos else None
    cb = _combo_tensor(combos, dev)
    rc = _lib.lib().dfu3d_eval_match_stats(
        int(metric), fr.F, fr.max_dt, *fr._off_args(), _chk(ov, "ov", torch.float64, min_numel=max(fr.n_pairs, 1)),
        *fr._box_args(), ctypes.cast(_chk(cb, "combos", torch.uint8, numel=ctypes.sizeof(_lib.EvalCombo) * C), _COMBO_P), C,
        _chk(thresholds, "thresholds", torch.float64, numel=C * T), _chk(n_thresh, "n_thresh", torch.int32, numel=C), T,
        1 if compute_aos else 0, _chk(pr, "pr", torch.int64, numel=C * T * 3),
        _chk(sim, "sim", torch.float64, numel=C * fr.F * T) if compute_aos else None, _stream())
    _lib.check(rc, "dfu3d_eval_match_stats")
    return pr, sim


def nms_bev(boxes, thresh, normal=False):
    """boxes (N,7) float32 CUDA sorted by descending score -> (keep int64 (N,), number kept)."""
    n = int(boxes.shape[0])
    dev = boxes.device
    keep = torch.zeros(max(n, 1), dtype=torch.int64, device=dev)
    if n == 0:
        return keep[:0], 0
    num = torch.zeros(1, dtype=torch.int32, device=dev)
    mask = torch.empty(max(n * ((n + 63) // 64), 1), dtype=torch.int64, device=dev)
    fn = _lib.lib().dfu3d_nms_normal_bev if normal else _lib.lib().dfu3d_nms_bev
    rc = fn(_chk(boxes, "boxes", torch.float32, numel=n * 7), n, ctypes.c_float(thresh),
            _chk(mask, "mask", torch.int64, min_numel=1), _chk(keep, "keep", torch.int64, min_numel=1),
            _chk(num, "num_keep", torch.int32, numel=1), _stream())
    _lib.check(rc, "dfu3d_nms_bev")
    return keep, int(num.item())


def selftest_classify(calib_record, H, W, geom, key_axis, n, seed=1, d_lo=0.5, d_hi=120.0, device="cuda:0"):
    """Float32 tier of the bin classification against the fp64 one on n random pixels under one calibration record
    and the BinGeom `geom` -> dict(tried, undecided, wrong, kept); `wrong` must be 0 (dfu3d_selftest_classify)."""
    cal = torch.as_tensor(np.asarray(calib_record, np.float32).reshape(CALIB_FLOATS)).to(device).contiguous()
    scratch = torch.zeros(SELFTEST_SCRATCH_BYTES // 4, dtype=torch.float32, device=device)
    out = torch.zeros(4, dtype=torch.int64, device=device)
    rc = _lib.lib().dfu3d_selftest_classify(_chk(cal, "calib", torch.float32, numel=CALIB_FLOATS), int(H), int(W),
                                            ctypes.byref(geom), int(key_axis), int(n), int(seed), float(d_lo),
                                            float(d_hi), _chk(scratch, "scratch", torch.float32),
                                            _chk(out, "out", torch.int64, numel=4), _stream())
    _lib.check(rc, "dfu3d_selftest_classify")
    t, u, w, k = out.cpu().tolist()
    return {"tried": t, "undecided": u, "wrong": w, "kept": k}


def selftest_backproject(calib_record, H, W, n, seed=1, d_lo=0.5, d_hi=120.0, device="cuda:0"):
    """-> max |float32 back-projection - fp64| / bound over n random pixels under one 48-float calibration record."""
    cal = torch.as_tensor(np.asarray(calib_record, np.float32).reshape(CALIB_FLOATS)).to(device).contiguous()
    scratch = torch.zeros(32, dtype=torch.float32, device=device)
    out = torch.zeros(1, dtype=torch.float64, device=device)
    rc = _lib.lib().dfu3d_selftest_backproject(_chk(cal, "calib", torch.float32, numel=CALIB_FLOATS), int(H), int(W),
                                               int(n), int(seed), float(d_lo), float(d_hi),
                                               _chk(scratch, "scratch", torch.float32, numel=32),
                                               _chk(out, "out", torch.float64, numel=1), _stream())
    _lib.check(rc, "dfu3d_selftest_backproject")
    return float(out.item())


def range_cluster(px, py, seg_base, seg_cnt, S, R0, Rd, label, pool_cap, sx=None, sy=None, si=None):
    dev = px.device
    sx = sx if sx is not None else torch.empty(pool_cap, dtype=torch.float64, device=dev)
    sy = sy if sy is not None else torch.empty(pool_cap, dtype=torch.float64, device=dev)
    si = si if si is not None else torch.empty(3 * pool_cap, dtype=torch.int32, device=dev)
    rc = _lib.lib().dfu3d_range_cluster(
        _chk(px, "px", torch.float64, numel=pool_cap), _chk(py, "py", torch.float64, numel=pool_cap),
        _chk(seg_base, "seg_base", torch.int64, numel=S),
        _chk(seg_cnt, "seg_cnt", torch.int32, numel=S), S, float(R0), float(Rd),
        _chk(label, "label", torch.int32, numel=pool_cap),
        _chk(sx, "sx", torch.float64, numel=pool_cap), _chk(sy, "sy", torch.float64, numel=pool_cap),
        _chk(si, "si", torch.int32, numel=3 * pool_cap), pool_cap, _stream())
    _lib.check(rc, "dfu3d_range_cluster")


def lshape_fit(px, py, pz, label, seg_base, seg_cnt, S, max_inst, calib, inst_class,
               inst_is_car, inst_box, inst_score, n_theta, dtheta, car_aspect_max, sx, sy,
               sroot, cap_rows, rows, n_rows, status, pool_cap, fit_ws=None):
    nws = int(_lib.lib().dfu3d_lshape_fit_ws_doubles(pool_cap, cap_rows))
    if fit_ws is None:
        fit_ws = torch.empty(nws, dtype=torch.float64, device=px.device)
    if S % max_inst:
        raise Dfu3dError("S must be V*max_inst")
    V = S // max_inst
    rc = _lib.lib().dfu3d_lshape_fit(
        _chk(px, "px", torch.float64, numel=pool_cap), _chk(py, "py", torch.float64, numel=pool_cap),
        _chk(pz, "pz", torch.float64, numel=pool_cap),
        _chk(label, "label", torch.int32, numel=pool_cap),
        _chk(seg_base, "seg_base", torch.int64, numel=S),
        _chk(seg_cnt, "seg_cnt", torch.int32, numel=S), S, max_inst,
        _chk(calib, "calib", torch.float32, numel=V * CALIB_FLOATS),
        _chk(inst_class, "inst_class", torch.int32, numel=S),
        _chk(inst_is_car, "inst_is_car", torch.int32, numel=S),
        _chk(inst_box, "inst_box", torch.float32, numel=S * 4),
        _chk(inst_score, "inst_score", torch.float32, numel=S), int(n_theta), float(dtheta),
        float(car_aspect_max), _chk(sx, "sx", torch.float64, numel=pool_cap),
        _chk(sy, "sy", torch.float64, numel=pool_cap),
        _chk(sroot, "sroot", torch.int32, numel=pool_cap), cap_rows,
        _chk(rows, "rows", torch.float64, numel=cap_rows * ROW_DOUBLES),
        _chk(n_rows, "n_rows", torch.int32, numel=1),
        _chk(status, "status", torch.int32, min_numel=1),
        _chk(fit_ws, "fit_ws", torch.float64, min_numel=nws), pool_cap, _stream())
    _lib.check(rc, "dfu3d_lshape_fit")


def status_message(word):
    return "; ".join(t for b, t in STATUS_TEXT.items() if word & b) or "ok"


def gt_sample_collide(boxes, box_off, gt_cnt, grp, gt_mask, max_boxes, status):
    """Ground-truth sampling, collision step (dfu3d_gt_sample_collide).  boxes float64 (Nt,7), box_off int32 (B+1),
    gt_cnt int32 (B), grp / gt_mask int32 (Nt) -> accept int32 (Nt), out_boxes float64 (Nt,7), out_src int32 (Nt),
    out_cnt int32 (B)."""
    nt, B = int(boxes.shape[0]), int(gt_cnt.shape[0])
    if max_boxes > GT_SAMPLE_MAX_BOXES:
        raise Dfu3dError("gt_sample: a scene has %d boxes (ground truths + candidates), at most %d"
                         % (max_boxes, GT_SAMPLE_MAX_BOXES))
    dev = boxes.device
    n1 = max(nt, 1)                    # never a null pointer for an empty batch of boxes
    accept = torch.zeros(n1, dtype=torch.int32, device=dev)
    out_boxes = torch.zeros((n1, 7), dtype=torch.float64, device=dev)
    out_src = torch.zeros(n1, dtype=torch.int32, device=dev)
    out_cnt = torch.zeros(max(B, 1), dtype=torch.int32, device=dev)
    if nt == 0:
        boxes = torch.zeros((1, 7), dtype=torch.float64, device=dev)
        grp = torch.zeros(1, dtype=torch.int32, device=dev)
        gt_mask = torch.zeros(1, dtype=torch.int32, device=dev)
    rc = _lib.lib().dfu3d_gt_sample_collide(
        _chk(boxes, "boxes", torch.float64, numel=n1 * 7), _chk(box_off, "box_off", torch.int32, numel=B + 1),
        _chk(gt_cnt, "gt_cnt", torch.int32, numel=B), _chk(grp, "grp", torch.int32, numel=n1),
        _chk(gt_mask, "gt_mask", torch.int32, numel=n1), B, int(max_boxes),
        _chk(accept, "accept", torch.int32, numel=n1), _chk(out_boxes, "out_boxes", torch.float64, numel=n1 * 7),
        _chk(out_src, "out_src", torch.int32, numel=n1), _chk(out_cnt, "out_cnt", torch.int32, min_numel=B),
        _chk(status, "status", torch.int32, numel=1), _stream())
    _lib.check(rc, "dfu3d_gt_sample_collide")
    return accept[:nt], out_boxes[:nt], out_src[:nt], out_cnt[:B]


def gt_sample_paste_scratch_bytes(B, max_scene_points):
    n = int(_lib.lib().dfu3d_gt_sample_paste_scratch_bytes(int(B), int(max_scene_points)))
    if n < 0:
        raise Dfu3dError("gt_sample_paste_scratch_bytes: impossible sizes")
    return n


def gt_sample_paste(points, pt_off, max_scene_points, box_off, gt_cnt, boxes, large, accept, pool, obj_src, obj_cnt,
                    cap_out, status):
    """Ground-truth sampling, point step (dfu3d_gt_sample_paste).  points float32 (N,C) by scene (pt_off int64 (B+1)),
    pool float32 (P,C); per box row: boxes / large float64 (Nt,7), accept / obj_cnt int32, obj_src int64 ->
    out float32 (cap_out,C), out_off int64 (B+1) (dense CSR)."""
    B = int(gt_cnt.shape[0])
    C = int(points.shape[1])
    dev = points.device
    nt = int(boxes.shape[0])
    if nt == 0:                        # every per-row operand non-null
        boxes = large = torch.zeros((1, 7), dtype=torch.float64, device=dev)
        accept = obj_cnt = torch.zeros(1, dtype=torch.int32, device=dev)
        obj_src = torch.zeros(1, dtype=torch.int64, device=dev)
    n1 = max(nt, 1)
    if pool is not None and (pool.dim() != 2 or int(pool.shape[1]) != C):
        raise Dfu3dError("gt_sample_paste: pool must be (P, %d)" % C)
    out = torch.empty((max(int(cap_out), 1), C), dtype=torch.float32, device=dev)
    out_off = torch.zeros(B + 1, dtype=torch.int64, device=dev)
    scratch = torch.empty((gt_sample_paste_scratch_bytes(B, max_scene_points) + 7) // 8, dtype=torch.int64,
                          device=dev)
    pool_p = None if pool is None or pool.numel() == 0 else _chk(pool, "pool", torch.float32)
    rc = _lib.lib().dfu3d_gt_sample_paste(
        _chk(points, "points", torch.float32, numel=int(points.shape[0]) * C), C,
        _chk(pt_off, "pt_off", torch.int64, numel=B + 1), B, int(max_scene_points),
        _chk(box_off, "box_off", torch.int32, numel=B + 1), _chk(gt_cnt, "gt_cnt", torch.int32, numel=B),
        _chk(boxes, "boxes", torch.float64, numel=n1 * 7), _chk(large, "large", torch.float64, numel=n1 * 7),
        _chk(accept, "accept", torch.int32, numel=n1), pool_p, _chk(obj_src, "obj_src", torch.int64, numel=n1),
        _chk(obj_cnt, "obj_cnt", torch.int32, numel=n1), _chk(out, "out", torch.float32, numel=out.shape[0] * C),
        _chk(out_off, "out_off", torch.int64, numel=B + 1), int(cap_out), ctypes.c_void_p(scratch.data_ptr()),
        _chk(status, "status", torch.int32, numel=1), _stream())
    _lib.check(rc, "dfu3d_gt_sample_paste")
    return out, out_off


def center_assign(gt_boxes, cls_tab, head_plane, n_cls, n_heads, W, H, range_xy, voxel_xy, stride, num_max_objs,
                  gaussian_overlap, min_radius, status):
    """CenterHead target assignment for all heads and samples (dfu3d_center_assign).  gt_boxes float32 (B,M,C) ->
    heat float32 (B * n_cls * H * W, head-major), target_boxes / target_boxes_src float32 (n_heads,B,num_max_objs,C),
    inds / masks int64 (n_heads,B,num_max_objs).  Nothing here synchronises or copies to the host."""
    if gt_boxes.dim() != 3 or gt_boxes.shape[2] < 8:
        raise Dfu3dError("center_assign: gt_boxes must be (B, M, C >= 8), got %s" % (tuple(gt_boxes.shape),))
    B, M, C = (int(v) for v in gt_boxes.shape)
    dev = gt_boxes.device
    heat = torch.empty(max(B * n_cls * H * W, 1), dtype=torch.float32, device=dev)
    tgt = torch.empty((n_heads, B, num_max_objs, C), dtype=torch.float32, device=dev)
    src = torch.empty((n_heads, B, num_max_objs, C), dtype=torch.float32, device=dev)
    inds = torch.empty((n_heads, B, num_max_objs), dtype=torch.int64, device=dev)
    masks = torch.empty((n_heads, B, num_max_objs), dtype=torch.int64, device=dev)
    if B == 0:
        return heat[:0], tgt, inds, masks, src
    gt_p = _chk(gt_boxes, "gt_boxes", torch.float32) if B * M else None
    rc = _lib.lib().dfu3d_center_assign(
        gt_p, B, M, C, _chk(cls_tab, "cls_tab", torch.int32, numel=2 * (n_cls + 1)), int(n_cls),
        _chk(head_plane, "head_plane", torch.int32, numel=n_heads + 1), int(n_heads), int(W), int(H),
        float(range_xy[0]), float(range_xy[1]), float(voxel_xy[0]), float(voxel_xy[1]), int(stride), int(num_max_objs),
        float(gaussian_overlap), int(min_radius), _chk(heat, "heat", torch.float32),
        _chk(tgt, "target_boxes", torch.float32), _chk(inds, "inds", torch.int64), _chk(masks, "masks", torch.int64),
        _chk(src, "target_boxes_src", torch.float32), _chk(status, "status", torch.int32, numel=1), _stream())
    _lib.check(rc, "dfu3d_center_assign")
    return heat, tgt, inds, masks, src


def center_decode(heat, rot_cos, rot_sin, center, center_z, dim, vel, iou, K, range_xy, voxel_xy, stride, limit,
                  score_thresh, out=None):
    """Top-K decode of a batch of head outputs (dfu3d_center_decode).  heat float32 (B,n_cls,H,W) and the regression
    maps -> boxes float32 (B,K,7|9), scores (B,K), labels int32 (B,K), iou (B,K) or None, count int32 (B); the first
    count[b] rows of sample b are valid.  out: (boxes, scores, labels, iou_out, count) preallocated, contiguous views
    of those shapes to write into (iou_out None without `iou`); they are what is returned."""
    if heat.dim() != 4:
        raise Dfu3dError("center_decode: heatmap must be (B, n_cls, H, W)")
    B, n_cls, H, W = (int(v) for v in heat.shape)
    if K > CENTER_MAX_K:
        raise Dfu3dError("center_decode: K = %d, at most %d" % (K, CENTER_MAX_K))
    dev = heat.device
    nb = 9 if vel is not None else 7
    if out is not None:
        boxes, scores, labels, iou_out, count = out
        if iou is None:
            iou_out = None
        elif iou_out is None:
            raise Dfu3dError("center_decode: out has no iou_out for the given iou map")
        for t, name, dtype, n in ((boxes, "boxes", torch.float32, B * K * nb), (scores, "scores", torch.float32, B * K),
                                  (labels, "labels", torch.int32, B * K), (iou_out, "iou_out", torch.float32, B * K),
                                  (count, "count", torch.int32, B)):
            if t is not None:
                _chk(t, "out." + name, dtype, numel=n)
        if B == 0:
            return boxes, scores, labels, iou_out, count
    else:
        boxes = torch.empty((B, K, nb), dtype=torch.float32, device=dev)
        scores = torch.empty((B, K), dtype=torch.float32, device=dev)
        labels = torch.empty((B, K), dtype=torch.int32, device=dev)
        iou_out = torch.empty((B, K), dtype=torch.float32, device=dev) if iou is not None else None
        count = torch.zeros(max(B, 1), dtype=torch.int32, device=dev)
        if B == 0:
            return boxes, scores, labels, iou_out, count[:0]
    hw = B * H * W
    rc = _lib.lib().dfu3d_center_decode(
        _chk(heat, "heatmap", torch.float32), _chk(rot_cos, "rot_cos", torch.float32, numel=hw),
        _chk(rot_sin, "rot_sin", torch.float32, numel=hw), _chk(center, "center", torch.float32, numel=2 * hw),
        _chk(center_z, "center_z", torch.float32, numel=hw), _chk(dim, "dim", torch.float32, numel=3 * hw),
        None if vel is None else _chk(vel, "vel", torch.float32, numel=2 * hw),
        None if iou is None else _chk(iou, "iou", torch.float32, numel=hw), B, n_cls, H, W, int(K),
        float(range_xy[0]), float(range_xy[1]), float(voxel_xy[0]), float(voxel_xy[1]), int(stride),
        _chk(limit, "post_center_limit_range", torch.float32, numel=6), 0 if score_thresh is None else 1,
        0.0 if score_thresh is None else float(score_thresh), _chk(boxes, "boxes", torch.float32),
        _chk(scores, "scores", torch.float32), _chk(labels, "labels", torch.int32),
        None if iou_out is None else _chk(iou_out, "iou_out", torch.float32), _chk(count, "count", torch.int32), _stream())
    _lib.check(rc, "dfu3d_center_decode")
    return boxes, scores, labels, iou_out, count


POST_MAX_CAP = _lib_post.CONSTANTS["DFU3D_POST_MAX_CAP"]


def nms_bev_segments(boxes, count, thresh, pre_max=None, post_max=None, normal=False):
    """Rotated NMS of S box lists in one launch chain (dfu3d_nms_bev_segments).  boxes float32 (S, cap, C >= 7), the rows
    of a segment in descending score order; count int32 (S) on the device: the rows of each segment that are valid.
    -> keep int32 (S, cap): the kept positions ascending, then -1; num_keep int32 (S).  No host read."""
    if boxes.dim() != 3 or boxes.shape[2] < 7:
        raise Dfu3dError("nms_bev_segments: boxes must be (S, cap, C >= 7), got %s" % (tuple(boxes.shape),))
    S, cap, C = (int(v) for v in boxes.shape)
    if cap > POST_MAX_CAP:
        raise Dfu3dError("nms_bev_segments: cap = %d, at most %d (DFU3D_ERANGE)" % (cap, POST_MAX_CAP))
    dev = boxes.device
    keep = torch.empty((S, cap), dtype=torch.int32, device=dev)
    num = torch.empty(S, dtype=torch.int32, device=dev)
    b_p = _chk(boxes, "boxes", torch.float32)
    c_p = _chk(count, "count", torch.int32, numel=S)
    if S == 0 or cap == 0:
        return keep, num.zero_()
    L = _lib_post.lib()
    nbytes = int(L.dfu3d_nms_segments_scratch_bytes(S, cap))
    scratch = torch.empty(max(nbytes, 8), dtype=torch.uint8, device=dev)
    rc = L.dfu3d_nms_bev_segments(b_p, S, cap, C, c_p, ctypes.c_float(thresh), int(pre_max or 0), int(post_max or 0),
                                  1 if normal else 0, ctypes.c_void_p(scratch.data_ptr()), nbytes,
                                  _chk(keep, "keep", torch.int32), _chk(num, "num_keep", torch.int32), _stream())
    _lib.check(rc, "dfu3d_nms_bev_segments")
    return keep, num


def center_collect(boxes, scores, labels, keep, num_keep, cls_map, out_cap):
    """The survivors of all heads per sample (dfu3d_center_collect).  boxes float32 (n_heads, B, cap, C), scores float32 and
    labels int32 (n_heads, B, cap), keep (n_heads * B, cap) and num_keep (n_heads * B) of nms_bev_segments, cls_map int32
    (n_heads, max_cls) -> out_boxes (B, out_cap, C), out_scores (B, out_cap), out_labels int64 (B, out_cap), out_count
    int32 (B); rows at or beyond out_count[b] are 0.  No host read."""
    if boxes.dim() != 4:
        raise Dfu3dError("center_collect: boxes must be (n_heads, B, cap, C), got %s" % (tuple(boxes.shape),))
    n_heads, B, cap, C = (int(v) for v in boxes.shape)
    if cls_map.dim() != 2 or cls_map.shape[0] != n_heads or cls_map.shape[1] < 1:
        raise Dfu3dError("center_collect: cls_map must be (n_heads, max_cls >= 1), got %s" % (tuple(cls_map.shape),))
    dev = boxes.device
    S, out_cap = n_heads * B, int(out_cap)
    out_boxes = torch.empty((B, out_cap, C), dtype=torch.float32, device=dev)
    out_scores = torch.empty((B, out_cap), dtype=torch.float32, device=dev)
    out_labels = torch.empty((B, out_cap), dtype=torch.int64, device=dev)
    out_count = torch.empty(B, dtype=torch.int32, device=dev)
    if B == 0:
        return out_boxes, out_scores, out_labels, out_count
    rc = _lib_post.lib().dfu3d_center_collect(
        _chk(boxes, "boxes", torch.float32), _chk(scores, "scores", torch.float32, numel=S * cap),
        _chk(labels, "labels", torch.int32, numel=S * cap), _chk(keep, "keep", torch.int32, numel=S * cap),
        _chk(num_keep, "num_keep", torch.int32, numel=S), n_heads, B, cap, C, _chk(cls_map, "cls_map", torch.int32),
        int(cls_map.shape[1]), out_cap, _chk(out_boxes, "out_boxes", torch.float32),
        _chk(out_scores, "out_scores", torch.float32), _chk(out_labels, "out_labels", torch.int64),
        _chk(out_count, "out_count", torch.int32), _stream())
    _lib.check(rc, "dfu3d_center_collect")
    return out_boxes, out_scores, out_labels, out_count


# Every integer macro DFU3D_AUG_<NAME> of include/dfu3d_aug.h is AUG_<NAME> here.
globals().update({name[len("DFU3D_"):]: value for name, value in _lib_aug.CONSTANTS.items()})

AUG_STATUS_TEXT = {
    AUG_ST_NONFINITE: "a point's x or y is not finite after the transform",
    AUG_ST_BOX_CAP: "a scene keeps more boxes than box_cap",
    AUG_ST_OFFSETS: "point_off / box_off / box_cnt do not describe the arrays",
}


def aug_status_message(word):
    return "; ".join(t for b, t in AUG_STATUS_TEXT.items() if word & b) or "ok"


def aug_params(records):
    """[{flags, cos_a, sin_a, scale_f, noise_rot_f, tx, ty, tz, noise_rot, scale}, ...] -> uint8 array (B, sizeof
    dfu3d_aug_params) laid out as the header's struct (missing keys: the neutral value)."""
    neutral = {"flags": 0, "cos_a": 1.0, "sin_a": 0.0, "scale_f": 1.0, "noise_rot_f": 0.0, "tx": 0.0, "ty": 0.0,
               "tz": 0.0, "noise_rot": 0.0, "scale": 1.0}
    arr = (_lib_aug.Params * max(len(records), 1))()
    for k, r in enumerate(records):
        unknown = set(r) - set(neutral)
        if unknown:
            raise Dfu3dError("aug_params: unknown field(s) %s" % sorted(unknown))
        for name, dv in neutral.items():
            setattr(arr[k], name, r.get(name, dv))
    raw = np.frombuffer(arr, dtype=np.uint8).reshape(max(len(records), 1), ctypes.sizeof(_lib_aug.Params))
    return raw[:len(records)].copy()


def world_aug_collate(points, point_off, boxes, box_off, box_cnt, box_cls, params, pc_range, mode, box_cap, status,
                      want_aug=False, want_keep=False):
    """World augmentation, range masks and collate for B scenes (dfu3d_world_aug_collate): points float32 (N, C) by
    scene (point_off int64 (B+1); N may exceed point_off[B]: the rows behind it are never read); boxes float32 or float64 (Nt, 7|9) with box_off int32 (B+1), box_cnt int32 (B),
    box_cls int32 (Nt); params uint8 (B, sizeof dfu3d_aug_params) of aug_params(); pc_range float32 (6); mode: AUG_MASK_POINTS |
    AUG_MASK_BOXES | AUG_FILTER_CLASS -> points_out float32 (N, 1 + C), n_kept int32 (1), point_cnt int32 (B),
    gt_boxes float32 (B, box_cap, 8|10), gt_cnt int32 (B), boxes_aug (Nt, 7|9) or None, box_keep int32 (Nt) or None.
    Everything is checked on the host before the first launch; nothing here synchronises or copies to the host."""
    if not isinstance(points, torch.Tensor) or points.dim() != 2 or points.shape[1] < 3:
        raise Dfu3dError("world_aug_collate: points must be a (N, C >= 3) tensor")
    if not isinstance(boxes, torch.Tensor) or boxes.dim() != 2 or boxes.shape[1] not in (7, 9):
        raise Dfu3dError("world_aug_collate: boxes must be (Nt, 7) or (Nt, 9), got %s"
                         % (tuple(boxes.shape) if isinstance(boxes, torch.Tensor) else type(boxes),))
    if boxes.dtype not in (torch.float32, torch.float64):
        raise Dfu3dError("world_aug_collate: boxes must be float32 or float64, got %s" % boxes.dtype)
    if not isinstance(box_cnt, torch.Tensor) or box_cnt.dim() != 1:
        raise Dfu3dError("world_aug_collate: box_cnt must be an int32 tensor (B)")
    N, C = (int(v) for v in points.shape)
    nt, nc = (int(v) for v in boxes.shape)
    B, box_cap, mode = int(box_cnt.shape[0]), int(box_cap), int(mode)
    if mode & ~(AUG_MASK_POINTS | AUG_MASK_BOXES | AUG_FILTER_CLASS):
        raise Dfu3dError("world_aug_collate: unknown mode bits in %d" % mode)
    if N > AUG_MAX_ROWS or B > AUG_MAX_SCENES or C > AUG_MAX_POINT_COLS or box_cap > AUG_MAX_BOX_CAP:
        raise Dfu3dError("world_aug_collate: N = %d, B = %d, C = %d, box_cap = %d beyond the caps of dfu3d_aug.h "
                         "(DFU3D_ERANGE)" % (N, B, C, box_cap))
    if box_cap < 0 or (B == 0 and (N or nt)):
        raise Dfu3dError("world_aug_collate: box_cap < 0, or rows without a scene")
    psize = ctypes.sizeof(_lib_aug.Params)
    dev = points.device
    pts_p = _chk(points, "points", torch.float32) if N else None
    box_p = _chk(boxes, "boxes", boxes.dtype) if nt else None
    cls_p = _chk(box_cls, "box_cls", torch.int32, numel=nt) if nt else None
    if B:
        poff_p = _chk(point_off, "point_off", torch.int64, numel=B + 1)
        boff_p = _chk(box_off, "box_off", torch.int32, numel=B + 1)
        bcnt_p = _chk(box_cnt, "box_cnt", torch.int32, numel=B)
        par_p = _chk(params, "params", torch.uint8, numel=B * psize)
        rng_p = _chk(pc_range, "pc_range", torch.float32, numel=6)
    else:
        poff_p = boff_p = bcnt_p = par_p = rng_p = None
    st_p = _chk(status, "status", torch.int32, numel=1)
    out = torch.empty((N, C + 1), dtype=torch.float32, device=dev)
    n_kept = torch.empty(1, dtype=torch.int32, device=dev)
    point_cnt = torch.empty(B, dtype=torch.int32, device=dev)
    gt = torch.empty((B, box_cap, nc + 1), dtype=torch.float32, device=dev)
    gt_cnt = torch.empty(B, dtype=torch.int32, device=dev)
    aug = torch.empty((nt, nc), dtype=boxes.dtype, device=dev) if want_aug else None
    keep = torch.empty(nt, dtype=torch.int32, device=dev) if want_keep else None
    L = _lib_aug.lib()
    nbytes = int(L.dfu3d_world_aug_scratch_bytes(N))
    scratch = torch.empty((nbytes + 7) // 8, dtype=torch.int64, device=dev)

    def ptr(t):
        return ctypes.c_void_p(t.data_ptr()) if t is not None and t.numel() else None
    rc = L.dfu3d_world_aug_collate(
        pts_p, N, C, poff_p, B, box_p, 1 if boxes.dtype == torch.float64 else 0, nc, nt, boff_p, bcnt_p, cls_p,
        ctypes.cast(par_p, ctypes.POINTER(_lib_aug.Params)) if par_p is not None else None, rng_p, mode, ptr(out),
        ptr(n_kept), ptr(point_cnt), ptr(gt), box_cap, ptr(gt_cnt), ptr(aug), ptr(keep),
        ctypes.c_void_p(scratch.data_ptr()), nbytes, st_p, _stream())
    _lib_aug.check(rc, "dfu3d_world_aug_collate")
    return out, n_kept, point_cnt, gt, gt_cnt, aug, keep
