// chain_stage.hip -- the whole pseudo-box path for V views behind ONE C call
// (vis_utils.py:136-166 -> my_loader.py:502-702 -> label rows), for hosts that do not want
// to sequence the stage entry points themselves.  It only sequences them: every kernel is
// the one the per-stage entry points launch, the workspace is carved from one caller-owned
// buffer, nothing is allocated, nothing synchronises.
#include "common.hpp"

namespace {

struct ChainWs {
  int32_t *fov_idx, *cand_idx, *ag_pt, *ib_pix, *n_fov, *n_ag, *K;
  double *plane;
  uint32_t *a_bits;
  double *a_x, *a_y, *a_z;
  int32_t *n_vox;
  uint32_t *vox_pix, *b_bits;
  double *b_x, *b_y, *b_z;
  void *table;
  uint32_t *pix_bin;
  int32_t *blk_cnt;
  double *px, *py, *pz, *sx, *sy;
  int32_t *label, *sroot, *si3;
  double *fit_ws;
  uint8_t *flags;
  int64_t *base_a, *base_b, *base_ab;
  int32_t *cnt_a, *cnt_b, *cnt_all, *cnt_ab, *tile_off, *queue, *stat_enable;
  double *rad_ab, *mean_d;
  void *vd_scratch;
  void *shadow;
  int32_t *chunk_cnt;
  int64_t *pool_cursor;
  int64_t table_entries;
};

// Bytes of the buffers of the path, each written ONCE, by the name it has in ChainWs: carve() slices the workspace with
// them and dfu3d_workspace_bytes() adds up the ones a stage's entry point takes (a slice is this rounded up to 256).
// Plain arithmetic on the sizes as given: a size function that refuses them leaves a figure <= 0, for the caller to refuse.
struct BufBytes {
  int64_t per_point_i32, per_point_f64;  // fov_idx, cand_idx, ag_pt, ib_pix, a_bits | a_x, a_y, a_z
  int64_t per_view_i32, plane;           // n_fov, n_ag, K, n_vox | plane
  int64_t per_vox_u32, per_vox_f64;      // vox_pix, b_bits | b_x, b_y, b_z
  int64_t table, pix_bin, blk_cnt;       // dense only
  int64_t per_slot_f64, per_slot_i32;    // px, py, pz, sx, sy, mean_d | label, sroot
  int64_t si3, fit_ws, flags;
  int64_t per_seg_i64, per_seg_i32;      // base_a, base_b (base_ab, rad_ab: two of them) | cnt_a, cnt_b, cnt_all, stat_enable (cnt_ab: two)
  int64_t queue, shadow, chunk_cnt, vd_scratch, pool_cursor;
};
// tile_off holds, per list of tiles a kernel builds, one offset per segment and the total.  The radius filter builds one
// list over its n segments (2S for the joint pass), the statistical filter one over S, the ball query two over S -- the
// largest, which is what carve() takes; dfu3d_workspace_bytes answers with each stage's own figure.
inline int64_t tile_off_bytes(int64_t segments, int lists) { return 4 * lists * (segments + 1); }

BufBytes buf_bytes(const dfu3d_sizes &z) {
  const int64_t V = z.V, S = V * z.max_inst, N = V * z.cap_n, X = V * z.cap_vox, P = z.pool_cap;
  BufBytes b;
  b.per_point_i32 = 4 * N; b.per_point_f64 = 8 * N;
  b.per_view_i32 = 4 * V; b.plane = 8 * V * 4;
  b.per_vox_u32 = 4 * X; b.per_vox_f64 = 8 * X;
  int64_t pw = 0, bw = 0;                // (stay 0 where the size function refuses the sizes)
  if (z.table_entries > 0)
    dfu3d_backproject_scratch_words(z.V, z.H, z.W, z.cap_vox, z.max_points_per_voxel, z.table_entries, &pw, &bw);
  b.table = V * z.table_entries * DFU3D_TABLE_ENTRY_BYTES; b.pix_bin = 4 * pw; b.blk_cnt = 4 * bw;
  b.per_slot_f64 = 8 * P; b.per_slot_i32 = 4 * P; b.si3 = 4 * 3 * P; b.flags = P;
  b.fit_ws = 8 * dfu3d_lshape_fit_ws_doubles(P, z.cap_rows);
  b.per_seg_i64 = 8 * S; b.per_seg_i32 = 4 * S;
  b.queue = 4 * DFU3D_RF_QUEUE_INTS(P); b.shadow = DFU3D_SHADOW_BYTES(P);
  b.chunk_cnt = 4 * dfu3d_segments_scratch_words(z.V, z.cap_n, z.cap_vox);
  b.vd_scratch = dfu3d_voxel_down_sample_scratch_bytes(P);
  b.pool_cursor = 8;
  return b;
}

dfu3d_sizes sizes_of(const dfu3d_chain_cfg *c) {
  dfu3d_sizes z = {};
  z.V = c->V; z.H = c->H; z.W = c->W; z.max_inst = c->max_inst; z.cap_n = c->cap_n; z.cap_vox = c->cap_vox;
  z.cap_rows = c->cap_rows; z.max_points_per_voxel = c->geom.max_points_per_voxel; z.pool_cap = c->pool_cap;
  z.table_entries = (int64_t)c->geom.t_n * c->geom.p_n; z.dense = c->dense; z.stat_filter = c->stat_filter;
  return z;
}

// carve the workspace; with base == nullptr only the size is computed
int64_t carve(const dfu3d_chain_cfg *c, char *base, ChainWs *w) {
  int64_t off = 0;
  auto take = [&](int64_t bytes) -> char * {
    char *p = base ? base + off : nullptr;
    off += (bytes + 255) / 256 * 256;
    return p;
  };
  const dfu3d_sizes z = sizes_of(c);
  const BufBytes b = buf_bytes(z);
  ChainWs t;
  t.fov_idx = (int32_t *)take(b.per_point_i32); t.cand_idx = (int32_t *)take(b.per_point_i32);
  t.ag_pt = (int32_t *)take(b.per_point_i32); t.ib_pix = (int32_t *)take(b.per_point_i32);
  t.n_fov = (int32_t *)take(b.per_view_i32); t.n_ag = (int32_t *)take(b.per_view_i32); t.K = (int32_t *)take(b.per_view_i32);
  t.plane = (double *)take(b.plane);
  t.a_bits = (uint32_t *)take(b.per_point_i32);
  t.a_x = (double *)take(b.per_point_f64); t.a_y = (double *)take(b.per_point_f64); t.a_z = (double *)take(b.per_point_f64);
  t.n_vox = (int32_t *)take(b.per_view_i32);
  t.vox_pix = (uint32_t *)take(b.per_vox_u32); t.b_bits = (uint32_t *)take(b.per_vox_u32);
  t.b_x = (double *)take(b.per_vox_f64); t.b_y = (double *)take(b.per_vox_f64); t.b_z = (double *)take(b.per_vox_f64);
  t.table_entries = z.table_entries;
  t.table = c->dense ? take(b.table) : nullptr;
  t.pix_bin = c->dense ? (uint32_t *)take(b.pix_bin) : nullptr;
  t.blk_cnt = c->dense ? (int32_t *)take(b.blk_cnt) : nullptr;
  t.px = (double *)take(b.per_slot_f64); t.py = (double *)take(b.per_slot_f64); t.pz = (double *)take(b.per_slot_f64);
  t.sx = (double *)take(b.per_slot_f64); t.sy = (double *)take(b.per_slot_f64);
  t.label = (int32_t *)take(b.per_slot_i32); t.sroot = (int32_t *)take(b.per_slot_i32); t.si3 = (int32_t *)take(b.si3);
  t.fit_ws = (double *)take(b.fit_ws);
  t.flags = (uint8_t *)take(b.flags);
  t.base_a = (int64_t *)take(b.per_seg_i64); t.base_b = (int64_t *)take(b.per_seg_i64); t.base_ab = (int64_t *)take(2 * b.per_seg_i64);
  t.cnt_a = (int32_t *)take(b.per_seg_i32); t.cnt_b = (int32_t *)take(b.per_seg_i32); t.cnt_all = (int32_t *)take(b.per_seg_i32);
  t.cnt_ab = (int32_t *)take(2 * b.per_seg_i32); t.tile_off = (int32_t *)take(tile_off_bytes((int64_t)z.V * z.max_inst, 2));
  t.queue = (int32_t *)take(b.queue); t.stat_enable = (int32_t *)take(b.per_seg_i32);
  t.shadow = take(b.shadow);
  t.chunk_cnt = (int32_t *)take(b.chunk_cnt);
  t.rad_ab = (double *)take(2 * b.per_seg_i64);
  t.mean_d = c->stat_filter ? (double *)take(b.per_slot_f64) : nullptr;
  t.vd_scratch = c->stat_filter ? (void *)take(b.vd_scratch) : nullptr;
  t.pool_cursor = (int64_t *)take(b.pool_cursor);
  if (w) *w = t;
  return off;
}

bool cfg_ok(const dfu3d_chain_cfg *c) {
  return c && c->V > 0 && c->H > 0 && c->W > 0 && c->max_inst > 0 && c->max_inst <= DFU3D_MAX_INST &&
         c->cap_n > 0 && c->cap_vox > 0 && c->cap_rows > 0 && c->pool_cap > 0 && c->n_theta > 0 &&
         c->bounds_h > 0 && c->bounds_w > 0 && c->bounds_h <= c->H && c->bounds_w <= c->W &&
         mask_format_ok(c->mask_format, c->max_inst) &&
         (!c->dense || (c->geom.t_n > 0 && c->geom.p_n > 0)) &&
         (!c->stat_filter || (c->stat_voxel > 0.0 && c->stat_nb_neighbors >= 1));
}

// apply_fov == 0: the caller's points are already the FOV points (vis_utils.py:152-154 done upstream)
__global__ void k_all_points(const int *__restrict__ pt_off, const int *__restrict__ view_frame,
                             int cap_n, int *__restrict__ fov_idx, int *__restrict__ n_fov) {
  const int v = blockIdx.y;
  const int f = view_frame[v];
  const int n = min(pt_off[f + 1] - pt_off[f], cap_n);
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < cap_n; i += gridDim.x * blockDim.x)
    fov_idx[(size_t)v * cap_n + i] = i;
  if (blockIdx.x == 0 && threadIdx.x == 0) n_fov[v] = n;
}

__global__ void k_sum_counts(int S, const int *__restrict__ a, const int *__restrict__ b, int *__restrict__ out) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s < S) out[s] = a[s] + b[s];
}

__global__ void k_fill_i32(int n, int v, int *__restrict__ p) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) p[i] = v;
}

}  // namespace

extern "C" int64_t dfu3d_chain_workspace_bytes(const dfu3d_chain_cfg *cfg) {
  if (!cfg_ok(cfg)) return DFU3D_EINVAL;
  return carve(cfg, nullptr, nullptr);
}

extern "C" int64_t dfu3d_workspace_bytes(int32_t stage, const dfu3d_sizes *z) {
  if (!z || z->V <= 0 || z->max_inst <= 0 || z->max_inst > DFU3D_MAX_INST) return DFU3D_EINVAL;
  auto up = [](int64_t bytes) { return (bytes + 255) / 256 * 256; };
  const int64_t S = (int64_t)z->V * z->max_inst, P = z->pool_cap;
  const BufBytes b = buf_bytes(*z);
  switch (stage) {
    case DFU3D_STAGE_FOV_FILTER:
      return 0;
    case DFU3D_STAGE_SEGMENTS_BUILD:
      return (z->cap_n > 0 && z->cap_vox > 0) ? up(b.chunk_cnt) : DFU3D_EINVAL;
    case DFU3D_STAGE_PLANE_RANSAC:                       /* cand_idx */
      return z->cap_n > 0 ? up(b.per_point_i32) : DFU3D_EINVAL;
    case DFU3D_STAGE_PROJECT_LABEL:                      /* ag_pt, ib_pix */
      return z->cap_n > 0 ? 2 * up(b.per_point_i32) : DFU3D_EINVAL;
    case DFU3D_STAGE_BACKPROJECT_BIN:
      return b.blk_cnt > 0 ? up(b.table) + up(b.pix_bin) + up(b.blk_cnt) : DFU3D_EINVAL;
    case DFU3D_STAGE_RADIUS_FILTER:                      /* (2S joint segments) */
      return P > 0 ? up(b.shadow) + up(tile_off_bytes(2 * S, 1)) + up(b.flags) + up(b.queue) : DFU3D_EINVAL;
    case DFU3D_STAGE_STAT_FILTER:                        /* tile_off, flags, mean_d */
      return P > 0 ? up(tile_off_bytes(S, 1)) + up(b.flags) + up(b.per_slot_f64) : DFU3D_EINVAL;
    case DFU3D_STAGE_VOXEL_DOWN_SAMPLE:
      return P > 0 ? up(b.vd_scratch) : DFU3D_EINVAL;
    case DFU3D_STAGE_BALLQUERY_FUSE:
      return P > 0 ? up(tile_off_bytes(S, 2)) + up(b.flags) : DFU3D_EINVAL;
    case DFU3D_STAGE_RANGE_CLUSTER:                      /* sx, sy, si */
      return P > 0 ? 2 * up(b.per_slot_f64) + up(b.si3) : DFU3D_EINVAL;
    case DFU3D_STAGE_LSHAPE_FIT:                         /* sx, sy, sroot, fit_ws */
      return (P > 0 && z->cap_rows > 0) ? 2 * up(b.per_slot_f64) + up(b.per_slot_i32) + up(b.fit_ws) : DFU3D_EINVAL;
    case DFU3D_STAGE_PSEUDO_BOXES: {
      dfu3d_chain_cfg c = {};
      c.V = z->V; c.H = z->H; c.W = z->W; c.max_inst = z->max_inst; c.cap_n = z->cap_n; c.cap_vox = z->cap_vox;
      c.cap_rows = z->cap_rows; c.dense = z->dense; c.stat_filter = z->stat_filter; c.pool_cap = z->pool_cap;
      c.bounds_h = z->H; c.bounds_w = z->W; c.n_theta = 1;
      c.geom.max_points_per_voxel = z->max_points_per_voxel;
      c.geom.t_n = 1; c.geom.p_n = (int32_t)z->table_entries;       /* only the product enters the size */
      if (z->dense && (z->table_entries <= 0 || z->table_entries > 0x7FFFFFFF)) return DFU3D_EINVAL;
      return dfu3d_chain_workspace_bytes(&c);
    }
    default:
      return DFU3D_EINVAL;
  }
}

extern "C" int dfu3d_chain_workspace_init(const dfu3d_chain_cfg *cfg, void *workspace, void *stream) {
  DFU3D_CLEAR_STALE_ERROR();
  if (!cfg_ok(cfg) || !workspace) return DFU3D_EINVAL;
  ChainWs w;
  carve(cfg, (char *)workspace, &w);
  if (cfg->dense) {
    const int rc = dfu3d_bin_table_init(w.table, (int64_t)cfg->V * w.table_entries, stream);
    if (rc) return rc;
    const int rt = dfu3d_bp_tables_forget(w.blk_cnt, cfg->V, cfg->H, cfg->W, cfg->cap_vox, cfg->geom.max_points_per_voxel,
                                          w.table_entries, stream);
    if (rt) return rt;
  }
  hipLaunchKernelGGL(k_fill_i32, dim3((cfg->V * cfg->max_inst + 255) / 256), dim3(256), 0,
                     (hipStream_t)stream, cfg->V * cfg->max_inst, 1, w.stat_enable);
  DFU3D_LAUNCH_CHECK();
  return DFU3D_OK;
}

#define CHAIN_TRY(call)      \
  do {                       \
    const int rc_ = (call);  \
    if (rc_) return rc_;     \
  } while (0)

extern "C" int dfu3d_pseudo_boxes(
    const dfu3d_chain_cfg *cfg, const float *points, const int32_t *pt_off,
    const int32_t *view_frame, const float *calib, const void *masks, const int32_t *n_inst,
    const float *depth, const int64_t *view_key, const double *plane_in, const int32_t *inst_class,
    const int32_t *inst_is_car, const double *inst_r_lidar, const double *inst_r_pseudo,
    const float *inst_box, const float *inst_score, void *workspace, double *rows, int32_t *n_rows,
    uint32_t *status, void *stream) {
  DFU3D_CLEAR_STALE_ERROR();
  if (!cfg_ok(cfg) || !points || !pt_off || !view_frame || !calib || !masks || !n_inst || !inst_class ||
      !inst_is_car || !inst_r_lidar || !inst_r_pseudo || !inst_box || !inst_score || !workspace || !rows ||
      !n_rows || !status)
    return DFU3D_EINVAL;
  if (!plane_in && !view_key) return DFU3D_EINVAL;
  if (cfg->dense && !depth) return DFU3D_EINVAL;
  ChainWs w;
  carve(cfg, (char *)workspace, &w);
  hipStream_t st = (hipStream_t)stream;
  const int V = cfg->V, M = cfg->max_inst, S = V * M, cap_n = cfg->cap_n;
  // (one kernel, not three memsets: common.hpp, k_fill_words; with the dense path the same launch zeroes the words the
  // back-projection starts from)
  if (cfg->dense) {
    CHAIN_TRY(dfu3d_bp_clear_chain(w.blk_cnt, V, cfg->H, cfg->W, w.table_entries, n_rows, sizeof(int32_t), status,
                                   sizeof(uint32_t), w.pool_cursor, sizeof(int64_t), stream));
  } else if (dfu3d_fill_small_async(n_rows, sizeof(int32_t), status, sizeof(uint32_t), w.pool_cursor, sizeof(int64_t), st) != hipSuccess) {
    return DFU3D_ELAUNCH;
  }
  // a4
  if (cfg->apply_fov) {
    CHAIN_TRY(dfu3d_fov_filter(points, pt_off, view_frame, calib, V, cfg->fov_h, cfg->fov_w, cap_n,
                               w.fov_idx, w.n_fov, stream));
  } else {
    hipLaunchKernelGGL(k_all_points, dim3((cap_n + 255) / 256 < 64 ? (cap_n + 255) / 256 : 64, V), dim3(256), 0, st,
                       pt_off, view_frame, cap_n, w.fov_idx, w.n_fov);
    DFU3D_LAUNCH_CHECK();
  }
  // a5
  const double *plane = plane_in;
  if (!plane) {
    CHAIN_TRY(dfu3d_plane_ransac(points, pt_off, view_frame, w.fov_idx, w.n_fov, V, cap_n, cfg->plane_max_hs,
                                 cfg->plane_range, cfg->ransac_trials, cfg->ransac_seed, view_key,
                                 w.cand_idx, w.plane, stream));
    plane = w.plane;
  }
  // a5/a6
  CHAIN_TRY(dfu3d_project_label(points, pt_off, view_frame, calib, plane, w.fov_idx, w.n_fov, masks,
                                cfg->mask_format, n_inst, V, M, cfg->H, cfg->W, cfg->bounds_h, cfg->bounds_w,
                                cap_n, cfg->plane_offset, cfg->plane_range, w.ag_pt,
                                w.ib_pix, w.n_ag, w.K, w.a_bits, w.a_x, w.a_y, w.a_z, stream));
  // a7-a9
  if (cfg->dense) {
    CHAIN_TRY(dfu3d_backproject_bin_chain(depth, calib, masks, cfg->mask_format, n_inst, V, M, cfg->H, cfg->W, &cfg->geom, 1,
                                          w.table, w.pix_bin, w.blk_cnt, cfg->cap_vox, w.n_vox, w.vox_pix, w.b_bits, w.b_x,
                                          w.b_y, w.b_z, status, stream));
  } else {
    if (dfu3d_fill_async(w.n_vox, 0, sizeof(int32_t) * V, st) != hipSuccess) return DFU3D_ELAUNCH;
  }
  const bool joint = !cfg->stat_filter;   // one radius-filter pass over the LiDAR and pseudo lists together
  CHAIN_TRY(dfu3d_segments_build(w.a_bits, w.a_x, w.a_y, w.a_z, w.K, cap_n, w.b_bits, w.b_x, w.b_y, w.b_z,
                                 w.n_vox, cfg->cap_vox, V, M, cfg->pool_cap, w.pool_cursor, w.px, w.py, w.pz,
                                 w.base_a, w.cnt_a, w.base_b, w.cnt_b, status, inst_r_lidar, inst_r_pseudo,
                                 joint ? w.shadow : nullptr, joint ? w.base_ab : nullptr, w.cnt_ab, w.rad_ab,
                                 w.chunk_cnt, stream));
  // a10 (+a11) + a12
  if (joint) {
    // the shadow and the joint segment table come from the segment build; both lists keep their flags for the
    // joint fuse (one compaction launch for both lists and both filters)
    CHAIN_TRY(dfu3d_radius_filter(w.px, w.py, w.pz, w.base_ab, w.cnt_ab, w.rad_ab, cfg->nb_points, 2 * S,
                                  cfg->pool_cap, w.pool_cursor, w.shadow, w.tile_off, w.flags, w.queue,
                                  DFU3D_RF_FLAGS | DFU3D_RF_RESOLVE, stream));
    CHAIN_TRY(dfu3d_ballquery_fuse_joint(w.px, w.py, w.pz, w.base_a, w.cnt_a, w.base_b, w.cnt_b, cfg->fuse_C,
                                          S, cfg->pool_cap, w.tile_off, w.flags, stream));
  } else {
    CHAIN_TRY(dfu3d_radius_filter(w.px, w.py, w.pz, w.base_a, w.cnt_a, inst_r_lidar, cfg->nb_points, S,
                                  cfg->pool_cap, w.pool_cursor, w.shadow, w.tile_off, w.flags, w.queue,
                                  DFU3D_RF_ALL, stream));
    CHAIN_TRY(dfu3d_radius_filter(w.px, w.py, w.pz, w.base_b, w.cnt_b, inst_r_pseudo, cfg->nb_points, S,
                                  cfg->pool_cap, w.pool_cursor, w.shadow, w.tile_off, w.flags, w.queue,
                                  DFU3D_RF_ALL, stream));
    CHAIN_TRY(dfu3d_voxel_down_sample(w.px, w.py, w.pz, w.base_b, w.cnt_b, w.stat_enable, cfg->stat_voxel, S,
                                      cfg->pool_cap, w.vd_scratch, status, stream));
    CHAIN_TRY(dfu3d_stat_filter(w.px, w.py, w.pz, w.base_b, w.cnt_b, w.stat_enable, cfg->stat_nb_neighbors,
                                cfg->stat_std_ratio, S, cfg->pool_cap, w.tile_off, w.flags, w.mean_d, nullptr,
                                stream));
    CHAIN_TRY(dfu3d_ballquery_fuse(w.px, w.py, w.pz, w.base_a, w.cnt_a, w.base_b, w.cnt_b, cfg->fuse_C, S,
                                   cfg->pool_cap, w.tile_off, w.flags, stream));
  }
  hipLaunchKernelGGL(k_sum_counts, dim3((S + 255) / 256), dim3(256), 0, st, S, w.cnt_a, w.cnt_b, w.cnt_all);
  DFU3D_LAUNCH_CHECK();
  // a13-a15
  CHAIN_TRY(dfu3d_range_cluster(w.px, w.py, w.base_a, w.cnt_all, S, cfg->R0, cfg->Rd, w.label, w.sx, w.sy,
                                w.si3, cfg->pool_cap, stream));
  CHAIN_TRY(dfu3d_lshape_fit(w.px, w.py, w.pz, w.label, w.base_a, w.cnt_all, S, M, calib, inst_class,
                             inst_is_car, inst_box, inst_score, cfg->n_theta, cfg->dtheta, cfg->car_aspect_max,
                             w.sx, w.sy, w.sroot, cfg->cap_rows, rows, n_rows, status, w.fit_ws, cfg->pool_cap,
                             stream));
  return DFU3D_OK;
}

#ifdef DFU3D_DBG_COUNT_LAUNCHES
long long g_dbg_launches = 0;
extern "C" long long dfu3d_debug_launch_count(int reset) {
  const long long n = g_dbg_launches;
  if (reset) g_dbg_launches = 0;
  return n;
}
#endif
