/* dfu3d_vfe.h -- C ABI of the dynamic pillar feature encoder stage of libdfu3d_hip.so (csrc/pillar_stage.hip).
 *
 * The entry points live in the same library as include/dfu3d.h's and follow its rules: device pointers, results in
 * device memory, the library never allocates and never synchronises, every call returns DFU3D_OK / DFU3D_EINVAL /
 * DFU3D_ELAUNCH / DFU3D_ERANGE (dfu3d.h) and validates its arguments on the host before any launch.  The header keeps
 * to the C subset dfu3d_amd/_header.py reads.
 *
 * Numerics: float32, IEEE, no contraction; every float sum runs over a pillar's points in ascending point index, so
 * every result is bit-reproducible.  x and the gradients must hold no NaN (the order of a maximum over NaN is not
 * defined).
 *
 * Sizes: the chain learns n_kept (points inside the grid) and P (occupied pillars) on the device: `sizes` is int32[2] =
 * {n_kept, P}, written by dfu3d_pillar_group and read by every later kernel, which are launched over the capacities
 * the caller passes (n_points resp. n_cap / p_cap).  Rows beyond n_kept / P of an output are not written.
 */
#ifndef DFU3D_VFE_H
#define DFU3D_VFE_H

#include <stdint.h>

#define DFU3D_VFE_VERSION 100

/* batch_size * nx * ny at most: a 2 MiB occupancy bitmap, keys far inside int32 */
#define DFU3D_VFE_MAX_CELLS 16777216
/* channels of dfu3d_pillar_max at most */
#define DFU3D_VFE_MAX_CHANNELS 256
/* columns of a point row (batch index + features) at most */
#define DFU3D_VFE_MAX_POINT_COLS 64

/* status bits of dfu3d_pillar_group (a word of its own, not dfu3d.h's) */
#define DFU3D_VFE_ST_BAD_POINT 1u   /* a point with non-finite x or y, or a batch index outside [0, batch_size): dropped */

/* feature / coordinate layouts */
#define DFU3D_VFE_LAYOUT_PILLAR 0   /* DynamicPillarVFE: [raw, f_cluster, f_center, (dist)]; coords [b, 0, y, x] */
#define DFU3D_VFE_LAYOUT_SIMPLE2D 1 /* DynamicPillarVFESimple2D: [f_center, raw, (dist)]; coords [b, y, x] */

#ifdef __cplusplus
extern "C" {
#endif

int32_t dfu3d_vfe_version(void);

/* bytes of scratch dfu3d_pillar_group / dfu3d_pillar_features need for n_points points over n_cells =
 * batch_size * nx * ny cells; -1 for a negative argument or n_cells beyond DFU3D_VFE_MAX_CELLS.  The scratch must be
 * 16-byte aligned; dfu3d_pillar_features reuses the block after the grouping for the pillar means. */
int64_t dfu3d_vfe_scratch_bytes(int64_t n_points, int64_t n_cells);

/* Pillar grouping.  points (n_points, point_cols) float32, column 0 the batch index, columns 1..3 x y z.
 * c = floor((xy - range) / voxel); a point is kept iff 0 <= c < (nx, ny), compared in float; key = b*nx*ny + cx*ny + cy.
 * With p_cap = min(n_points, batch_size*nx*ny):
 *   kept_idx (n_points)   index of every kept point, ascending
 *   unq_inv  (n_points)   pillar of every kept point; pillars are numbered in ascending key order
 *   unq_cnt  (p_cap)      points per pillar
 *   coords   (p_cap, 4|3) per pillar [b, 0, cy, cx] (LAYOUT_PILLAR) or [b, cy, cx] (LAYOUT_SIMPLE2D)
 *   offsets  (p_cap + 1), plist (n_points): CSR of the pillars over rows of the kept list, ascending inside a pillar
 *   sizes    int32[2] = {n_kept, P};  status: DFU3D_VFE_ST_* (both reset by the call) */
int dfu3d_pillar_group(const float *points, int32_t n_points, int32_t point_cols, int32_t batch_size,
                       float range_x, float range_y, float voxel_x, float voxel_y, int32_t nx, int32_t ny,
                       int32_t layout, int32_t *kept_idx, int32_t *unq_inv, int32_t *unq_cnt, int32_t *coords,
                       int32_t *offsets, int32_t *plist, int32_t *sizes, uint32_t *status, void *scratch,
                       int64_t scratch_bytes, void *stream);

/* The matrix entering the first PFN layer, (n_kept, feat_cols) into `features` (n_points rows of room):
 * raw = columns 1.. (use_abs_xyz) or 4.. of the point; f_cluster = xyz - mean of the pillar (float32 sum in ascending
 * point index / float(count)); f_center = xy - (float(c) * voxel + offset), z - offset_z; dist = sqrt(fma(z, z, fma(y, y, x*x))).
 * feat_cols must equal the layout's width.  Runs after dfu3d_pillar_group on the same stream. */
int dfu3d_pillar_features(const float *points, int32_t n_points, int32_t point_cols, float range_x, float range_y,
                          float voxel_x, float voxel_y, float offset_x, float offset_y, float offset_z,
                          int32_t layout, int32_t use_abs_xyz, int32_t with_distance, const int32_t *kept_idx,
                          const int32_t *unq_inv, const int32_t *offsets, const int32_t *plist, const int32_t *sizes,
                          float *features, int32_t feat_cols, void *scratch, int64_t scratch_bytes, void *stream);

/* Per-pillar maximum over rows.  x (n_cap, C) float32, C <= DFU3D_VFE_MAX_CHANNELS -> x_max (p_cap, C), arg (p_cap, C)
 * the row of the maximum (the lowest among equals), and, when concat is not null, concat (n_cap, 2C) =
 * [x, x_max[unq_inv]]. */
int dfu3d_pillar_max(const float *x, int32_t n_cap, int32_t C, const int32_t *offsets, const int32_t *plist,
                     int32_t p_cap, const int32_t *sizes, float *x_max, int32_t *arg, float *concat, void *stream);

/* Backward of dfu3d_pillar_max.  Exactly one of grad_max (p_cap, C) and grad_concat (n_cap, 2C) is not null.
 * grad_x (n_cap, C) = grad_max routed to arg, or grad_concat[:, :C] + (the per-pillar sum of grad_concat[:, C:], in
 * ascending row order, routed to arg).  Every row below n_kept is written; no float atomics. */
int dfu3d_pillar_max_backward(const float *grad_max, const float *grad_concat, int32_t n_cap, int32_t C,
                              const int32_t *arg, const int32_t *offsets, const int32_t *plist, int32_t p_cap,
                              const int32_t *sizes, float *grad_x, void *stream);

#ifdef __cplusplus
}
#endif

#endif
