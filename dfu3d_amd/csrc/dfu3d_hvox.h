/* dfu3d_hvox.h -- C ABI of the hard-voxel stage in libdfu3d_hip.so (csrc/hardvoxel_stage.hip): what
 * DataProcessor.transform_points_to_voxels computes scene by scene on the host with a third-party voxel generator -- at
 * most max_voxels voxels per scene in first-seen order, at most max_points rows each -- and what MeanVFE makes of it, for a
 * whole batch in DFU3D_HVOX_LAUNCHES kernel launches and without a read from the device.
 *
 * The entry points live in the library of the headers under include/ and follow its rules: device pointers, results in
 * device memory, the library never allocates, never synchronises and never reads from the device; every call returns
 * DFU3D_OK / DFU3D_EINVAL / DFU3D_ELAUNCH / DFU3D_ERANGE and validates its arguments on the host before any launch.  The
 * header keeps to the C subset dfu3d_amd/_header.py reads.  (It sits next to the sources and not under include/ because
 * the set of files there is pinned by an existing test: INTEGRATION.md.)
 *
 * That generator is not part of the build: THE RULE below is the contract.  The result is a pure function of the inputs.
 *
 * THE RULE.  Scene b owns the n = point_cnt[b] rows that start at the exclusive prefix sum of point_cnt; rows are
 * numbered i = 0 .. n-1 inside their scene and taken in that order.  For j = x, y, z
 *     c_j = floor(fl32(fl32(p_j - range_min_j) / voxel_size_j))
 * every operation rounded to float32 on its own, a true division (no reciprocal, no fused multiply-add).  A row is OUT if
 * any c_j is NaN, negative or >= fl32(grid_j), compared as floats before any conversion to an integer.  A row with a
 * non-finite x, y or z is OUT and ORs DFU3D_HVOX_ST_BAD_POINT into status.  A row that is not OUT belongs to the cell
 * (c_z, c_y, c_x) of its scene.  The first row of a cell makes a new voxel if the scene has fewer than max_voxels so
 * far; otherwise that row is dropped, and so is every later row of that cell.  Voxel ids are in first-seen order.  A row
 * is STORED in its voxel at slot s = the number of rows stored there before it, if s < max_points; otherwise it is
 * dropped.
 *
 * A negative point_cnt[b] is taken as 0, and counts that sum beyond R cut the scene at R (nothing outside `points` is
 * read); both OR DFU3D_HVOX_ST_BAD_COUNT into status.
 *
 * THE MEAN of a voxel with `count` stored rows, per feature column: acc = +0.0f, then acc = fl32(acc + v) over the stored
 * rows in slot order, then fl32(acc / (float)max(count, 1)).
 */
#ifndef DFU3D_HVOX_H
#define DFU3D_HVOX_H

#include <stddef.h>
#include <stdint.h>

#define DFU3D_HVOX_VERSION 1

/* kernel launches of one call of dfu3d_hard_voxels, for any B: the fills and the scene offsets, the cell table, the
 * counts of a block of rows, their prefix and the voxels of every scene, the voxel ids, the slots, the outputs */
#define DFU3D_HVOX_LAUNCHES 7
/* max_points at most.  Beyond it DFU3D_ERANGE */
#define DFU3D_HVOX_MAX_POINTS 128
/* scenes of a batch at most.  Beyond it DFU3D_ERANGE */
#define DFU3D_HVOX_MAX_BATCH 65535
/* elements of every block at most: R * (1 + C), V_cap * 4, V_cap * max_points * out_cols.  Beyond it DFU3D_ERANGE.  A
 * scene and a cell have no cap of their own below it */
#define DFU3D_HVOX_MAX_ELEMS 2147483647
/* B * grid_x * grid_y * grid_z stays below 2^DFU3D_HVOX_KEY_BITS (the cell keys are 64-bit words).  Beyond it
 * DFU3D_ERANGE */
#define DFU3D_HVOX_KEY_BITS 62
/* the cell table is an open-addressing hash over (b, cell) keys with the smallest power of two of entries that is at
 * least DFU3D_HVOX_TABLE_PER_ROW * R (and at least 16): its load never exceeds 1 / DFU3D_HVOX_TABLE_PER_ROW */
#define DFU3D_HVOX_TABLE_PER_ROW 2

/* bits OR-ed into *status (never cleared by the stage) */
/* a row with a non-finite x, y or z (the row is OUT) */
#define DFU3D_HVOX_ST_BAD_POINT 1
/* a negative point_cnt[b] (taken as 0), or counts that sum beyond R (the scene is cut at R) */
#define DFU3D_HVOX_ST_BAD_COUNT 2

/* The shape of the kernels, stated here because their LDS follows from it (tests/test_kernel_resources_hard_voxel.py):
 * threads of a workgroup of the row kernels (one workgroup takes a block of that many consecutive rows) and of the
 * single-workgroup kernels; threads of a workgroup of the output kernel */
#define DFU3D_HVOX_ROW_THREADS 1024
#define DFU3D_HVOX_OUT_THREADS 256

#ifdef __cplusplus
extern "C" {
#endif

int32_t dfu3d_hvox_version(void);

/* Bytes of scratch dfu3d_hard_voxels needs for these sizes: the cell table (per entry a 64-bit key, the first row, the
 * row count and the voxel: 20 bytes), per input row its table entry and a place in the slot lists, per possible voxel
 * the start and the length of its list, per block of DFU3D_HVOX_ROW_THREADS rows two prefixes, per scene its first row,
 * its first voxel and the voxels before it.  It grows with R and B only: no grid enters.  0 for B = 0 (nothing is launched
 * then) and for arguments out of range (negative sizes, B > DFU3D_HVOX_MAX_BATCH). */
size_t dfu3d_hvox_scratch_bytes(int32_t B, int32_t R);

/* points float32 (R, 1 + C), the output form of dfu3d_world_aug_collate / dfu3d_sample_points: column 0 is not read (the
 * scenes are contiguous and in order, point_cnt says where they are), then C feature columns, the first three x, y, z.
 * point_cnt int32 (B).  Rows at or beyond sum(point_cnt) are never read.  Neither is written.  range_min, voxel_size
 * (3 float32: x, y, z) and grid (3 int32: x, y, z) are read on the HOST during the call.  scratch: 16-byte aligned,
 * dfu3d_hvox_scratch_bytes(B, R) bytes at least, its content on entry does not matter.
 *
 * V_cap = min(B * max_voxels, R).  Voxels of scene 0 come first, then scene 1, ..., each in id order.
 *     voxel_cnt        int32 (B)                          voxels of every scene
 *     n_voxels         int32 (1)                          their sum
 *     voxel_coords     int32 (V_cap, 4)                   [b, z, y, x]; rows at or beyond n_voxels are -1
 *     voxel_num_points int32 (V_cap)                      stored rows, at least 1; the tail is 0
 *     voxels           float32 (V_cap, max_points, out_cols)  may be null.  Copies of the stored rows' first out_cols
 *                                                         features (the same bits); empty slots and the tail are +0.0
 *     voxel_mean       float32 (V_cap, out_cols)          may be null.  THE MEAN; the tail is +0.0
 *     point_voxel      int32 (R)                          the output row of the voxel the input row is stored in, or -1
 *     status           int32 (1)                          DFU3D_HVOX_ST_* bits, OR-ed
 * EVERY element of every block is written; the caller clears nothing.
 *
 * A null pointer (points and point_voxel may be null when R == 0; voxel_coords, voxel_num_points, voxels and voxel_mean
 * when V_cap == 0; one of voxels / voxel_mean always), voxels and voxel_mean both null, B < 0, R < 0, C < 3, out_cols
 * outside 3 .. C, max_points < 1, max_voxels < 1, a grid_j < 1, a voxel_size_j that is not finite and positive, a
 * range_min_j that is not finite, a scratch that is not 16-byte aligned or too short: DFU3D_EINVAL.  max_points >
 * DFU3D_HVOX_MAX_POINTS, B > DFU3D_HVOX_MAX_BATCH, B * grid_x * grid_y * grid_z >= 2^DFU3D_HVOX_KEY_BITS, R * (1 + C),
 * V_cap * 4 or V_cap * max_points * out_cols > DFU3D_HVOX_MAX_ELEMS: DFU3D_ERANGE.  B == 0: DFU3D_OK and nothing is launched
 * or written. */
int dfu3d_hard_voxels(const float *points, const int32_t *point_cnt, int32_t B, int32_t R, int32_t C,
                      const float *range_min, const float *voxel_size, const int32_t *grid, int32_t max_points,
                      int32_t max_voxels, int32_t out_cols, void *scratch, size_t scratch_bytes, int32_t *voxel_cnt,
                      int32_t *n_voxels, int32_t *voxel_coords, int32_t *voxel_num_points, float *voxels,
                      float *voxel_mean, int32_t *point_voxel, int32_t *status, void *stream);

#ifdef __cplusplus
}
#endif

#endif
