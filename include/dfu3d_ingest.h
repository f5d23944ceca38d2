/* dfu3d_ingest.h -- C ABI of the batched FOV ingest of libdfu3d_hip.so (csrc/ingest_stage.hip): what OpenPCDet's
 * KittiDataset does to the raw points of a frame before anything else -- lidar_to_rect, rect_to_img, the five comparisons
 * of get_fov_flag and the boolean gather (kitti_dataset.py:140-156, 480-486) -- and, for the info files, the number of
 * kept points inside every labelled box (:262-275), for a whole batch of frames in at most DFU3D_ING_LAUNCHES launches.
 *
 * The entry points live in the same library as include/dfu3d.h's and follow its rules: device pointers, results in
 * device memory, the library never allocates and never synchronises, every call returns DFU3D_OK / DFU3D_EINVAL /
 * DFU3D_ELAUNCH / DFU3D_ERANGE (dfu3d.h) and validates its arguments on the host before any launch.  The header keeps
 * to the C subset dfu3d_amd/_header.py reads.
 *
 * KEEP RULE (the reference's, bit for bit)
 *   rect = lidar_to_rect(x, y, z) and (u, v, depth) = rect_to_img(rect) are the float32 chains of csrc/common.hpp
 *   (lidar_to_rect_f32, rect_to_img_f32: the chains dfu3d_fov_filter uses and golden G7 pins), with the scene's own
 *   calibration record.  A point stays iff  0 <= u < w,  0 <= v < h  and  depth >= 0, all in float32, (h, w) the scene's
 *   own image shape.  A NaN in any comparison drops the point; a rect z of 0 goes through the division as it is.
 * BOX RULE
 *   A kept point is inside a box by the test of points_in_boxes_cpu (csrc/pt_in_box.hpp), the rule of the ground-truth
 *   database stage -- not by the reference's Delaunay hull, from which it differs only for points on a face.
 */
#ifndef DFU3D_INGEST_H
#define DFU3D_INGEST_H

#include <stddef.h>
#include <stdint.h>

#define DFU3D_ING_VERSION 1

/* rows of a compaction chunk: one workgroup of DFU3D_ING_CHUNK threads, one row per thread */
#define DFU3D_ING_CHUNK 256
/* kernel launches of one dfu3d_fov_ingest with both mode bits, whatever B: the flags and chunk counts, the scan with
 * out_off, the write (the last two only with DFU3D_ING_EMIT), the box counts (only with DFU3D_ING_COUNT) */
#define DFU3D_ING_LAUNCHES 4
/* caps: beyond them DFU3D_ERANGE */
#define DFU3D_ING_MAX_ROWS 1073741824
#define DFU3D_ING_MAX_SCENES 65535
#define DFU3D_ING_MAX_POINT_COLS 64
#define DFU3D_ING_MAX_BOXES 1048576
/* an image side beyond this is not exact in float32: DFU3D_ING_ST_SHAPE */
#define DFU3D_ING_MAX_SIDE 16777216

/* `mode` of dfu3d_fov_ingest: at least one */
#define DFU3D_ING_EMIT 1
#define DFU3D_ING_COUNT 2

/* bits of the status word */
#define DFU3D_ING_ST_OFFSETS 1
#define DFU3D_ING_ST_SHAPE 2

#ifdef __cplusplus
extern "C" {
#endif

int32_t dfu3d_ing_version(void);

/* bytes of scratch dfu3d_fov_ingest needs for n_rows point rows (two ints per chunk, one flag byte per row, slack);
 * 0 for an argument out of range */
size_t dfu3d_fov_ingest_scratch_bytes(int64_t n_rows);

/* points float32 (n_rows, C), C >= 3, 4-byte aligned (C = 4 and 16-byte aligned: one 16-byte load per row), the scenes
 * one after the other: scene b is rows point_off[b] .. point_off[b+1] (int64 (B + 1), ascending, point_off[0] = 0,
 * point_off[B] <= n_rows; rows at or beyond point_off[B] are never kept; a table that is not so sets
 * DFU3D_ING_ST_OFFSETS and no row outside [0, n_rows) is touched).
 * calib float32 (B, DFU3D_CALIB_FLOATS): one record per scene (dfu3d.h).  image_shape int32 (B, 2): (h, w) per scene,
 * 0 .. DFU3D_ING_MAX_SIDE each, else DFU3D_ING_ST_SHAPE and the scene keeps nothing.
 * boxes float64 (n_boxes, 7) (x, y, z, dx, dy, dz, heading) with box_off int32 (B + 1): scene b owns rows
 * box_off[b] .. box_off[b+1] (ascending, box_off[0] = 0, box_off[B] = n_boxes, else DFU3D_ING_ST_OFFSETS and the
 * rows no scene owns count 0).  Both are read only with DFU3D_ING_COUNT.
 *
 * DFU3D_ING_EMIT: points_out float32 (n_rows, C) gets the kept rows, all C columns bit for bit, in scene order and in
 * input order inside a scene; rows at or beyond out_off[B] are not written.  out_off int64 (B + 1): the kept rows of
 * scene b are out_off[b] .. out_off[b+1].
 * DFU3D_ING_COUNT: box_cnt int32 (n_boxes): the number of kept points of box k's scene inside box k (exact: a
 * fixed-shape integer sum).
 * status: ORed into, never cleared.  scratch: 8-byte aligned, dfu3d_fov_ingest_scratch_bytes(n_rows) bytes; every byte
 * is written before it is read.  The inputs are not written; no output may alias an input. */
int dfu3d_fov_ingest(const float *points, int64_t n_rows, int32_t C, const int64_t *point_off, int32_t B,
                     const float *calib, const int32_t *image_shape, const double *boxes, int32_t n_boxes,
                     const int32_t *box_off, int32_t mode, float *points_out, int64_t *out_off, int32_t *box_cnt,
                     void *scratch, size_t scratch_bytes, uint32_t *status, void *stream);

#ifdef __cplusplus
}
#endif

#endif
