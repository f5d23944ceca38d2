/* dfu3d_aug.h -- C ABI of the world-augmentation stage of libdfu3d_hip.so (csrc/worldaug_stage.hip): what OpenPCDet does
 * to a scene between the ground-truth sampler and the model's batch_dict -- random_world_flip / _rotation / _scaling /
 * _translation, the heading wrap, the class filter with its class column, mask_points_and_boxes_outside_range and
 * collate_batch -- for a whole batch in four launches.
 *
 * The entry points live in the same library as include/dfu3d.h's and follow its rules: device pointers, results in
 * device memory, the library never allocates and never synchronises, every call returns DFU3D_OK / DFU3D_EINVAL /
 * DFU3D_ELAUNCH / DFU3D_ERANGE (dfu3d.h) and validates its arguments on the host before any launch.  The header keeps
 * to the C subset dfu3d_amd/_header.py reads.
 *
 * Nothing random happens here: the host draws every scene's parameters and fills one record per scene.
 */
#ifndef DFU3D_AUG_H
#define DFU3D_AUG_H

#include <stddef.h>
#include <stdint.h>

#define DFU3D_AUG_VERSION 1

/* rows of a compaction chunk (one workgroup) */
#define DFU3D_AUG_CHUNK 1024
/* caps: beyond them DFU3D_ERANGE */
#define DFU3D_AUG_MAX_ROWS 1073741824
#define DFU3D_AUG_MAX_SCENES 65535
#define DFU3D_AUG_MAX_POINT_COLS 64
#define DFU3D_AUG_MAX_BOX_CAP 65536

/* dfu3d_aug_params.flags: the steps of a scene, applied in this order */
#define DFU3D_AUG_FLIP_X 1
#define DFU3D_AUG_FLIP_Y 2
#define DFU3D_AUG_ROTATE 4
#define DFU3D_AUG_SCALE 8
#define DFU3D_AUG_TRANSLATE 16
#define DFU3D_AUG_WRAP 32
/* the flip along y comes before the flip along x (ALONG_AXIS_LIST ['y', 'x']); it matters for the heading only */
#define DFU3D_AUG_FLIP_Y_FIRST 64

/* `mode` of dfu3d_world_aug_collate */
#define DFU3D_AUG_MASK_POINTS 1
#define DFU3D_AUG_MASK_BOXES 2
#define DFU3D_AUG_FILTER_CLASS 4

/* bits of the status word */
#define DFU3D_AUG_ST_NONFINITE 1
#define DFU3D_AUG_ST_BOX_CAP 2
#define DFU3D_AUG_ST_OFFSETS 4

/* One scene's drawn values.  cos_a / sin_a: cosine and sine of float32(noise_rot), formed in float32 on the host.
 * scale_f / noise_rot_f: float32(scale), float32(noise_rot): what a float32 array is multiplied by / gets added.
 * tx, ty, tz: the float32 translation.  noise_rot, scale: the values as drawn, for float64 boxes. */
typedef struct dfu3d_aug_params {
  uint32_t flags;
  float cos_a, sin_a;
  float scale_f;
  float noise_rot_f;
  float tx, ty, tz;
  double noise_rot;
  double scale;
} dfu3d_aug_params;

#ifdef __cplusplus
extern "C" {
#endif

int32_t dfu3d_aug_version(void);

/* bytes of scratch dfu3d_world_aug_collate needs for n_rows point rows (two ints per chunk, 16 bytes of slack);
 * 0 for an argument out of range */
size_t dfu3d_world_aug_scratch_bytes(int64_t n_rows);

/* points float32 (n_rows, C), C >= 3, the scenes one after the other: scene b is rows point_off[b] .. point_off[b+1]
 * (int64 (B + 1), ascending, point_off[0] = 0, point_off[B] <= n_rows: n_rows is the array's capacity, as the
 * ground-truth sampler's output has one, and rows at or beyond point_off[B] are never read; an offset table that is not
 * so sets DFU3D_AUG_ST_OFFSETS and no row outside [0, n_rows) is touched).
 * boxes: float32 (box_f64 = 0) or float64 (box_f64 != 0) values (n_box_rows, box_cols), box_cols 7 or 9
 * (x, y, z, dx, dy, dz, heading[, vx, vy]); scene b owns rows box_off[b] .. box_off[b] + box_cnt[b] (int32; box_off
 * (B + 1), box_cnt (B), box_cnt[b] <= box_off[b+1] - box_off[b]); box_cls int32 (n_box_rows): the class id of a row, 1-based,
 * 0 = not in class_names.  params: dfu3d_aug_params (B) in DEVICE memory.  range float32 (6) in device memory:
 * (x_min, y_min, z_min, x_max, y_max, z_max).
 *
 * Per scene, in the order of the flag values: flips, rotation (x' = fma(y, -s, x c), y' = fma(y, c, x s) in float32),
 * scaling, translation; boxes also the heading wrap h - floor(h / float32(2 pi) + 0.5f) * float32(2 pi) in float32.
 * DFU3D_AUG_MASK_POINTS: a point is kept iff x_min <= x <= x_max and y_min <= y <= y_max; a point whose x or y is
 * not finite fails that test and sets DFU3D_AUG_ST_NONFINITE.  DFU3D_AUG_FILTER_CLASS: rows of class id <= 0 are dropped.
 * DFU3D_AUG_MASK_BOXES: a box is kept iff its centre lies in the closed 3-D range.
 *
 * points_out float32 (n_rows, 1 + C): the kept rows in input order, column 0 = the scene's index; rows at or
 * beyond n_kept[0] are (-1, 0, ..., 0).  n_kept int32 (1).  point_cnt int32 (B): kept rows per scene.
 * gt_boxes_out float32 (B, box_cap, box_cols + 1): the kept boxes of a scene in input order, last column = the class id;
 * every slot behind them is 0.  gt_cnt int32 (B).  Kept boxes beyond box_cap are dropped and set DFU3D_AUG_ST_BOX_CAP.
 * boxes_aug (may be NULL): the transformed rows in the input's type and layout (n_box_rows, box_cols), nothing dropped;
 * box_keep (may be NULL) int32 (n_box_rows): 1 where the row passed the class filter and the box mask.
 * status: ORed into, never cleared.  scratch: 8-byte aligned, dfu3d_world_aug_scratch_bytes(n_rows) bytes.
 * The inputs are not written; no output may alias an input. */
int dfu3d_world_aug_collate(const float *points, int64_t n_rows, int32_t C, const int64_t *point_off, int32_t B,
                            const void *boxes, int32_t box_f64, int32_t box_cols, int64_t n_box_rows,
                            const int32_t *box_off, const int32_t *box_cnt, const int32_t *box_cls,
                            const dfu3d_aug_params *params, const float *range, int32_t mode, float *points_out,
                            int32_t *n_kept, int32_t *point_cnt, float *gt_boxes_out, int32_t box_cap, int32_t *gt_cnt,
                            void *boxes_aug, int32_t *box_keep, void *scratch, size_t scratch_bytes, uint32_t *status,
                            void *stream);

#ifdef __cplusplus
}
#endif

#endif
