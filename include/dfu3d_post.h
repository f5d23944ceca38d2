/* dfu3d_post.h -- C ABI of the CenterHead post-processing stage of libdfu3d_hip.so (csrc/postproc_stage.hip): rotated
 * non-maximum suppression of many box lists ("segments") at once, and the gather of the survivors of all heads into one
 * padded block per sample.  Three launches for any number of heads and samples.
 *
 * The entry points live in the same library as include/dfu3d.h's and follow its rules: device pointers, results in
 * device memory, the library never allocates and never synchronises, every call returns DFU3D_OK / DFU3D_EINVAL /
 * DFU3D_ELAUNCH / DFU3D_ERANGE (dfu3d.h) and validates its arguments on the host before any launch.  The header keeps
 * to the C subset dfu3d_amd/_header.py reads.
 *
 * The overlap of a pair is the one dfu3d_nms_bev computes (csrc/rect_overlap.hpp, the earlier row in the role of A), so
 * a pair's decision is the same bits in both.
 */
#ifndef DFU3D_POST_H
#define DFU3D_POST_H

#include <stddef.h>
#include <stdint.h>

#define DFU3D_POST_VERSION 1

/* rows of a segment at most */
#define DFU3D_POST_MAX_CAP 1024

#ifdef __cplusplus
extern "C" {
#endif

/* bytes of scratch dfu3d_nms_bev_segments needs for S segments of cap rows (the suppression masks, 16 bytes of slack);
 * 0 for an argument out of range */
size_t dfu3d_nms_segments_scratch_bytes(int32_t S, int32_t cap);

/* Greedy suppression of S box lists.  boxes float32 (S, cap, C), C >= 7, columns 0..6 = (x, y, z, dx, dy, dz, heading),
 * the rows of a segment in descending score order; count int32 (S): segment s holds n_s = clamp(count[s], 0, cap) rows,
 * rows at or beyond n_s are never read.  The first min(n_s, pre_max) rows are candidates (pre_max <= 0: all); row i is
 * suppressed iff an earlier kept row j of its segment has IoU(j, i) > thresh; the walk stops after post_max kept rows
 * (post_max <= 0: never).  normal != 0: axis-aligned IoU, headings ignored.
 * keep int32 (S, cap): the kept positions ascending, then -1 (every slot is written); num_keep int32 (S).
 * scratch: 8-byte aligned, at least dfu3d_nms_segments_scratch_bytes(S, cap) bytes.  cap > DFU3D_POST_MAX_CAP:
 * DFU3D_ERANGE.  S == 0 or cap == 0: DFU3D_OK without a launch. */
int dfu3d_nms_bev_segments(const float *boxes, int32_t S, int32_t cap, int32_t C, const int32_t *count, float thresh,
                           int32_t pre_max, int32_t post_max, int32_t normal, void *scratch, size_t scratch_bytes,
                           int32_t *keep, int32_t *num_keep, void *stream);

/* The survivors of all heads, per sample.  Segment s = h * B + b of boxes (n_heads * B, cap, C), scores and labels
 * (n_heads * B, cap), keep and num_keep as dfu3d_nms_bev_segments writes them.  cls_map int32 (n_heads, max_cls): class id
 * within the head -> 0-based id over the detector's classes.  For sample b the heads in order, within a head the kept
 * rows in `keep` order: out_boxes (B, out_cap, C) all C columns, out_scores (B, out_cap), out_labels int64 (B, out_cap)
 * = cls_map[h][label] + 1, out_count int32 (B) the number of rows, at most out_cap (rows that do not fit are dropped).
 * Rows at or beyond out_count[b] are written as 0.  A label outside [0, max_cls) or a keep entry outside [0, cap) is
 * never dereferenced: the row gets label 0 (and, for the keep entry, zeros). */
int dfu3d_center_collect(const float *boxes, const float *scores, const int32_t *labels, const int32_t *keep,
                         const int32_t *num_keep, int32_t n_heads, int32_t B, int32_t cap, int32_t C,
                         const int32_t *cls_map, int32_t max_cls, int32_t out_cap, float *out_boxes, float *out_scores,
                         int64_t *out_labels, int32_t *out_count, void *stream);

#ifdef __cplusplus
}
#endif

#endif
