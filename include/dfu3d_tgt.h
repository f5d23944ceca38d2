/* dfu3d_tgt.h -- C ABI of PointRCNN's two target-assignment steps in libdfu3d_hip.so (csrc/rcnntarget_stage.hip), each
 * for a whole batch in one kernel launch and without a read from the device:
 *
 *   dfu3d_tgt_point_targets   what OpenPCDet's PointHeadBox.assign_targets computes: per point the class label of the
 *                             first ground-truth box that holds it (-1 inside an enlarged box only, 0 outside all) and
 *                             the PointResidualCoder code of that box against the point;
 *   dfu3d_tgt_roi_max_iou     ProposalTargetLayer's get_max_iou_with_same_class, or its plain IoU matrix and row maximum:
 *                             per RoI the largest volume IoU with an eligible ground-truth box and that box's row;
 *   dfu3d_tgt_roi_sample      ProposalTargetLayer's subsample_rois with sample_bg_inds: R RoI indices per sample,
 *                             foreground first, then hard, then easy background, from random numbers the caller passes.
 *
 * The entry points live in the library of the other headers under include/ and follow its rules: device pointers, results
 * in device memory, the library never allocates, never synchronises and never reads from the device; every call returns
 * DFU3D_OK / DFU3D_EINVAL / DFU3D_ELAUNCH / DFU3D_ERANGE and validates its arguments on the host before any launch.  The
 * header keeps to the C subset dfu3d_amd/_header.py reads.
 *
 * Arithmetic: float32 unless stated, no contraction, IEEE subtract, divide and sqrt; cos, sin and log are evaluated in
 * double on the float32 argument and rounded once to float32.  Every result is exactly what a sequential restatement
 * gives (tests/rcnn_target_ref.py).
 */
#ifndef DFU3D_TGT_H
#define DFU3D_TGT_H

#include <stddef.h>
#include <stdint.h>

#define DFU3D_TGT_VERSION 1

/* elements of any one tensor of a call (B * N * 8, B * G * 8, B * M * 7, ...): at or above it DFU3D_ERANGE */
#define DFU3D_TGT_MAX_ELEMS 2147483647
/* samples of a batch: beyond it DFU3D_ERANGE */
#define DFU3D_TGT_MAX_BATCH 65535
/* RoIs of a sample in dfu3d_tgt_roi_sample (its three index lists and the keys live in LDS): beyond it DFU3D_ERANGE */
#define DFU3D_TGT_MAX_ROIS 2048
/* sampled RoIs of a sample (ROI_PER_IMAGE): beyond it DFU3D_ERANGE */
#define DFU3D_TGT_MAX_SAMPLED 4096
/* mean sizes (classes) of dfu3d_tgt_point_targets: beyond it DFU3D_ERANGE */
#define DFU3D_TGT_MAX_CLASSES 64
/* kernel launches of one call of each entry point */
#define DFU3D_TGT_POINT_LAUNCHES 1
#define DFU3D_TGT_IOU_LAUNCHES 1
#define DFU3D_TGT_SAMPLE_LAUNCHES 1
/* bit of *status: a sample of dfu3d_tgt_roi_sample had neither a foreground nor a background RoI */
#define DFU3D_TGT_STATUS_NO_ROI 1

#ifdef __cplusplus
extern "C" {
#endif

int32_t dfu3d_tgt_version(void);

/* points: float32, point n of sample b at points[(b * N + n) * pts_stride + 0 .. 2] (3 <= pts_stride <= 64: 4 for the
 * x, y, z columns of stacked (B * N, 4) coordinates, whose sample column is not read); gt_boxes float32 (B, G, 8)
 * [x, y, z, dx, dy, dz, heading, class], not written; extra_x / y / z (GT_EXTRA_WIDTH) are added to dx / dy / dz in
 * float32 for the enlarged test; mean_size float32 (K, 3) on the device, or NULL with K = 0 (use_mean_size = False).
 *
 * Per point: k = the first row of its sample, ascending, whose box holds it, e = the first whose enlarged box does; both
 * by the in-box test of the RoI pooling (margin 1e-5f):
 *     inside  <=>  !((double)|z - cz| > (double)dz / 2)  &&  (double)|lx| < (double)dx / 2 + (double)1e-5f  &&  same in y
 *     lx = sx * cosa + sy * (-sina),  ly = sx * sina + sy * cosa,  sx = x - cx,  sy = y - cy,  cosa / sina of -heading.
 * All-zero (padded) rows are tested like any other.  With c = the class column of row k:
 *     k >= 0 and 1 <= c (and c <= K when K > 0):  cls_labels = num_class == 1 ? 1 : (int64)c and, with d = max(dim, 1e-5f)
 *         taken in registers and s = mean_size[(int)c - 1],
 *         box_labels = [(bx - x) / diag, (by - y) / diag, (bz - z) / s2, log(d0 / s0), log(d1 / s1), log(d2 / s2),
 *                       cos(heading), sin(heading)],  diag = sqrt(s0 * s0 + s1 * s1);
 *         with K = 0: [bx - x, by - y, bz - z, log(d0), log(d1), log(d2), cos(heading), sin(heading)];
 *     k >= 0 and any other c (a NaN included):  cls_labels = 0, box_labels = 0;
 *     k < 0 and e >= 0:  cls_labels = -1, box_labels = 0;        neither:  cls_labels = 0, box_labels = 0.
 * cls_labels int64 (B * N), box_labels float32 (B * N, 8), gt_idx int32 (B * N) or NULL: k, -1 when there is none.
 * EVERY element of the outputs is written; the caller does not clear them.  A NaN coordinate puts a point into no box.
 * B, N, G, num_class >= 1, K >= 0, else DFU3D_EINVAL. */
int dfu3d_tgt_point_targets(const float *points, int32_t pts_stride, const float *gt_boxes, const float *mean_size,
                            int32_t B, int32_t N, int32_t G, int32_t K, int32_t num_class, float extra_x, float extra_y,
                            float extra_z, int64_t *cls_labels, float *box_labels, int32_t *gt_idx, void *stream);

/* rois float32 (B, M, 7), roi_labels int64 (B, M), gt_boxes float32 (B, G, 8) -> max_overlaps float32 (B, M),
 * gt_assignment int32 (B, M).  Eligible rows of the RoI's sample: rows 0 .. k, k the sample's last row whose eight
 * columns, summed left to right, are not zero (the trailing padding is cut, as the reference cuts it); with
 * by_class = 1 of these only the rows whose class column, truncated to int64, equals the RoI's label.
 * IoU of RoI a and row b, every operation float32:
 *     half = 0.5f * dz,  lo = z - half,  hi = z + half,  common_z = max(min(a_hi, b_hi) - max(a_lo, b_lo), 0)
 *     inter = overlap(a, b) * common_z,  vol = (dx * dy) * dz,  union = (va + vb) - inter,  iou = inter / max(union, 1e-6f)
 * overlap: the exact footprint overlap of the IoU entry points of dfu3d.h; min and max hand a NaN on.  The largest IoU
 * wins, among equal ones the lowest row; a NaN never wins.  No eligible row, or only NaNs: overlap 0, assignment 0.
 * B, M, G >= 1, by_class 0 or 1, else DFU3D_EINVAL. */
int dfu3d_tgt_roi_max_iou(const float *rois, const int64_t *roi_labels, const float *gt_boxes, int32_t B, int32_t M,
                          int32_t G, int32_t by_class, float *max_overlaps, int32_t *gt_assignment, void *stream);

/* max_overlaps float32 (B, M), rand_key int32 (B, M), rand_u float32 (B, R) in [0, 1) -> sampled_inds int32 (B, R).
 * Lists of a sample, in ascending index: fg: ov >= fg_thresh; easy: ov < bg_thresh_lo; hard: ov < reg_fg_thresh and
 * ov >= bg_thresh_lo (a NaN is in none); nf, ne, nh their lengths.  draw(list, n, j) = list[min((int)floor((double)
 * rand_u[j] * n), n - 1)] (index 0 for a rand_u that is no number or negative).
 *     nf > 0 and ne + nh > 0:  take = min(fg_per, nf); slots 0 .. take - 1 = the take members of fg with the smallest
 *                              (rand_key, index), in that order; the other R - take slots are background slots;
 *     nf > 0, no background:   every slot j = draw(fg, nf, j);
 *     nf = 0, background:      all R slots are background slots;
 *     neither:                 every slot 0 and DFU3D_TGT_STATUS_NO_ROI is OR-ed into *status.
 * `need` background slots starting at slot j0: with nh > 0 and ne > 0, h = min((int)((double)need * hard_ratio), nh);
 * slots j0 .. j0 + h - 1 = draw(hard, nh, j), the rest draw(easy, ne, j); else all from the list that is not empty.
 * status: one uint32 word that is only ever OR-ed into -- the caller zeroes it when it wants a fresh one.
 * B, M, R >= 1, 0 <= fg_per <= R, hard_ratio a number in [0, 1], else DFU3D_EINVAL; M > DFU3D_TGT_MAX_ROIS or
 * R > DFU3D_TGT_MAX_SAMPLED: DFU3D_ERANGE. */
int dfu3d_tgt_roi_sample(const float *max_overlaps, const int32_t *rand_key, const float *rand_u, int32_t B, int32_t M,
                         int32_t R, int32_t fg_per, float fg_thresh, float reg_fg_thresh, float bg_thresh_lo,
                         double hard_ratio, int32_t *sampled_inds, uint32_t *status, void *stream);

#ifdef __cplusplus
}
#endif

#endif
