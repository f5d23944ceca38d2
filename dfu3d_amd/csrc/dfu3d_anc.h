/* dfu3d_anc.h -- C ABI of the anchor target assignment in libdfu3d_hip.so (csrc/anchor_stage.hip): what
 * AxisAlignedTargetAssigner.assign_targets computes sample by sample and anchor class by anchor class -- the nearest-BEV
 * IoU of every anchor with the boxes of its class, the two maxima, the labels, the encoded regression targets and their
 * weights -- for a whole batch in DFU3D_ANC_LAUNCHES kernel launches and without a read from the device.
 *
 * The entry points live in the library of the headers under include/ and follow its rules: results in device memory, the
 * library never allocates, never synchronises and never reads from the device; every call returns DFU3D_OK /
 * DFU3D_EINVAL / DFU3D_ELAUNCH / DFU3D_ERANGE and validates its arguments on the host before any launch.  The header
 * keeps to the C subset dfu3d_amd/_header.py reads.  (It sits next to the sources and not under include/ because the set
 * of files there is pinned by an existing test: INTEGRATION.md.)
 *
 * THE CONTRACT is the reference's assign_targets for POS_FRACTION < 0 (no sampling), NORM_BY_NUM_EXAMPLES: False,
 * MATCH_HEIGHT: False and no multihead; no configuration the reference ships uses the first three otherwise, and only
 * its five *_multihead.yaml files the last.  Boxes and anchors are finite.
 *
 * ANCHORS AND CLASS SETS.  anchors is the head's flattened block (A, 7): locations in y, x order, and at every location
 * per_loc anchors, the class sets one after another, each with its sizes x rotations.  The sets are given by their
 * EXTENTS at a location: set s owns the slots set_begin[s] .. set_begin[s + 1] - 1 of every location (set_begin[0] = 0,
 * set_begin[S] = per_loc), so anchor a belongs to the set of slot a % per_loc.  Set s takes the boxes of the 1-based class
 * class_id[s], and anchors of its own only.
 *
 * THE BOXES OF A SAMPLE.  gt_boxes (B, M, 8) = x, y, z, dx, dy, dz, heading, class.  Trailing rows whose first seven
 * values sum to 0 (float32, left to right) are cut, but row 0 always stays; interior zero rows stay.  The class is the
 * float truncated to an integer.  A row of class 0 belongs to the LAST class set (the reference's class_names[c - 1]);
 * a row of a class no set takes is matched against nothing.
 *
 * THE IoU of an anchor and a box is boxes3d_nearest_bev_iou in float32, operation by operation: r = |h - floor(h /
 * (float)pi + 0.5) * (float)pi|; r < (float)(pi / 4) takes (dx, dy), else (dy, dx); corners = centre -+ dims / 2; then
 * the max / min / clamp / product / clamp_min(union, 1e-6) / divide of boxes_iou_normal.  One device function states it.
 *
 * PER ANCHOR: best = the largest IoU over the boxes of its set, arg = the lowest box row that has it.
 * PER BOX:    top = the largest IoU over the anchors of its set.  top == 0 forces nothing; otherwise EVERY anchor whose
 *             IoU with the box equals top is forced.
 * LABEL:      class of box arg if the anchor is forced or best >= matched[s]; else 0 if best < unmatched[s]; else -1.
 *             A forced anchor takes the class and the target of ITS OWN arg, not of the box that forced it.  In a
 *             (sample, set) without a box every anchor is 0.
 * TARGET:     ResidualCoder.encode_torch(box arg, anchor) for labels > 0 (dims clamped to 1e-5), zeros elsewhere.
 * WEIGHT:     1.0 for labels > 0, 0 elsewhere.
 * Labels and weights are a pure function of the input; so are the targets (no float atomics: two runs, the same bits).
 */
#ifndef DFU3D_ANC_H
#define DFU3D_ANC_H

#include <stddef.h>
#include <stdint.h>

#define DFU3D_ANC_VERSION 1

/* kernel launches of one call of dfu3d_anchor_targets, for any B: the box lists, the per-box maxima, the outputs */
#define DFU3D_ANC_LAUNCHES 3
/* class sets at most (they travel as a kernel argument).  Beyond it DFU3D_ERANGE */
#define DFU3D_ANC_MAX_SETS 8
/* boxes of a sample at most, M (a sample's lists live in LDS).  Beyond it DFU3D_ERANGE */
#define DFU3D_ANC_MAX_BOXES 512
/* samples of a batch at most.  Beyond it DFU3D_ERANGE */
#define DFU3D_ANC_MAX_BATCH 65535
/* elements of the target block, B * A * 7, at most.  Beyond it DFU3D_ERANGE */
#define DFU3D_ANC_MAX_ELEMS 2147483647

/* The shape of the kernels, stated here because their LDS follows from it (tests/test_kernel_resources_anchor_target.py):
 * anchors of a workgroup of the two streaming kernels, one per thread */
#define DFU3D_ANC_THREADS 256

#ifdef __cplusplus
extern "C" {
#endif

int32_t dfu3d_anc_version(void);

/* Bytes of scratch dfu3d_anchor_targets needs for these sizes: per sample DFU3D_ANC_MAX_SETS + 1 list offsets and, per
 * box row, its BEV rectangle (16 bytes), its row, its class and its top IoU (4 bytes each); every part rounded up to 16.
 * A does not enter.  0 for B = 0, and for arguments out of range (negative sizes, M > DFU3D_ANC_MAX_BOXES,
 * B > DFU3D_ANC_MAX_BATCH). */
size_t dfu3d_anc_scratch_bytes(int32_t B, int32_t A, int32_t M);

/* DEVICE: anchors float32 (A, 7); gt_boxes float32 (B, M, 8); neither is written.  scratch: 16-byte aligned,
 * dfu3d_anc_scratch_bytes(B, A, M) bytes at least, its content on entry does not matter.
 * HOST, read during the call: set_begin int32 (S + 1); matched, unmatched float32 (S); class_id int32 (S).
 *
 *     box_cls_labels  int32   (B, A)
 *     box_reg_targets float32 (B, A, 7)
 *     reg_weights     float32 (B, A)
 * EVERY element of the outputs is written; the caller clears nothing.
 *
 * A null pointer (gt_boxes may be null for M = 0), A < 0, B < 0, M < 0, S < 1, per_loc < 1, A no multiple of per_loc,
 * set_begin not ascending strictly from 0 to per_loc, a threshold that is not finite, unmatched[s] > matched[s],
 * class_id[s] < 1 or equal to another set's, a scratch that is not 16-byte aligned or too short: DFU3D_EINVAL.
 * S > DFU3D_ANC_MAX_SETS, M > DFU3D_ANC_MAX_BOXES, B > DFU3D_ANC_MAX_BATCH, B * A * 7 > DFU3D_ANC_MAX_ELEMS:
 * DFU3D_ERANGE.  B == 0 or A == 0: DFU3D_OK and nothing is launched or written. */
int dfu3d_anchor_targets(const float *anchors, int32_t A, int32_t per_loc, const int32_t *set_begin, const float *matched,
                         const float *unmatched, const int32_t *class_id, int32_t S, const float *gt_boxes, int32_t B,
                         int32_t M, void *scratch, size_t scratch_bytes, int32_t *box_cls_labels, float *box_reg_targets,
                         float *reg_weights, void *stream);

#ifdef __cplusplus
}
#endif

#endif
