/* dfu3d_prop.h -- C ABI of PointRCNN's proposal stage in libdfu3d_hip.so (csrc/proposal_stage.hip): what
 * PointRCNNHead.proposal_layer computes sample by sample -- the NMS_PRE_MAXSIZE best points by score, their rotated NMS,
 * the first NMS_POST_MAXSIZE survivors and the padded RoI block -- for a whole batch in DFU3D_PROP_LAUNCHES kernel
 * launches and without a read from the device.
 *
 * The entry points live in the library of the headers under include/ and follow its rules: device pointers, results in
 * device memory, the library never allocates, never synchronises and never reads from the device; every call returns
 * DFU3D_OK / DFU3D_EINVAL / DFU3D_ELAUNCH / DFU3D_ERANGE and validates its arguments on the host before any launch.  The
 * header keeps to the C subset dfu3d_amd/_header.py reads.  (It sits next to the sources and not under include/ because
 * the set of files there is pinned by an existing test: INTEGRATION.md.)
 *
 * THE ORDER RULE.  Per sample the K = min(pre_max, N) best points, best first, under one total order:
 *     key(s)  = the monotone uint32 image of the float32 score s: -0.0 is taken as +0.0; every NaN, whatever its sign and
 *               payload, maps to the one key 0xFFFFFFFF, above the key of +inf (0xFF800000); any other s with bits u maps
 *               to ~u when its sign bit is set and to u | 0x80000000 when not;
 *     point i comes before point j  <=>  key(s_i) > key(s_j), or key(s_i) == key(s_j) and i < j.
 * The result is a pure function of the input, and equals torch.topk's wherever the scores are distinct.
 *
 * THE SUPPRESSION.  The candidates are walked in that order.  A candidate is kept unless an EARLIER KEPT candidate A
 * suppresses it: IoU of the footprints (the exact polygon overlap of the NMS of dfu3d.h, A the earlier row: the same
 * bits) > thresh.  The walk ends after K candidates or as soon as post_max are kept, so a candidate is tested against
 * at most post_max boxes.  The first post_max survivors of the full greedy walk are the survivors of the walk that stops
 * there: the result is that of nms_gpu on the sorted boxes cut to post_max.
 */
#ifndef DFU3D_PROP_H
#define DFU3D_PROP_H

#include <stddef.h>
#include <stdint.h>

#define DFU3D_PROP_VERSION 1

/* kernel launches of one call of dfu3d_proposals, for any B: the order, then the suppression with the gather */
#define DFU3D_PROP_LAUNCHES 2
/* post_max (NMS_POST_MAXSIZE) at most: the kept boxes of a sample live in LDS.  Beyond it DFU3D_ERANGE */
#define DFU3D_PROP_MAX_POST 1024
/* points of a sample at most (one workgroup sorts a sample).  Beyond it DFU3D_ERANGE */
#define DFU3D_PROP_MAX_POINTS 16384
/* samples of a batch at most.  Beyond it DFU3D_ERANGE */
#define DFU3D_PROP_MAX_BATCH 65535
/* elements of the box block, B * N * C, and of the RoI block, B * post_max * C, at most.  Beyond it DFU3D_ERANGE */
#define DFU3D_PROP_MAX_ELEMS 2147483647

/* The shape of the two kernels, stated here because their LDS follows from it (tests/test_kernel_resources_proposals.py):
 * threads of the workgroup that sorts a sample; candidates the suppression takes at a time (one per lane of a wave);
 * pairs its queue of polygon clips holds (2 bytes each: what the rest of its LDS leaves of 64 KiB) */
#define DFU3D_PROP_SORT_THREADS 1024
#define DFU3D_PROP_BLOCK_ROWS 64
#define DFU3D_PROP_QUEUE_PAIRS 2936

#ifdef __cplusplus
extern "C" {
#endif

int32_t dfu3d_prop_version(void);

/* Bytes of scratch dfu3d_proposals needs for these sizes: two (key, index) buffers of N entries per sample for the
 * sort to alternate between, and the order int32 (B, min(pre_max, N)), rounded up to 16.  0 for B = 0 or N = 0 (nothing
 * is launched then) and for arguments out of range (negative sizes, pre_max < 1, N > DFU3D_PROP_MAX_POINTS,
 * B > DFU3D_PROP_MAX_BATCH). */
size_t dfu3d_prop_scratch_bytes(int32_t B, int32_t N, int32_t pre_max);

/* scores float32 (B, N); labels int64 (B, N), 0-based; boxes float32 (B, N, C), C >= 7, columns 0 .. 6 = x, y, z, dx, dy,
 * dz, heading, the others copied along; none is written.  scratch: 16-byte aligned, dfu3d_prop_scratch_bytes(B, N,
 * pre_max) bytes at least, its content on entry does not matter.
 *
 * With r_0, r_1, ... the points of sample b that survive (the rules above) and n = their number (<= post_max):
 *     rois          float32 (B, post_max, C)   row k = boxes[b, r_k, :]             rows k >= n: 0
 *     roi_scores    float32 (B, post_max)      scores[b, r_k]                                   0
 *     roi_labels    int64   (B, post_max)      labels[b, r_k] + 1                               1
 *     roi_point_idx int64   (B, post_max)      r_k                                              -1
 *     num_rois      int32   (B)                n
 * EVERY element of the outputs is written; the caller clears nothing.  Floats are copies: the same bits.
 *
 * A null pointer, C < 7, B < 0, N < 0, pre_max < 1, a scratch that is not 16-byte aligned or too short: DFU3D_EINVAL.
 * post_max outside 1 .. DFU3D_PROP_MAX_POST, N > DFU3D_PROP_MAX_POINTS, B > DFU3D_PROP_MAX_BATCH, B * N * C or
 * B * post_max * C > DFU3D_PROP_MAX_ELEMS: DFU3D_ERANGE.  B == 0 or N == 0: DFU3D_OK and nothing is launched or written. */
int dfu3d_proposals(const float *scores, const int64_t *labels, const float *boxes, int32_t B, int32_t N, int32_t C,
                    float thresh, int32_t pre_max, int32_t post_max, void *scratch, size_t scratch_bytes, float *rois,
                    float *roi_scores, int64_t *roi_labels, int64_t *roi_point_idx, int32_t *num_rois, void *stream);

#ifdef __cplusplus
}
#endif

#endif
