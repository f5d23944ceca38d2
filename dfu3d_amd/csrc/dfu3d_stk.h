/* dfu3d_stk.h -- C ABI of the stacked set-abstraction ops of libdfu3d_hip.so (csrc/pointstack_stage.hip): what
 * OpenPCDet's pcdet/ops/pointnet2/pointnet2_stack computes for PV-RCNN -- per-sample counts of a stacked tensor,
 * farthest point sampling over stacked samples, ball query, query-and-group -- and the bilinear BEV sampling of
 * VoxelSetAbstraction.interpolate_from_bev_features.
 *
 * The entry points live in the same library as include/dfu3d.h's and follow its rules: device pointers, results in
 * device memory, the library never allocates and never synchronises, every call returns DFU3D_OK / DFU3D_EINVAL /
 * DFU3D_ELAUNCH / DFU3D_ERANGE (dfu3d.h) and validates its arguments on the host before any launch.  The header keeps
 * to the C subset dfu3d_amd/_header.py reads.
 *
 * Layouts are the reference's stacked ones: the rows of all samples one after the other, sample 0 first.  A set of
 * coordinates is a pointer to the x of row 0 and a row stride in floats (>= 3): (N, 3) has stride 3, columns 1..3 of
 * `points` (N, 1 + 3 + C) are points + 1 with stride 4 + C.  The rows of sample b are start[b] .. start[b + 1]:
 * start int32 (B + 1) in device memory, as dfu3d_stk_counts / dfu3d_stk_starts leave it; no call needs a count on the
 * host.  A start array that is not ascending inside [0, rows] is clamped to that (nothing is read out of bounds) and
 * sets DFU3D_STK_ST_BAD_COUNT.  Indices int32, SAMPLE-LOCAL (row start[b] + i), as in the reference.
 * Arithmetic: no contraction, IEEE divide; the squared distance is dfu3d_pn2.h's, every operation rounded to float32
 * -- every integer result below is exactly what a sequential float32 restatement gives (tests/point_stack_ref.py).
 * status: one uint32 in device memory, ORed into, never cleared.
 */
#ifndef DFU3D_STK_H
#define DFU3D_STK_H

#include <stddef.h>
#include <stdint.h>

#define DFU3D_STK_VERSION 1

/* rows * stride of any stacked tensor, and elements of any output: beyond it DFU3D_ERANGE */
#define DFU3D_STK_MAX_ELEMS 2147483647
/* samples of a batch: beyond it DFU3D_ERANGE */
#define DFU3D_STK_MAX_BATCH 65535
/* (radius, nsample) pairs of one dfu3d_stk_ball_query call (= DFU3D_PN2_MAX_SCALES): beyond it DFU3D_EINVAL */
#define DFU3D_STK_MAX_SCALES 2
/* rows of a sample dfu3d_stk_fps keeps in registers (= DFU3D_PN2_FPS_ONCHIP) */
#define DFU3D_STK_FPS_ONCHIP 16384

/* bits of the status word */
#define DFU3D_STK_ST_BAD_POINT 1    /* a non-finite coordinate in farthest point sampling */
#define DFU3D_STK_ST_BAD_INDEX 2    /* an index outside its sample */
#define DFU3D_STK_ST_BAD_BATCH 4    /* a sample index outside [0, B) */
#define DFU3D_STK_ST_UNSORTED 8     /* rows not in ascending sample order */
#define DFU3D_STK_ST_EMPTY 16       /* farthest point sampling of a sample without rows */
#define DFU3D_STK_ST_BAD_COUNT 32   /* starts not ascending inside [0, rows], or a sample beyond the caller's cap */

#ifdef __cplusplus
extern "C" {
#endif

int32_t dfu3d_stk_version(void);

/* Counts and starts from a batch column: col is column 0 of rows of `stride` elements -- float32 (is_int = 0: points,
 * keypoints) or int32 (is_int = 1: the indices (N, 4) of a sparse tensor).  cnt int32 (B): the rows of every sample;
 * start int32 (B + 1): their exclusive prefix, start[B] the rows counted.  A value outside [0, B) (or not an integer)
 * sets DFU3D_STK_ST_BAD_BATCH and the row is not counted; a row whose value is below the row before's sets
 * DFU3D_STK_ST_UNSORTED.  Integer atomics only: the result does not depend on their order.  rows may be 0 (all
 * zeros; col is not read).  B >= 1, stride >= 1, else DFU3D_EINVAL. */
int dfu3d_stk_counts(const void *col, int32_t is_int, int64_t rows, int32_t stride, int32_t B, int32_t *cnt,
                     int32_t *start, uint32_t *status, void *stream);

/* start (B + 1) from cnt (B) alone: the exclusive prefix, a negative count taken as 0 (DFU3D_STK_ST_BAD_COUNT). */
int dfu3d_stk_starts(const int32_t *cnt, int32_t B, int32_t *start, uint32_t *status, void *stream);

/* bytes of scratch of dfu3d_stk_fps: 0 when the bound on a sample -- cap if 1 <= cap < rows, else rows -- is at most
 * DFU3D_STK_FPS_ONCHIP, one float32 per row beyond; -1 for arguments out of range */
int64_t dfu3d_stk_fps_scratch_bytes(int64_t rows, int32_t cap);

/* Stacked farthest point sampling, the FPS of VoxelSetAbstraction.get_sampled_points for the whole batch: one
 * workgroup per sample over start.  The picks of a sample are those of dfu3d_pn2_fps on that sample alone (first pick
 * 0, the lowest index among equal maxima).  idx int32 (B, K), sample-local; keypoints float32 (B * K, 4), row
 * b * K + j = [b, x, y, z] of pick j.  A sample of n < K rows repeats its n picks: idx[j] = idx[j mod n].  n = 0 sets
 * DFU3D_STK_ST_EMPTY and writes index 0 and [b, 0, 0, 0].  cap: a bound on the rows of one sample the caller knows
 * (0: none, the bound is rows); a sample beyond the bound sets DFU3D_STK_ST_BAD_COUNT and only its first `bound` rows
 * are sampled.  A non-finite coordinate sets DFU3D_STK_ST_BAD_POINT; the picks are then unspecified, but inside the
 * sample.  K >= 1, rows >= 0, stride >= 3, else DFU3D_EINVAL.
 * scratch: dfu3d_stk_fps_scratch_bytes(rows, cap) bytes, may be NULL when that is 0. */
int dfu3d_stk_fps(const float *xyz, int32_t stride, int64_t rows, const int32_t *start, int32_t B, int32_t K,
                  int32_t cap, int32_t *idx, float *keypoints, void *scratch, uint32_t *status, void *stream);

/* Stacked ball query, ball_query_kernel_stack with the wrapper's clean-up folded in, for up to DFU3D_STK_MAX_SCALES
 * (radius, nsample) pairs in ONE launch: xyz N rows over start, centres M rows over cstart.  For scale s idx_s int32
 * (M, nsample_s): the first nsample_s sample-local indices in ascending order with d2 < radius_s * radius_s (strict;
 * the product in float32) among the rows of the centre's OWN sample, the remaining slots the first hit; empty_s uint8
 * (M): 1 for a ball without a hit, whose slots are all 0.  Every element is written.  The sample of a centre is found
 * in cstart; a centre beyond cstart[B] is an empty ball (DFU3D_STK_ST_BAD_COUNT).  N or M may be 0 (M = 0: nothing is launched, the outputs may be NULL).  n_scales 1 or 2;
 * the arguments of scale 1 are ignored for n_scales = 1.  nsample_s >= 1, radius_s not NaN, else DFU3D_EINVAL. */
int dfu3d_stk_ball_query(const float *xyz, int32_t stride, int64_t N, const int32_t *start, const float *centres,
                         int32_t cstride, int64_t M, const int32_t *cstart, int32_t B, int32_t n_scales, float radius0,
                         int32_t nsample0, int32_t *idx0, uint8_t *empty0, float radius1, int32_t nsample1,
                         int32_t *idx1, uint8_t *empty1, uint32_t *status, void *stream);

/* QueryAndGroup.forward behind the ball query, for one scale: out float32 (3 + C, M, nsample), contiguous -- the order
 * a 1x1 convolution reads.  Channels 0..2: xyz[start[b] + idx] - centre (the only float operation); channels 3..:
 * features (N, C) of that row, moved as bits.  A ball with empty = 1 is all zeros.  features NULL or C = 0: the three
 * xyz channels only.  xyz and centres both NULL (C >= 1): the plain grouping_operation, out (C, M, nsample), N the
 * rows of features.  An index outside its sample sets DFU3D_STK_ST_BAD_INDEX and reads the sample's row 0 (an empty
 * sample: zeros). */
int dfu3d_stk_group(const float *xyz, int32_t stride, int64_t N, const int32_t *start, const float *centres,
                    int32_t cstride, int64_t M, const int32_t *cstart, int32_t B, const float *features, int32_t C,
                    const int32_t *idx, const uint8_t *empty, int32_t nsample, float *out, uint32_t *status,
                    void *stream);

/* The index tensor of the grouping backward: gidx int32 (M * nsample) = start[b] + idx, the GLOBAL row of every
 * entry, and -1 for the entries of an empty ball and for an index outside its sample (that one sets
 * DFU3D_STK_ST_BAD_INDEX).  A centre beyond cstart[B] sets DFU3D_STK_ST_BAD_COUNT as in dfu3d_stk_group, whatever its
 * empty flag.  dfu3d_pn2_invert(gidx, 1, N, M * nsample, ...) leaves the -1 entries out and
 * dfu3d_pn2_gather_backward(grad_out + 3 * M * nsample, NULL, csr, list, 1, C, N, ...) sums the rest in ascending entry
 * number: grad_features as (C, N). */
int dfu3d_stk_global_index(const int32_t *idx, const uint8_t *empty, int64_t M, int32_t nsample, int64_t N,
                           const int32_t *start, const int32_t *cstart, int32_t B, int32_t *gidx, uint32_t *status,
                           void *stream);

/* Bilinear BEV sampling, interpolate_from_bev_features for the whole batch: keypoints M rows of kstride floats
 * [b, x, y, ...], spatial float32 (B, C, H, W) read in place, out float32 (M, C).  In float32, operation by operation:
 *     fx = ((x - range_x) / voxel_x) / bev_stride (true divisions), fy likewise;
 *     x0 = floor(fx), x1 = x0 + 1, both clamped to [0, W - 1]; y0, y1 likewise in [0, H - 1];
 *     wa = (x1 - fx) * (y1 - fy), wb = (x1 - fx) * (fy - y0), wc = (fx - x0) * (y1 - fy), wd = (fx - x0) * (fy - y0)
 *     out = I[y0, x0] * wa + I[y1, x0] * wb + I[y0, x1] * wc + I[y1, x1] * wd, summed left to right.
 * A sample index outside [0, B) sets DFU3D_STK_ST_BAD_BATCH and the row is zeros; a non-finite fx (NaN, +inf, -inf)
 * takes x0 = x1 = 0 and a non-finite fy y0 = y1 = 0, as the reference's floor().long() and clamp give on the host.
 * M >= 1, C, H, W >= 1, kstride >= 3, else DFU3D_EINVAL. */
int dfu3d_stk_bev_sample(const float *keypoints, int32_t kstride, int64_t M, const float *spatial, int32_t B, int32_t C,
                         int32_t H, int32_t W, float range_x, float range_y, float voxel_x, float voxel_y,
                         float bev_stride, float *out, uint32_t *status, void *stream);

#ifdef __cplusplus
}
#endif

#endif
