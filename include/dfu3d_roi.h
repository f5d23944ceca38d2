/* dfu3d_roi.h -- C ABI of the RoI-point pooling of libdfu3d_hip.so (csrc/roipoint_stage.hip): what OpenPCDet's
 * pcdet/ops/roipoint_pool3d computes for PointRCNN's second stage -- for every RoI the first S points of its sample that
 * lie inside the (enlarged) box, in ascending point index, and their gathered rows -- in two forms behind one entry
 * point: the op's own (raw coordinates, then the features) and PointRCNNHead.roipool3d_gpu's (canonical coordinates,
 * score, depth, then the features) without the concatenated (B * N, 2 + C) tensor and the (B, N, M) assignment matrix.
 *
 * The entry points live in the same library as include/dfu3d.h's and follow its rules: device pointers, results in
 * device memory, the library never allocates, never synchronises and never reads from the device, every call returns
 * DFU3D_OK / DFU3D_EINVAL / DFU3D_ELAUNCH / DFU3D_ERANGE (dfu3d.h) and validates its arguments on the host before any
 * launch.  The header keeps to the C subset dfu3d_amd/_header.py reads.
 *
 * Arithmetic: float32, no contraction, IEEE divide and sqrt.  The in-box test is csrc/pt_in_box.hpp's with this op's
 * constants: the box read as float32, the dims with the extra width added in float32, hz = (double)dz / 2.0,
 * hx = (double)dx / 2.0 + (double)1e-5f (hy likewise), cosa / sina = cos / sin of (double)(-heading) rounded to float32:
 *     inside  <=>  !((double)|z - cz| > hz)  &&  (double)|lx| < hx  &&  (double)|ly| < hy
 *     lx = sx * cosa + sy * (-sina),  ly = sx * sina + sy * cosa,  sx = x - cx,  sy = y - cy
 * every operation rounded, the sums left to right.  Every comparison with a NaN is false, so there is no special path:
 * a point with a NaN x or y is outside every box, a box with a NaN centre x / y, heading, dx or dy is empty (the z test
 * is a rejection, as the reference's: a NaN in z, cz or dz alone rejects nothing).  Every result is exactly what a
 * sequential float32 restatement gives (tests/roipoint_ref.py).
 */
#ifndef DFU3D_ROI_H
#define DFU3D_ROI_H

#include <stddef.h>
#include <stdint.h>

#define DFU3D_ROI_VERSION 1

/* elements of any one tensor of a call (B * N * pts_stride, B * N * C, B * M * S * (3 + C), ...): at or above it
 * DFU3D_ERANGE */
#define DFU3D_ROI_MAX_ELEMS 2147483647
/* samples of a batch: beyond it DFU3D_ERANGE */
#define DFU3D_ROI_MAX_BATCH 65535
/* floats between two points of `points`: 3 for (B, N, 3), 4 for the xyz columns of stacked (B * N, 4) coordinates */
#define DFU3D_ROI_MAX_PTS_STRIDE 64
/* kernel launches of one dfu3d_roi_pool call: the search, then the gather */
#define DFU3D_ROI_LAUNCHES 2
/* leading columns of a pooled row: x, y, z in the plain form; x', y', z', score, depth in the fused form */
#define DFU3D_ROI_PREFIX_PLAIN 3
#define DFU3D_ROI_PREFIX_FUSED 5

#ifdef __cplusplus
extern "C" {
#endif

int32_t dfu3d_roi_version(void);

/* points: float32, point n of sample b at points[(b * N + n) * pts_stride + 0 .. 2] (3 <= pts_stride <=
 * DFU3D_ROI_MAX_PTS_STRIDE); features float32 (B, N, C), may be NULL when C = 0; boxes3d float32 (B, M, 7)
 * [x, y, z, dx, dy, dz, heading]; extra_x / y / z are added to dx / dy / dz (enlarge_box3d).
 *
 * pooled_idx int32 (B, M, S): the first S point indices inside the RoI, ascending; with cnt < S of them, slot k >= cnt
 * holds what slot k % cnt holds; all zeros when cnt = 0.  pooled_empty_flag int32 (B, M): 1 when cnt = 0, else 0.
 *
 * fused = 0 (RoIPointPool3dFunction.forward): pooled float32 (B, M, S, 3 + C), a row = [x, y, z, features...] of
 * the slot's point, moved as bits; scores and depth_normalizer are not looked at.
 * fused = 1 (PointRCNNHead.roipool3d_gpu): scores float32 (B, N); pooled float32 (B * M, S, 5 + C), a row =
 * [x', y', z', score, depth, features...]:
 *     sx = x - cx, sy = y - cy, z' = z - cz, x' = sx * cosa + sy * (-sina), y' = sx * sina + sy * cosa
 *     depth = sqrt(x * x + y * y + z * z) / depth_normalizer - 0.5f          (raw coordinates, left to right)
 * with the cosa / sina of the in-box test.  depth_normalizer > 0, else DFU3D_EINVAL.
 * In both forms the rows of an empty RoI are +0.0f.  EVERY element of the three outputs is written; the caller does
 * not clear them.  The three outputs must not overlap the inputs or each other.
 * B, N, M, S >= 1, C >= 0, else DFU3D_EINVAL; a tensor of DFU3D_ROI_MAX_ELEMS elements or more, or more than
 * DFU3D_ROI_MAX_BATCH samples: DFU3D_ERANGE.
 * DFU3D_ROI_LAUNCHES kernel launches, no scratch. */
int dfu3d_roi_pool(const float *points, int32_t pts_stride, const float *features, const float *scores,
                   const float *boxes3d, int32_t B, int32_t N, int32_t M, int32_t C, int32_t S, float extra_x,
                   float extra_y, float extra_z, int32_t fused, float depth_normalizer, float *pooled,
                   int32_t *pooled_empty_flag, int32_t *pooled_idx, void *stream);

#ifdef __cplusplus
}
#endif

#endif
