/* dfu3d_pn2.h -- C ABI of the PointNet++ set-abstraction ops of libdfu3d_hip.so (csrc/pointnet2_stage.hip): what
 * OpenPCDet's pcdet/ops/pointnet2/pointnet2_batch computes -- farthest point sampling, ball query, grouping, the three
 * nearest neighbours, three-point interpolation -- and ONE backward for both gathers that uses no float atomics.
 *
 * The entry points live in the same library as include/dfu3d.h's and follow its rules: device pointers, results in
 * device memory, the library never allocates and never synchronises, every call returns DFU3D_OK / DFU3D_EINVAL /
 * DFU3D_ELAUNCH / DFU3D_ERANGE (dfu3d.h) and validates its arguments on the host before any launch.  The header keeps
 * to the C subset dfu3d_amd/_header.py reads.
 *
 * Layouts are the reference's: coordinates float32 (B, N, 3), features float32 (B, C, N), indices int32; everything
 * contiguous.  Arithmetic: no contraction, IEEE divide and sqrt; a squared distance is
 *     (a.x-b.x)*(a.x-b.x) + (a.y-b.y)*(a.y-b.y) + (a.z-b.z)*(a.z-b.z)
 * every operation rounded to float32, summed left to right -- every integer result below is exactly what a sequential
 * float32 restatement gives (tests/pointnet2_ref.py).
 * status: one uint32 in device memory, ORed into, never cleared.
 */
#ifndef DFU3D_PN2_H
#define DFU3D_PN2_H

#include <stddef.h>
#include <stdint.h>

#define DFU3D_PN2_VERSION 1

/* points of one sample (N, M, n, m of every entry point): beyond it DFU3D_ERANGE */
#define DFU3D_PN2_MAX_POINTS 1048576
/* samples of a batch: beyond it DFU3D_ERANGE */
#define DFU3D_PN2_MAX_BATCH 65535
/* elements of any one tensor of a call (B * C * M * nsample, B * E, ...): beyond it DFU3D_ERANGE */
#define DFU3D_PN2_MAX_ELEMS 2147483647
/* (radius, nsample) pairs of one dfu3d_pn2_ball_query call: beyond it DFU3D_EINVAL */
#define DFU3D_PN2_MAX_SCALES 2
/* points of a sample dfu3d_pn2_fps keeps in registers; a larger sample takes the form that keeps the running minima in
 * the scratch (the same results) */
#define DFU3D_PN2_FPS_ONCHIP 16384

/* bits of the status word */
#define DFU3D_PN2_ST_BAD_POINT 1
#define DFU3D_PN2_ST_BAD_INDEX 2
#define DFU3D_PN2_ST_BAD_BATCH 4

#ifdef __cplusplus
extern "C" {
#endif

int32_t dfu3d_pn2_version(void);

/* bytes of scratch of dfu3d_pn2_fps for xyz (B, N, 3) -- 0 up to DFU3D_PN2_FPS_ONCHIP points, one float32 per point
 * beyond -- (E = 0), or of dfu3d_pn2_invert for idx (B, E) over N sources (E >= 1); -1 for arguments out of range */
int64_t dfu3d_pn2_scratch_bytes(int32_t B, int32_t N, int64_t E);

/* Farthest point sampling, farthest_point_sampling_kernel with gather_operation on xyz folded in: idx int32
 * (B, npoint), new_xyz float32 (B, npoint, 3) = xyz[idx].  The first pick is index 0; the running minimum of every
 * point starts at 1e10f and becomes d < min ? d : min with d the squared distance to the last pick; every later pick
 * is the point of the largest running minimum.  Among equal maxima THE LOWEST POINT INDEX WINS (the reference's choice
 * depends on its block size; for inputs without exact ties the two agree).
 * 1 <= npoint <= N, else DFU3D_EINVAL; N <= DFU3D_PN2_MAX_POINTS, else DFU3D_ERANGE.  A non-finite coordinate sets
 * DFU3D_PN2_ST_BAD_POINT; the indices written are then unspecified, but always inside [0, N).
 * scratch: dfu3d_pn2_scratch_bytes(B, N, 0) bytes, may be NULL when that is 0. */
int dfu3d_pn2_fps(const float *xyz, int32_t B, int32_t N, int32_t npoint, int32_t *idx, float *new_xyz, void *scratch,
                  uint32_t *status, void *stream);

/* Ball query, ball_query_kernel_fast for up to DFU3D_PN2_MAX_SCALES (radius, nsample) pairs in ONE launch: xyz
 * (B, N, 3), centres (B, M, 3); for scale s idx_s int32 (B, M, nsample_s): the first nsample_s point indices in
 * ascending order with d2 < radius_s * radius_s (strict; the product in float32), the remaining slots the first hit,
 * all zeros without a hit.  Every element of idx_s is written.  n_scales 1 or 2; the arguments of scale 1 are ignored
 * for n_scales = 1.  nsample_s >= 1 and radius_s not NaN, else DFU3D_EINVAL. */
int dfu3d_pn2_ball_query(const float *xyz, const float *centres, int32_t B, int32_t N, int32_t M, int32_t n_scales,
                         float radius0, int32_t nsample0, int32_t *idx0, float radius1, int32_t nsample1,
                         int32_t *idx1, void *stream);

/* QueryAndGroup.forward for one scale: idx int32 (B, M, nsample) into N points; out float32
 * (B, (use_xyz ? 3 : 0) + C, M, nsample): channels 0..2 xyz[idx] - centre (the only float operation) when use_xyz,
 * then features[idx], moved as bits.  features NULL or C = 0: the three xyz channels only (use_xyz required).
 * use_xyz = 0: the plain grouping_operation; xyz and centres are not read and may be NULL.
 * An index outside [0, N) sets DFU3D_PN2_ST_BAD_INDEX and reads point 0. */
int dfu3d_pn2_group(const float *xyz, const float *centres, const float *features, const int32_t *idx, int32_t B,
                    int32_t N, int32_t M, int32_t nsample, int32_t C, int32_t use_xyz, float *out, uint32_t *status,
                    void *stream);

/* three_nn_kernel_fast with torch.sqrt folded in: unknown (B, n, 3), known (B, m, 3) -> dist float32 (B, n, 3) =
 * sqrt(squared distance), idx int32 (B, n, 3): the reference's cascade of strict < over ascending k, so among equal
 * distances the lower index ranks first.  m < 3 leaves the unfilled ranks at distance +inf, index 0. */
int dfu3d_pn2_three_nn(const float *unknown, const float *known, int32_t B, int32_t n, int32_t m, float *dist,
                       int32_t *idx, void *stream);

/* out[b, c, j] = w[b,j,0] * f[b,c,i0] + w[b,j,1] * f[b,c,i1] + w[b,j,2] * f[b,c,i2], products rounded, summed left
 * to right: features (B, C, m), idx int32 (B, n, 3), weight (B, n, 3), out (B, C, n).  An index outside [0, m) sets
 * DFU3D_PN2_ST_BAD_INDEX and reads column 0. */
int dfu3d_pn2_three_interpolate(const float *features, const int32_t *idx, const float *weight, int32_t B, int32_t C,
                                int32_t m, int32_t n, float *out, uint32_t *status, void *stream);

/* The inverse of a gather: idx int32 (B, E), values in [0, N) -> csr int32 (B, N + 1), list int32 (B, E): the entries
 * e with idx[b, e] = s are list[b, csr[b, s] .. csr[b, s + 1]), in ASCENDING entry number.  Integer atomics place the
 * entries, a sort of every source's run makes the order independent of them.  A value outside [0, N) sets
 * DFU3D_PN2_ST_BAD_INDEX and the entry is left out.  scratch: dfu3d_pn2_scratch_bytes(B, N, E) bytes. */
int dfu3d_pn2_invert(const int32_t *idx, int32_t B, int32_t N, int64_t E, int32_t *csr, int32_t *list, void *scratch,
                     uint32_t *status, void *stream);

/* The backward of grouping (k = 1, w = NULL: weight 1) and of interpolation (k = 3, w float32 (B, E)):
 *     grad_features[b, c, s] = sum over the entries e of s, ascending, of w[b, e] * grad_out[b, c, e / k]
 * starting from +0.0f, in float32, one addition per entry; grad_out (B, C, E / k), grad_features (B, C, N): EVERY
 * element is written, the caller does not clear it.  The same bits on every run.  csr, list: as dfu3d_pn2_invert left
 * them; a list element outside [0, E) is skipped. */
int dfu3d_pn2_gather_backward(const float *grad_out, const float *w, const int32_t *csr, const int32_t *list,
                              int32_t B, int32_t C, int32_t N, int64_t E, int32_t k, float *grad_features,
                              void *stream);

/* points float32 (rows, cols), column 0 the sample index: a row r whose column 0 is not r / per_sample sets
 * DFU3D_PN2_ST_BAD_BATCH.  rows a multiple of per_sample >= 1, cols >= 4, else DFU3D_EINVAL. */
int dfu3d_pn2_check_batch(const float *points, int64_t rows, int32_t cols, int32_t per_sample, uint32_t *status,
                          void *stream);

#ifdef __cplusplus
}
#endif

#endif
