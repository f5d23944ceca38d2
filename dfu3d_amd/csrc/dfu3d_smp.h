/* dfu3d_smp.h -- C ABI of the point-sampling stage in libdfu3d_hip.so (csrc/pointsample_stage.hip): what
 * DataProcessor.sample_points computes scene by scene on the host -- a cloud of exactly K points out of a scene's n, the
 * far points kept, in a random order -- for a whole batch in DFU3D_SMP_LAUNCHES kernel launches and without a read from
 * the device.
 *
 * The entry points live in the library of the headers under include/ and follow its rules: device pointers, results in
 * device memory, the library never allocates, never synchronises and never reads from the device; every call returns
 * DFU3D_OK / DFU3D_EINVAL / DFU3D_ELAUNCH / DFU3D_ERANGE and validates its arguments on the host before any launch.  The
 * header keeps to the C subset dfu3d_amd/_header.py reads.  (It sits next to the sources and not under include/ because
 * the set of files there is pinned by an existing test: INTEGRATION.md.)
 *
 * The randomness is the caller's: three blocks of 32-bit words, read as uint32.  The result is a pure function of the
 * inputs.
 *
 * THE RULE.  Scene b owns the n = point_cnt[b] rows that start at the exclusive prefix sum of point_cnt; rows are
 * numbered 0 .. n-1 inside their scene.  The depth of a row is
 *     d = fl32(sqrt(fl32(fl32(x*x + y*y) + z*z)))
 * every product and every sum rounded to float32 on its own, no fused multiply-add, the square root correctly rounded
 * (NumPy's np.linalg.norm(points[:, 0:3], axis=1) on float32).  A row is NEAR iff d < 40.0f; a NaN depth is not near.
 * F = the number of rows that are not near.  "Smallest" always means by (sel[row], row) ascending, sel indexed by the
 * row's place in `points`: the row index breaks ties.
 *
 * The chosen list L has K scene-local rows:
 *     n > K and F < K    all far rows and the K - F smallest near rows, in ascending row order
 *     n > K and F >= K   the K smallest of all rows, in ascending row order (the reference's quirk: it draws from every
 *                        row, not from the far ones)
 *     n == K             0 .. n-1
 *     n < K <= 2n        0 .. n-1, then the K - n smallest rows in ascending row order (no row a third time)
 *     K > 2n             0 .. n-1, then for j = 0 .. K-n-1 the row (uint64(rep[b, j]) * n) >> 32
 *     n == 0             no row: the scene's K output rows are b followed by zeros, and DFU3D_SMP_EMPTY_SCENE is OR-ed into
 *                        status
 * The depth is looked at in the first two cases only.
 *
 * THE SHUFFLE.  The slots j = 0 .. K-1 are sorted ascending by (ord[b, j], j): j_0, j_1, ...  Then
 *     out[b * K + t] = (b, the first out_cols feature columns of the scene's row L[j_t]).
 */
#ifndef DFU3D_SMP_H
#define DFU3D_SMP_H

#include <stddef.h>
#include <stdint.h>

#define DFU3D_SMP_VERSION 1

/* kernel launches of one call of dfu3d_sample_points, for any B: the shuffle orders, the lists, the gather */
#define DFU3D_SMP_LAUNCHES 3
/* K at most (one workgroup sorts a scene's K shuffle words).  Beyond it DFU3D_ERANGE */
#define DFU3D_SMP_MAX_OUT 16384
/* scenes of a batch at most.  Beyond it DFU3D_ERANGE */
#define DFU3D_SMP_MAX_BATCH 65535
/* elements of the input block, R * (1 + C), and of the output block, B * K * (1 + out_cols), at most.  Beyond it
 * DFU3D_ERANGE.  A scene has no cap of its own below it */
#define DFU3D_SMP_MAX_ELEMS 2147483647

/* bits OR-ed into *status (never cleared by the stage) */
/* a scene without rows: its K output rows are (b, 0, ..., 0) */
#define DFU3D_SMP_EMPTY_SCENE 1
/* a negative point_cnt[b] (taken as 0), or counts that sum beyond R (the scene is cut at R: nothing outside `points` is read) */
#define DFU3D_SMP_BAD_COUNT 2

/* The shape of the kernels, stated here because their LDS follows from it (tests/test_kernel_resources_sample_points.py):
 * threads of the workgroup that sorts a scene's shuffle words and of the one that selects its list; threads of a gather
 * workgroup */
#define DFU3D_SMP_SCENE_THREADS 1024
#define DFU3D_SMP_GATHER_THREADS 256

#ifdef __cplusplus
extern "C" {
#endif

int32_t dfu3d_smp_version(void);

/* Bytes of scratch dfu3d_sample_points needs for these sizes: a far flag of one byte per input row, per scene two
 * (key, index) buffers of K entries for the sort to alternate between, the shuffle order and the list (K int32 each),
 * and the scene's first row and row count; rounded up to 16.  0 for B = 0 (nothing is launched then) and for arguments
 * out of range (negative sizes, K < 1, K > DFU3D_SMP_MAX_OUT, B > DFU3D_SMP_MAX_BATCH). */
size_t dfu3d_smp_scratch_bytes(int32_t B, int32_t R, int32_t K);

/* points float32 (R, 1 + C), the output form of dfu3d_world_aug_collate: column 0 the scene index (not read: the scenes
 * are contiguous and in order, point_cnt says where they are), then C feature columns, the first three x, y, z.
 * point_cnt int32 (B).  Rows at or beyond sum(point_cnt) are never read.  sel int32 (R), ord and rep int32 (B, K): the
 * random words.  None of them is written.  scratch: 16-byte aligned, dfu3d_smp_scratch_bytes(B, R, K) bytes at least,
 * its content on entry does not matter.
 *
 *     out     float32 (B * K, 1 + out_cols)   THE RULE and THE SHUFFLE above
 *     status  int32 (1)                       DFU3D_SMP_* bits, OR-ed
 * EVERY element of out is written; the caller clears nothing.  Floats are copies: the same bits.
 *
 * A null pointer (points and sel may be null when R == 0), B < 0, R < 0, K < 1, C < 3, out_cols outside 3 .. C, a
 * scratch that is not 16-byte aligned or too short: DFU3D_EINVAL.  K > DFU3D_SMP_MAX_OUT, B > DFU3D_SMP_MAX_BATCH,
 * R * (1 + C) or B * K * (1 + out_cols) > DFU3D_SMP_MAX_ELEMS: DFU3D_ERANGE.  B == 0: DFU3D_OK and nothing is launched or
 * written. */
int dfu3d_sample_points(const float *points, const int32_t *point_cnt, int32_t B, int32_t R, int32_t C, int32_t K,
                        int32_t out_cols, const int32_t *sel, const int32_t *ord, const int32_t *rep, void *scratch,
                        size_t scratch_bytes, float *out, int32_t *status, void *stream);

#ifdef __cplusplus
}
#endif

#endif
