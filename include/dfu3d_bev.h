/* dfu3d_bev.h -- C ABI of the pillar-to-BEV scatter of libdfu3d_hip.so (csrc/bevscatter_stage.hip): OpenPCDet's
 * PointPillarScatter / PointPillarScatter3d -- pillar_features (P, C) and voxel_coords (P, 4) into the dense canvas
 * (B, C, nz, ny, nx) -- for a whole batch in three launches, and its backward in one.
 *
 * The entry points live in the same library as include/dfu3d.h's and follow its rules: device pointers, results in
 * device memory, the library never allocates and never synchronises, every call returns DFU3D_OK / DFU3D_EINVAL /
 * DFU3D_ELAUNCH / DFU3D_ERANGE (dfu3d.h) and validates its arguments on the host before any launch.  The header keeps
 * to the C subset dfu3d_amd/_header.py reads.
 */
#ifndef DFU3D_BEV_H
#define DFU3D_BEV_H

#include <stddef.h>
#include <stdint.h>

#define DFU3D_BEV_VERSION 1

/* cells of the canvas, B * nz * ny * nx (the pillar encoder's limit): beyond it DFU3D_ERANGE */
#define DFU3D_BEV_MAX_CELLS 16777216
/* rows of the pillar list (p_cap): beyond it DFU3D_ERANGE */
#define DFU3D_BEV_MAX_ROWS 1073741824
/* channels of a pillar: 1 .. DFU3D_BEV_MAX_CHANNELS, else DFU3D_EINVAL */
#define DFU3D_BEV_MAX_CHANNELS 256
/* consecutive x of one (b, z, y) line a workgroup of the canvas kernels owns */
#define DFU3D_BEV_RUN 64

/* bits of the status word */
#define DFU3D_BEV_ST_BAD_COORD 1
#define DFU3D_BEV_ST_DUPLICATE 2

#ifdef __cplusplus
extern "C" {
#endif

int32_t dfu3d_bev_version(void);

/* bytes of the cell map of a canvas of n_cells cells (one int32 each); -1 for n_cells < 0 or beyond DFU3D_BEV_MAX_CELLS */
int64_t dfu3d_bev_scratch_bytes(int64_t n_cells);

/* features float32 (p_cap, C); coords int32 (p_cap, coord_cols): [b, z, y, x] for coord_cols = 4, [b, y, x] for
 * coord_cols = 3 (nz = 1 only).  n_pillars: NULL (all p_cap rows are pillars) or one int32 in device memory: rows at or
 * beyond min(*n_pillars, p_cap) are never read.
 * canvas float32 (batch_size, C, nz, ny, nx), contiguous: EVERY element is written exactly once per call -- the bits of
 * the pillar's value or +0.0f; the caller does not clear it.  No float arithmetic, no float atomics: the result does
 * not depend on the order of the rows.
 * cell_map int32 (batch_size * nz * ny * nx), an output: the row that owns a cell, or -1.  A row whose b, z, y or x lies
 * outside the canvas is dropped and sets DFU3D_BEV_ST_BAD_COORD.  Two or more rows on one cell set
 * DFU3D_BEV_ST_DUPLICATE and the highest row index owns the cell (what a sequential assignment leaves).
 * status: ORed into, never cleared.  features, coords may be NULL when p_cap = 0. */
int dfu3d_pillar_scatter(const float *features, const int32_t *coords, int32_t coord_cols, int32_t p_cap,
                         const int32_t *n_pillars, int32_t C, int32_t batch_size, int32_t nz, int32_t ny, int32_t nx,
                         float *canvas, int32_t *cell_map, uint32_t *status, void *stream);

/* grad_canvas float32 in the canvas's layout; coords, n_pillars, cell_map as given to / left by dfu3d_pillar_scatter.
 * grad_features float32 (p_cap, C): row p = the gradient at p's cell when p owns it, +0.0f otherwise (dropped rows,
 * losing duplicates); every row below the pillar count is written, no row at or beyond it is touched. */
int dfu3d_pillar_scatter_backward(const float *grad_canvas, const int32_t *coords, int32_t coord_cols, int32_t p_cap,
                                  const int32_t *n_pillars, int32_t C, int32_t batch_size, int32_t nz, int32_t ny,
                                  int32_t nx, const int32_t *cell_map, float *grad_features, void *stream);

#ifdef __cplusplus
}
#endif

#endif
