/* dfu3d_spc.h -- C ABI of the sparse 3-D convolution stage in libdfu3d_hip.so (csrc/sparseconv_stage.hip): what
 * SubMConv3d and SparseConv3d of the voxel backbones compute -- the index plan (site sets, neighbour tables), the
 * forward sum, and both gradients -- on 32-bit float features.
 *
 * The entry points live in the library of the headers under include/ and follow its rules: device pointers, results in
 * device memory, the library never allocates, never synchronises and never reads from the device; every call returns
 * DFU3D_OK / DFU3D_EINVAL / DFU3D_ELAUNCH / DFU3D_ERANGE and validates its arguments on the host before any launch.  The
 * header keeps to the C subset dfu3d_amd/_header.py reads.  (It sits next to the sources and not under include/ because
 * the set of files there is pinned by an existing test: INTEGRATION.md.)
 *
 * The library these layers come from elsewhere is not part of the build: the rules below are the contract, restated
 * sequentially in tests/sparse_conv_ref.py and pinned there against a dense float64 convolution.  Every result is a pure
 * function of the inputs: no float atomics, every output element written exactly once.
 *
 * SITES.  A sparse tensor is `features` float32 (N, C) and `indices` int32 (N, 4) = [b, z, y, x] over the spatial shape
 * (D, H, W) and B scenes; `count` (a device int) says how many leading rows there are, min(max(count, 0), N) is used and
 * rows at or beyond it are never read.  A row below the count whose b is outside [0, B) or whose cell is outside the
 * shape ORs DFU3D_SPC_ST_BAD_COORD into status; it is no site.  Of several rows in one cell the lowest is the site (it
 * OWNS the cell), the others are no sites, and DFU3D_SPC_ST_DUP_SITE is OR-ed into status.  A row that is no site is
 * nobody's neighbour, feeds nothing, and where it is an output row (submanifold) all its neighbours are absent: +0.0.
 *
 * THE GEOMETRY.  Per axis a = z, y, x with kernel k_a, stride s_a, padding p_a: out_a = floor((in_a + 2 p_a - k_a) / s_a)
 * + 1.  Output cell o reads input cell o * s - p + j for j in [0, k) on every axis; the flat offset index is
 * K = (jz * ky + jy) * kx + jx, KV = kz * ky * kx of them.
 *
 * THE OUTPUT SITES.  Submanifold (subm != 0: every stride 1, every p = k / 2, k odd): the output rows are the input rows,
 * in the same order, with the same indices.  Strided (subm == 0): the output sites are the cells with at least one input
 * site in their window, listed in first-seen order over the candidates (input row i ascending, then K ascending), a
 * candidate being a pair whose output cell o = (in + p - j) / s is whole and inside the output shape on every axis.
 *
 * THE CAPACITY BOUND.  For an input site and one axis the numbers in + p - j, j in [0, k), are k consecutive integers,
 * of which at most ceil(k / s) are multiples of s: an input site reaches at most prod_a ceil(k_a / s_a) output cells.
 * And no more than B * out_z * out_y * out_x cells exist.  So with N input rows
 *     N_out <= min(N * prod_a ceil(k_a / s_a), B * out_z * out_y * out_x)
 * and dfu3d_spc_downsample asks for at least that many output rows (`N_out_cap`), which makes every rank it writes fit.
 *
 * THE TABLES.  nbr[o][K] int32 is the input site (row) at the cell output site o reads through offset K, or -1 (outside
 * the shape, no site there, o itself no site or at or beyond its count).  inv[i][K] int32 is the output site that input
 * site i feeds through offset K, or -1; there is at most one, since o = (in + p - j) / s is one cell and a cell has one
 * owner.  nbr[o][K] == i exactly when inv[i][K] == o.
 *
 * THE SUM (forward).  y[o][co] = sum over K and ci of x[nbr[o][K]][ci] * w[co][K][ci]:
 *     acc = +0.0f;  for K ascending, for ci ascending:  acc = fmaf(x[nbr[o][K]][ci], w[co][K][ci], acc)
 * one rounding per step, an absent neighbour contributing +0.0 terms (x taken as +0.0).  The kernel may leave out the
 * offsets that are absent for a whole tile and pads short channel counts with +0.0 * +0.0 terms; both change at most
 * the sign of a zero, so results are compared as float32 VALUES (-0.0 == +0.0).  The contract holds for finite features
 * and weights.  There is no bias in the op.
 *
 * THE FEATURE GRADIENT.  dx[i][ci] = sum over K and co of dy[inv[i][K]][co] * w[co][K][ci]: THE SUM with (K ascending,
 * co ascending), absent entries of inv as +0.0 terms.
 *
 * THE WEIGHT GRADIENT.  dw[co][K][ci] = sum over o of dy[o][co] * x[nbr[o][K]][ci].  The output rows are cut into
 * chunks of DFU3D_SPC_WGRAD_CHUNK consecutive rows (the last may be short).  A chunk's partial is acc = +0.0f and
 * acc = fmaf(dy[o][co], x[nbr[o][K]][ci], acc) for o ascending, absent neighbours as +0.0 terms.  The partials are added
 * in ascending chunk order in float64, from +0.0, and the sum is rounded once to float32.
 */
#ifndef DFU3D_SPC_H
#define DFU3D_SPC_H

#include <stddef.h>
#include <stdint.h>

#define DFU3D_SPC_VERSION 1

/* kernel launches of one call, for any sizes */
/* dfu3d_spc_index: the fill of the cell table, the insert */
#define DFU3D_SPC_LAUNCHES_INDEX 2
/* dfu3d_spc_downsample: the fills, the candidates' insert, the counts of a block of candidates, their prefix and the
 * output count, the ranks and the output indices */
#define DFU3D_SPC_LAUNCHES_DOWNSAMPLE 5
/* dfu3d_spc_tables: the fill of inv, both tables */
#define DFU3D_SPC_LAUNCHES_TABLES 2
#define DFU3D_SPC_LAUNCHES_FORWARD 1
#define DFU3D_SPC_LAUNCHES_DGRAD 1
/* dfu3d_spc_wgrad: the chunk partials, their float64 sum (with no output row there is no chunk: the sum alone) */
#define DFU3D_SPC_LAUNCHES_WGRAD 2

/* rows of a chunk of THE WEIGHT GRADIENT: part of the contract, not of the device or the launch */
#define DFU3D_SPC_WGRAD_CHUNK 1024
/* channels at most, on either side.  Beyond it DFU3D_ERANGE */
#define DFU3D_SPC_MAX_CHANNELS 256
/* offsets of a kernel at most (3 x 3 x 3) */
#define DFU3D_SPC_MAX_KV 27
/* B * D * H * W stays below 2^DFU3D_SPC_KEY_BITS (the cell keys are 64-bit words).  Beyond it DFU3D_ERANGE */
#define DFU3D_SPC_KEY_BITS 62
/* rows of a tensor at most: the candidates (row, K) of a downsample and the entries of a cell table fit an int.  Beyond
 * it DFU3D_ERANGE */
#define DFU3D_SPC_MAX_ROWS 67108864
/* scenes at most.  Beyond it DFU3D_ERANGE */
#define DFU3D_SPC_MAX_BATCH 65535
/* a cell table is an open-addressing hash over cell keys with the smallest power of two of entries that is at least
 * DFU3D_SPC_TABLE_PER_ROW * rows (and at least 16): its load never exceeds 1 / DFU3D_SPC_TABLE_PER_ROW */
#define DFU3D_SPC_TABLE_PER_ROW 2

/* bits OR-ed into *status (never cleared by the stage) */
#define DFU3D_SPC_ST_BAD_COORD 1
#define DFU3D_SPC_ST_DUP_SITE 2

/* The shape of the kernels, stated here because their LDS follows from it (tests/test_kernel_resources_sparse_conv.py):
 * threads of a workgroup of the index kernels (a block of that many rows or candidates), of the gather-product kernel
 * and of the weight-gradient kernel; the tile of the gather-product kernel is 32 * 4 / WN rows by 32 * WN channels for
 * WN = 1 (at most 32 output channels) or 2, and DFU3D_SPC_TILE_K input channels are staged at a time */
#define DFU3D_SPC_ROW_THREADS 1024
#define DFU3D_SPC_GEMM_THREADS 256
#define DFU3D_SPC_WGRAD_THREADS 64
#define DFU3D_SPC_TILE_K 32

#ifdef __cplusplus
extern "C" {
#endif

int32_t dfu3d_spc_version(void);

/* Bytes of the cell table of a tensor of N_cap rows (per entry a 64-bit key and the row that owns the cell).  0 for
 * N_cap out of range. */
size_t dfu3d_spc_table_bytes(int32_t N_cap);

/* Bytes of scratch dfu3d_spc_downsample needs: per candidate (N_in * KV) its entry of the output table, per entry of
 * the output table (of N_out_cap rows) the first candidate, per block of DFU3D_SPC_ROW_THREADS candidates a prefix.  It
 * grows with the rows and KV only: no shape and no launch size enters.  0 for arguments out of range. */
size_t dfu3d_spc_scratch_bytes(int32_t N_in, int32_t N_out_cap, int32_t KV);

/* Bytes of scratch dfu3d_spc_wgrad needs: one partial of the weight's size per chunk.  0 for arguments out of range. */
size_t dfu3d_spc_wgrad_scratch_bytes(int32_t N_out, int32_t KV, int32_t Cin, int32_t Cout);

/* The cell table of a tensor's sites (SITES).  indices int32 (N, 4), count int32 (1), shape 3 int32 (D, H, W) read on
 * the HOST during the call; table: 16-byte aligned, dfu3d_spc_table_bytes(N) bytes, every byte written; status int32
 * (1).  N == 0: the table is filled (empty), indices may be null.
 * A null pointer otherwise, N < 0, B < 1, a shape_j < 1, a table that is not 16-byte aligned or too short:
 * DFU3D_EINVAL.  N > DFU3D_SPC_MAX_ROWS, B > DFU3D_SPC_MAX_BATCH, B * D * H * W >= 2^DFU3D_SPC_KEY_BITS: DFU3D_ERANGE. */
int dfu3d_spc_index(const int32_t *indices, const int32_t *count, int32_t N, int32_t B, const int32_t *shape, void *table,
                    size_t table_bytes, int32_t *status, void *stream);

/* THE OUTPUT SITES of a strided layer.  in_table: what dfu3d_spc_index (or an earlier call of this function) made for
 * the input tensor of N_in rows.  ksize, stride, padding: 3 int32 each (z, y, x), read on the HOST; every k in {1, 3},
 * every s in {1, 2}, 0 <= p < k; in_shape as above, the output shape follows from THE GEOMETRY and every out_a >= 1.
 *     out_indices int32 (N_out_cap, 4)   the output sites; rows at or beyond out_count are -1
 *     out_count   int32 (1)              their number
 *     out_table   dfu3d_spc_table_bytes(N_out_cap) bytes: the cell table of the output tensor
 * EVERY element of each is written.  N_out_cap at least THE CAPACITY BOUND for N_in.  scratch: 16-byte aligned,
 * dfu3d_spc_scratch_bytes(N_in, N_out_cap, KV) bytes at least, its content on entry does not matter.
 * Null pointers (in_indices may be null when N_in == 0), sizes below their minimum, a k, s or p outside the above, an
 * out_a < 1, N_out_cap < 1 or below the bound, misaligned or short tables or scratch: DFU3D_EINVAL.  N_in or N_out_cap
 * > DFU3D_SPC_MAX_ROWS, N_in * KV > 2^31 - 1, B or the key bits as above: DFU3D_ERANGE. */
int dfu3d_spc_downsample(const int32_t *in_indices, const int32_t *in_count, int32_t N_in, const void *in_table, int32_t B,
                         const int32_t *in_shape, const int32_t *ksize, const int32_t *stride, const int32_t *padding,
                         int32_t N_out_cap, void *scratch, size_t scratch_bytes, int32_t *out_indices,
                         int32_t *out_count, void *out_table, size_t out_table_bytes, void *stream);

/* THE TABLES of one layer.  The input tensor (N_in rows, in_table made for in_table_rows rows) and the
 * output tensor (out_indices, out_count, N_out rows, out_table made for out_table_rows rows); for a submanifold layer
 * pass the input tensor for both.  in_shape, ksize, stride, padding as above (the layer need not be one
 * dfu3d_spc_downsample accepts: stride 1 is a submanifold layer's).
 *     nbr int32 (N_out, KV)    inv int32 (N_in, KV)
 * EVERY element of both is written.  nbr may be null when N_out == 0, inv when N_in == 0.
 * Null pointers otherwise, negative sizes, table rows below the tensor's rows, geometry outside the above: DFU3D_EINVAL.
 * Sizes beyond the limits above: DFU3D_ERANGE. */
int dfu3d_spc_tables(int32_t N_in, const void *in_table, int32_t in_table_rows, const int32_t *out_indices,
                     const int32_t *out_count, int32_t N_out, const void *out_table, int32_t out_table_rows, int32_t B,
                     const int32_t *in_shape, const int32_t *ksize, const int32_t *stride, const int32_t *padding,
                     int32_t *nbr, int32_t *inv, void *stream);

/* THE SUM.  x float32 (N_in, Cin), nbr int32 (N_out, KV) with entries in [-1, N_in) (anything else is taken as -1),
 * w float32 (Cout, KV, Cin), y float32 (N_out, Cout): every element written.  N_out == 0: DFU3D_OK, nothing launched.
 * Null pointers (x may be null when N_in == 0), negative sizes, KV outside 1 .. DFU3D_SPC_MAX_KV, Cin or Cout < 1:
 * DFU3D_EINVAL.  Cin or Cout > DFU3D_SPC_MAX_CHANNELS, rows > DFU3D_SPC_MAX_ROWS: DFU3D_ERANGE. */
int dfu3d_spc_forward(const float *x, int32_t N_in, const int32_t *nbr, int32_t N_out, int32_t KV, const float *w,
                      int32_t Cin, int32_t Cout, float *y, void *stream);

/* THE FEATURE GRADIENT.  dy float32 (N_out, Cout), inv int32 (N_in, KV), w as above, dx float32 (N_in, Cin): every
 * element written.  N_in == 0: DFU3D_OK, nothing launched.  Errors as dfu3d_spc_forward's (dy may be null when
 * N_out == 0). */
int dfu3d_spc_dgrad(const float *dy, int32_t N_out, const int32_t *inv, int32_t N_in, int32_t KV, const float *w,
                    int32_t Cin, int32_t Cout, float *dx, void *stream);

/* THE WEIGHT GRADIENT.  x, dy, nbr as above; scratch: 16-byte aligned, dfu3d_spc_wgrad_scratch_bytes(N_out, KV, Cin,
 * Cout) bytes at least (may be null when that is 0); dw float32 (Cout, KV, Cin): every element written (+0.0 for
 * N_out == 0).  Errors as dfu3d_spc_forward's, and a misaligned or short scratch: DFU3D_EINVAL. */
int dfu3d_spc_wgrad(const float *x, int32_t N_in, const float *dy, const int32_t *nbr, int32_t N_out, int32_t KV,
                    int32_t Cin, int32_t Cout, void *scratch, size_t scratch_bytes, float *dw, void *stream);

#ifdef __cplusplus
}
#endif

#endif
