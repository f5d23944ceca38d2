// bevscatter_stage.hip -- SURVEY.md §8 row f-11: the one layer between the pillar encoder and the 2-D backbone
// (include/dfu3d_bev.h).
//
// What it stands in for in the reference: pcdet/models/backbones_2d/map_to_bev/pointpillar_scatter.py -- a device read
// for the batch size, then per sample a boolean mask, a zero canvas, an index assignment of the transposed rows, and a
// stack of the canvases.  Here the canvas is written once, driven from the output:
//
//   k_bs_clear   cell_map <- -1.
//   k_bs_mark    one thread per pillar: coordinate check, integer atomicMax of the row index on the pillar's cell (the
//                highest row wins, as a sequential assignment leaves it); status bits, one atomicOr per wave.
//   k_bs_write   one workgroup per run of DFU3D_BEV_RUN consecutive x of one (b, z, y) line: the run's cell_map entries
//                (coalesced), the owners' rows into an LDS tile [x][channel] (a coalesced row read each; pitch 65 words,
//                so the transposed read is conflict-free as words and two-way as quads), then for every channel
//                the full line along x -- zeros for empty cells in the same stores, 16 bytes per lane where nx allows.
//                A run without any pillar never touches the LDS tile.  Channels in chunks of 64.
//   k_bs_gather  the backward, the mirror of k_bs_write: lines of grad_canvas are read only where a cell has an owner,
//                transposed through the same tile and written as full rows of grad_features; the blocks behind the
//                tiles zero the rows that own no cell (dropped rows, losing duplicates).
// Values move as 32-bit words: no float instruction touches them, so NaN payloads and the sign of zero survive.
#include "common.hpp"
#include "dfu3d_bev.h"

namespace {

constexpr int BT = 256;                             // threads per workgroup
constexpr int RUN = DFU3D_BEV_RUN;                  // cells of a run
constexpr int CH = 64;                              // channels of a chunk
constexpr int PITCH = CH + 1;                       // words per cell of the LDS tile
static_assert(RUN == 64 && BT == 4 * RUN, "a wave per quarter of the run");

__device__ __forceinline__ int pillar_count(const int *__restrict__ n_pillars, int p_cap) {
  if (!n_pillars) return p_cap;
  const int n = n_pillars[0];
  return n < 0 ? 0 : (n < p_cap ? n : p_cap);
}

// the cell of row p, or -1 when a coordinate lies outside the canvas
__device__ __forceinline__ int cell_of(const int *__restrict__ coords, int cols, int p, int B, int nz, int ny, int nx) {
  const int *q = coords + (size_t)p * cols;
  const int b = q[0], z = cols == 4 ? q[1] : 0, y = q[cols - 2], x = q[cols - 1];
  if ((unsigned)b >= (unsigned)B || (unsigned)z >= (unsigned)nz || (unsigned)y >= (unsigned)ny ||
      (unsigned)x >= (unsigned)nx)
    return -1;
  return ((b * nz + z) * ny + y) * nx + x;         // < DFU3D_BEV_MAX_CELLS
}

__global__ __launch_bounds__(BT) void k_bs_clear(int *__restrict__ cell_map, int n_cells) {
  for (int i = blockIdx.x * BT + threadIdx.x; i < n_cells; i += gridDim.x * BT) cell_map[i] = -1;
}

__global__ __launch_bounds__(BT) void k_bs_mark(const int *__restrict__ coords, int cols, int p_cap,
                                                const int *__restrict__ n_pillars, int B, int nz, int ny, int nx,
                                                int *__restrict__ cell_map, uint32_t *__restrict__ status) {
  const int n = pillar_count(n_pillars, p_cap);
  uint32_t st = 0u;
  for (int p = blockIdx.x * BT + threadIdx.x; p < n; p += gridDim.x * BT) {
    const int cell = cell_of(coords, cols, p, B, nz, ny, nx);
    if (cell < 0)
      st |= DFU3D_BEV_ST_BAD_COORD;
    else if (atomicMax(&cell_map[cell], p) >= 0)
      st |= DFU3D_BEV_ST_DUPLICATE;                  // whoever comes second sees the first, whichever of them wins
  }
  st = wave_or_u32_dpp(st);
  if (lane_id() == 0 && st) atomicOr(status, st);
}

// The run of this workgroup: its owners into s_win (-1: none, or an entry no row of this call can have left).
// Returns whether the run holds any pillar (uniform over the workgroup); contains a barrier.
__device__ __forceinline__ bool load_run(const int *__restrict__ cell_map, size_t first_cell, int len, int n, int *s_win) {
  const int t = threadIdx.x;
  int win = -1;
  if (t < RUN) {
    if (t < len) {
      win = cell_map[first_cell + t];
      if (win < 0 || win >= n) win = -1;
    }
    s_win[t] = win;
  }
  return __syncthreads_or(win >= 0) != 0;
}

__global__ __launch_bounds__(BT) void k_bs_write(const uint32_t *__restrict__ feat, int p_cap,
                                                 const int *__restrict__ n_pillars, int C, int lines, int nx,
                                                 int tiles_x, const int *__restrict__ cell_map,
                                                 uint32_t *__restrict__ canvas, int vec) {
  __shared__ int s_win[RUN];
  __shared__ uint32_t s_tile[RUN * PITCH];
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  const int line = blockIdx.x / tiles_x, x0 = (blockIdx.x - line * tiles_x) * RUN;   // line = (b * nz + z) * ny + y
  const int b = line / lines, zy = line - b * lines;
  const int len = nx - x0 < RUN ? nx - x0 : RUN;
  const bool any = load_run(cell_map, (size_t)line * nx + x0, len, pillar_count(n_pillars, p_cap), s_win);
  const size_t plane = (size_t)lines * nx;           // words of one (b, channel)
  uint32_t *base = canvas + ((size_t)b * C * lines + zy) * nx + x0;
  for (int c0 = 0; c0 < C; c0 += CH) {
    const int cc = C - c0 < CH ? C - c0 : CH;
    if (any) {
      if (c0) __syncthreads();                       // the chunk before has been read
      for (int i = w; i < len; i += BT / 64) {
        const int win = s_win[i];
        uint32_t v = 0u;
        if (win >= 0 && lane < cc) v = feat[(size_t)win * C + c0 + lane];
        s_tile[i * PITCH + lane] = v;
      }
      __syncthreads();
    }
    if (vec) {                                       // nx % 4 == 0 and a 16-byte aligned canvas: len % 4 == 0 as well
      const int xq = (t & 15) * 4;
      if (xq < len) {
        for (int ch = t >> 4; ch < cc; ch += BT / 16) {
          uint4 v = make_uint4(0u, 0u, 0u, 0u);
          if (any) {
            const uint32_t *s = s_tile + xq * PITCH + ch;
            v = make_uint4(s[0], s[PITCH], s[2 * PITCH], s[3 * PITCH]);
          }
          *reinterpret_cast<uint4 *>(base + (size_t)(c0 + ch) * plane + xq) = v;
        }
      }
    } else if (lane < len) {
      for (int ch = w; ch < cc; ch += BT / 64) base[(size_t)(c0 + ch) * plane + lane] = any ? s_tile[lane * PITCH + ch] : 0u;
    }
  }
}

__global__ __launch_bounds__(BT) void k_bs_gather(const uint32_t *__restrict__ gcanvas, const int *__restrict__ coords,
                                                  int cols, int p_cap, const int *__restrict__ n_pillars, int C, int B,
                                                  int nz, int ny, int nx, int tiles_x, int n_tile_blocks,
                                                  const int *__restrict__ cell_map, uint32_t *__restrict__ gfeat) {
  __shared__ int s_win[RUN];
  __shared__ uint32_t s_tile[RUN * PITCH];
  const int n = pillar_count(n_pillars, p_cap);
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  if ((int)blockIdx.x >= n_tile_blocks) {            // the rows that own no cell
    const int p = ((int)blockIdx.x - n_tile_blocks) * BT + t;
    if (p < n) {
      const int cell = cell_of(coords, cols, p, B, nz, ny, nx);
      if (cell < 0 || cell_map[cell] != p) {
        uint32_t *g = gfeat + (size_t)p * C;
        for (int c = 0; c < C; c++) g[c] = 0u;
      }
    }
    return;
  }
  const int lines = nz * ny;
  const int line = blockIdx.x / tiles_x, x0 = (blockIdx.x - line * tiles_x) * RUN;
  const int b = line / lines, zy = line - b * lines;
  const int len = nx - x0 < RUN ? nx - x0 : RUN;
  if (!load_run(cell_map, (size_t)line * nx + x0, len, n, s_win)) return;
  const size_t plane = (size_t)lines * nx;
  const uint32_t *base = gcanvas + ((size_t)b * C * lines + zy) * nx + x0;
  const bool mine = lane < len && s_win[lane] >= 0;
  for (int c0 = 0; c0 < C; c0 += CH) {
    const int cc = C - c0 < CH ? C - c0 : CH;
    if (c0) __syncthreads();
    if (mine)
      for (int ch = w; ch < cc; ch += BT / 64) s_tile[lane * PITCH + ch] = base[(size_t)(c0 + ch) * plane + lane];
    __syncthreads();
    for (int i = w; i < len; i += BT / 64) {
      const int win = s_win[i];
      if (win >= 0 && lane < cc) gfeat[(size_t)win * C + c0 + lane] = s_tile[i * PITCH + lane];
    }
  }
}

// DFU3D_OK, or the code the arguments earn; cells <- batch_size * nz * ny * nx
int check_shape(int32_t coord_cols, int32_t p_cap, int32_t C, int32_t batch_size, int32_t nz, int32_t ny, int32_t nx,
                int64_t &cells) {
  if (coord_cols != 3 && coord_cols != 4) return DFU3D_EINVAL;
  if (coord_cols == 3 && nz != 1) return DFU3D_EINVAL;
  if (p_cap < 0 || batch_size < 1 || nz < 1 || ny < 1 || nx < 1) return DFU3D_EINVAL;
  if (C < 1 || C > DFU3D_BEV_MAX_CHANNELS) return DFU3D_EINVAL;
  if (p_cap > DFU3D_BEV_MAX_ROWS) return DFU3D_ERANGE;
  cells = 1;
  const int32_t dims[4] = {batch_size, nz, ny, nx};
  for (int k = 0; k < 4; k++) {                      // every partial product stays below 2^55
    cells *= dims[k];
    if (cells > DFU3D_BEV_MAX_CELLS) return DFU3D_ERANGE;
  }
  return DFU3D_OK;
}

unsigned blocks_for(int64_t n, unsigned cap) {
  const int64_t g = (n + BT - 1) / BT;
  return (unsigned)(g < 1 ? 1 : (g > (int64_t)cap ? (int64_t)cap : g));
}

}  // namespace

extern "C" int32_t dfu3d_bev_version(void) { return DFU3D_BEV_VERSION; }

extern "C" int64_t dfu3d_bev_scratch_bytes(int64_t n_cells) {
  if (n_cells < 0 || n_cells > DFU3D_BEV_MAX_CELLS) return -1;
  return n_cells * (int64_t)sizeof(int32_t);
}

extern "C" int dfu3d_pillar_scatter(const float *features, const int32_t *coords, int32_t coord_cols, int32_t p_cap,
                                    const int32_t *n_pillars, int32_t C, int32_t batch_size, int32_t nz, int32_t ny,
                                    int32_t nx, float *canvas, int32_t *cell_map, uint32_t *status, void *stream) {
  DFU3D_CLEAR_STALE_ERROR();
  int64_t cells = 0;
  const int rc = check_shape(coord_cols, p_cap, C, batch_size, nz, ny, nx, cells);
  if (!canvas || !cell_map || !status || (p_cap > 0 && (!features || !coords))) return DFU3D_EINVAL;
  if (rc != DFU3D_OK) return rc;
  if ((const void *)features == (const void *)canvas) return DFU3D_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  const int tiles_x = (nx + RUN - 1) / RUN;
  const int64_t n_tiles = (int64_t)batch_size * nz * ny * tiles_x;   // <= cells
  const int vec = (nx % 4 == 0 && ((uintptr_t)canvas & 15u) == 0) ? 1 : 0;
  hipLaunchKernelGGL(k_bs_clear, dim3(blocks_for(cells / 4, 4096)), dim3(BT), 0, st, cell_map, (int)cells);
  DFU3D_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_bs_mark, dim3(blocks_for(p_cap, 1u << 20)), dim3(BT), 0, st, coords, coord_cols, p_cap, n_pillars,
                     batch_size, nz, ny, nx, cell_map, status);
  DFU3D_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_bs_write, dim3((unsigned)n_tiles), dim3(BT), 0, st, (const uint32_t *)features, p_cap, n_pillars,
                     C, nz * ny, nx, tiles_x, (const int *)cell_map, (uint32_t *)canvas, vec);
  DFU3D_LAUNCH_CHECK();
  return DFU3D_OK;
}

extern "C" int dfu3d_pillar_scatter_backward(const float *grad_canvas, const int32_t *coords, int32_t coord_cols,
                                             int32_t p_cap, const int32_t *n_pillars, int32_t C, int32_t batch_size,
                                             int32_t nz, int32_t ny, int32_t nx, const int32_t *cell_map,
                                             float *grad_features, void *stream) {
  DFU3D_CLEAR_STALE_ERROR();
  int64_t cells = 0;
  const int rc = check_shape(coord_cols, p_cap, C, batch_size, nz, ny, nx, cells);
  if (!grad_canvas || !cell_map || (p_cap > 0 && (!coords || !grad_features))) return DFU3D_EINVAL;
  if (rc != DFU3D_OK) return rc;
  if ((const void *)grad_canvas == (const void *)grad_features) return DFU3D_EINVAL;
  const int tiles_x = (nx + RUN - 1) / RUN;
  const int64_t n_tiles = (int64_t)batch_size * nz * ny * tiles_x;
  const int64_t row_blocks = ((int64_t)p_cap + BT - 1) / BT;
  hipLaunchKernelGGL(k_bs_gather, dim3((unsigned)(n_tiles + (row_blocks < 1 ? 1 : row_blocks))), dim3(BT), 0,
                     (hipStream_t)stream, (const uint32_t *)grad_canvas, coords, coord_cols, p_cap, n_pillars, C, batch_size,
                     nz, ny, nx, tiles_x, (int)n_tiles, cell_map, (uint32_t *)grad_features);
  DFU3D_LAUNCH_CHECK();
  return DFU3D_OK;
}
