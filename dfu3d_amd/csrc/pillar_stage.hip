// pillar_stage.hip -- dynamic pillar feature encoder (include/dfu3d_vfe.h): pillar grouping without a sort, the point
// feature matrix, per-pillar maximum with its argument, and the backward of the maximum.
//
// Grouping.  The reference sorts the cell keys (torch.unique).  Here every kept point sets the bit of its cell in an
// occupancy bitmap; a prefix over the popcounts of the bitmap's words gives every occupied cell its rank in ascending
// key order, which is the pillar number torch.unique gives.  Kept points are compacted in input order (block counts
// + prefix).  A point takes a slot of its pillar with an integer atomic, so the CSR segment of a pillar first holds
// its rows in arrival order; k_pv_sort then ranks every row inside its segment, so the CSR the caller sees is in
// ascending row order whatever the arrival order was.  Every float sum over a pillar walks that list: bit-reproducible.
//
// All kernels read n_kept / P from `sizes` in device memory and are launched over the caller's capacities.
#include <math.h>

#include "common.hpp"
#include "dfu3d_vfe.h"

namespace {

constexpr int PT = 256;            // threads of the per-point kernels
constexpr int ST = 1024, SI = 8;   // the single-block scans: threads, consecutive items per thread
constexpr int PW = 8;              // pillars per wave of k_pv_mean
constexpr int MW = 4;              // waves (= pillars) per workgroup of the maximum kernels
constexpr int LONG_PILLAR = 128;   // above this many rows the workgroup's MW waves share a pillar

struct PvGeom {
  float rx, ry, vx, vy;
  int nx, ny, B, layout;
};

// ---- scratch: ONE definition of the carve-up; dfu3d_vfe_scratch_bytes is its last field ----------------------------
struct PvScratch {
  size_t key, slot, tmp, blk_cnt, blk_off, bitmap, wpre, bytes;
  int64_t words, blocks, p_cap;
};
inline size_t up16(size_t v) { return (v + 15u) & ~(size_t)15u; }
PvScratch pv_scratch(int64_t n, int64_t cells) {
  PvScratch s;
  s.words = (cells + 31) / 32;
  s.blocks = (n + PT - 1) / PT;
  s.p_cap = n < cells ? n : cells;
  size_t o = 0;
  // key, slot and tmp are dead once the grouping has run: dfu3d_pillar_features keeps the pillar means (3 floats for
  // each of at most n pillars) in their place
  s.key = o;     o = up16(o + (size_t)n * 4);            // int32 per point: cell key, -1 = dropped
  s.slot = o;    o = up16(o + (size_t)n * 4);            // int32 per kept row: arrival slot inside its pillar
  s.tmp = o;     o = up16(o + (size_t)n * 4);            // int32 per kept row: the CSR in arrival order
  s.blk_cnt = o; o = up16(o + (size_t)s.blocks * 4);     // kept points per block of PT points
  s.blk_off = o; o = up16(o + (size_t)s.blocks * 4);     // their exclusive prefix
  s.bitmap = o;  o = up16(o + (size_t)s.words * 4);      // occupancy, one bit per cell
  s.wpre = o;    o = up16(o + (size_t)s.words * 4);      // occupied cells before each word
  s.bytes = o + 16;
  return s;
}

// key of a point, -1 if it is dropped; bad: the point is reported in the status word
__device__ __forceinline__ int pv_key(const float *__restrict__ p, const PvGeom &g, bool &bad) {
  const float bf = p[0], x = p[1], y = p[2];
  const bool finite = (x - x == 0.0f) && (y - y == 0.0f);
  const bool batch_ok = bf > -1.0f && bf < (float)g.B;                  // (int32)bf in [0, B)
  bad = !finite || !batch_ok;
  if (bad) return -1;
  const float fx = floorf((x - g.rx) / g.vx), fy = floorf((y - g.ry) / g.vy);
  if (!(fx >= 0.0f && fx < (float)g.nx && fy >= 0.0f && fy < (float)g.ny)) return -1;
  return (int)bf * (g.nx * g.ny) + (int)fx * g.ny + (int)fy;
}

__global__ __launch_bounds__(PT) void k_pv_clear(uint32_t *__restrict__ bitmap, int64_t words, int *__restrict__ cnt,
                                                 int64_t p_cap, int *__restrict__ offsets, int *__restrict__ sizes,
                                                 uint32_t *__restrict__ status) {
  const int64_t tid = (int64_t)blockIdx.x * PT + threadIdx.x, nth = (int64_t)gridDim.x * PT;
  for (int64_t i = tid; i < words; i += nth) bitmap[i] = 0u;
  for (int64_t i = tid; i < p_cap; i += nth) cnt[i] = 0;
  if (tid == 0) {
    sizes[0] = 0;
    sizes[1] = 0;
    offsets[0] = 0;                                  // the whole CSR of an empty call
    *status = 0u;
  }
}

__global__ __launch_bounds__(PT) void k_pv_mark(const float *__restrict__ pts, int n, int cols, PvGeom g,
                                                int *__restrict__ key, uint32_t *__restrict__ bitmap,
                                                int *__restrict__ blk_cnt, uint32_t *__restrict__ status) {
  __shared__ int s_w[PT / 64];
  const int i = blockIdx.x * PT + threadIdx.x;
  int k = -1;
  bool bad = false;
  if (i < n) {
    k = pv_key(pts + (size_t)i * cols, g, bad);
    key[i] = k;
    if (k >= 0) atomicOr(&bitmap[k >> 5], 1u << (k & 31));
  }
  const unsigned long long any_bad = __ballot(bad);
  if (any_bad && lane_id() == 0) atomicOr(status, DFU3D_VFE_ST_BAD_POINT);
  int tot;
  block_rank<PT / 64>(k >= 0, s_w, tot);
  if (threadIdx.x == 0) blk_cnt[blockIdx.x] = tot;
}

// exclusive prefix of load(0..n) into out by the one workgroup of ST threads; returns the total (in every thread)
template <class F>
__device__ __forceinline__ int pv_scan(int n, F load, int *__restrict__ out, int *s_w) {
  return block_scan_range<ST, SI, int, int>(n, load, [&](int i, int ex) { out[i] = ex; }, s_w);
}

__global__ __launch_bounds__(ST) void k_pv_scan(const uint32_t *__restrict__ bitmap, int words, int *__restrict__ wpre,
                                                const int *__restrict__ blk_cnt, int blocks, int *__restrict__ blk_off,
                                                int *__restrict__ sizes) {
  __shared__ int s_w[ST / 64];
  const int P = pv_scan(words, [&](int i) { return __popc(bitmap[i]); }, wpre, s_w);
  const int kept = pv_scan(blocks, [&](int i) { return blk_cnt[i]; }, blk_off, s_w);
  if (threadIdx.x == 0) {
    sizes[0] = kept;
    sizes[1] = P;
  }
}

__global__ __launch_bounds__(PT) void k_pv_rank(const int *__restrict__ key, int n, PvGeom g,
                                                const uint32_t *__restrict__ bitmap, const int *__restrict__ wpre,
                                                const int *__restrict__ blk_off, int *__restrict__ kept_idx,
                                                int *__restrict__ unq_inv, int *__restrict__ cnt, int *__restrict__ slot,
                                                int *__restrict__ coords) {
  __shared__ int s_w[PT / 64];
  const int i = blockIdx.x * PT + threadIdx.x;
  const int k = i < n ? key[i] : -1;
  int tot;
  const int r = block_rank<PT / 64>(k >= 0, s_w, tot);
  if (k < 0) return;
  const int pos = blk_off[blockIdx.x] + r;
  const int w = k >> 5;
  const int pid = wpre[w] + __popc(bitmap[w] & ((1u << (k & 31)) - 1u));
  kept_idx[pos] = i;
  unq_inv[pos] = pid;
  slot[pos] = atomicAdd(&cnt[pid], 1);
  // every point of a pillar stores the same coordinates
  const int cell = k % (g.nx * g.ny), b = k / (g.nx * g.ny), cx = cell / g.ny, cy = cell % g.ny;
  if (g.layout == DFU3D_VFE_LAYOUT_PILLAR) {
    int *c = coords + (size_t)pid * 4;
    c[0] = b; c[1] = 0; c[2] = cy; c[3] = cx;
  } else {
    int *c = coords + (size_t)pid * 3;
    c[0] = b; c[1] = cy; c[2] = cx;
  }
}

__global__ __launch_bounds__(ST) void k_pv_offsets(const int *__restrict__ cnt, const int *__restrict__ sizes,
                                                   int *__restrict__ offsets) {
  __shared__ int s_w[ST / 64];
  const int P = sizes[1];
  const int tot = pv_scan(P, [&](int i) { return cnt[i]; }, offsets, s_w);
  if (threadIdx.x == 0) offsets[P] = tot;
}

__global__ __launch_bounds__(PT) void k_pv_place(const int *__restrict__ sizes, const int *__restrict__ unq_inv,
                                                 const int *__restrict__ slot, const int *__restrict__ offsets,
                                                 int *__restrict__ tmp) {
  const int pos = blockIdx.x * PT + threadIdx.x;
  if (pos < sizes[0]) tmp[offsets[unq_inv[pos]] + slot[pos]] = pos;
}

// rank of every row among the rows of its pillar: the rows of a pillar are distinct, so the ranks are a permutation
// of the segment.  A lane compares with its whole segment; the 64 rows of a wave inside one long pillar read the same
// addresses, so a long pillar is shared by rows / 64 waves.
__global__ __launch_bounds__(PT) void k_pv_sort(const int *__restrict__ sizes, const int *__restrict__ unq_inv,
                                                const int *__restrict__ offsets, const int *__restrict__ tmp,
                                                int *__restrict__ plist) {
  const int t = blockIdx.x * PT + threadIdx.x;
  if (t >= sizes[0]) return;
  const int e = tmp[t];
  const int p = unq_inv[e];
  const int s = offsets[p], n = offsets[p + 1] - s;
  int rank = 0;
  for (int j = 0; j < n; j++) rank += tmp[s + j] < e ? 1 : 0;
  plist[s + rank] = e;
}

// Mean of every pillar: one wave walks the CSR range of PW consecutive pillars, 64 rows per step gathered by the lanes
// (the next step's rows are requested before this step's are added), and adds them one after the other in list order.
__global__ __launch_bounds__(64) void k_pv_mean(const float *__restrict__ pts, int cols, const int *__restrict__ kept_idx,
                                                const int *__restrict__ offsets, const int *__restrict__ plist,
                                                const int *__restrict__ sizes, float *__restrict__ mean) {
  const int P = sizes[1];
  const int p0 = blockIdx.x * PW;
  if (p0 >= P) return;
  const int p1 = p0 + PW < P ? p0 + PW : P;
  const int lane = threadIdx.x;
  const int e_end = offsets[p1];
  int e = offsets[p0];
  int cur = p0, cur_begin = e, cur_end = offsets[p0 + 1];
  float sx = 0.0f, sy = 0.0f, sz = 0.0f;
  float nx = 0.0f, ny = 0.0f, nz = 0.0f;
  if (e + lane < e_end) {
    const float *q = pts + (size_t)kept_idx[plist[e + lane]] * cols;
    nx = q[1]; ny = q[2]; nz = q[3];
  }
  for (; e < e_end; e += 64) {
    const float x = nx, y = ny, z = nz;
    if (e + 64 + lane < e_end) {
      const float *q = pts + (size_t)kept_idx[plist[e + 64 + lane]] * cols;
      nx = q[1]; ny = q[2]; nz = q[3];
    }
    const int m = e_end - e < 64 ? e_end - e : 64;
    for (int j = 0; j < m; j++) {
      if (e + j >= cur_end) {                      // (every pillar holds a point: one step)
        if (lane == 0) {
          const float c = (float)(cur_end - cur_begin);
          mean[cur * 3 + 0] = sx / c; mean[cur * 3 + 1] = sy / c; mean[cur * 3 + 2] = sz / c;
        }
        cur++;
        cur_begin = cur_end;
        cur_end = offsets[cur + 1];
        sx = sy = sz = 0.0f;
      }
      sx += readlane_f(x, j);
      sy += readlane_f(y, j);
      sz += readlane_f(z, j);
    }
  }
  if (lane == 0) {
    const float c = (float)(cur_end - cur_begin);
    mean[cur * 3 + 0] = sx / c; mean[cur * 3 + 1] = sy / c; mean[cur * 3 + 2] = sz / c;
  }
}

struct PfCfg {
  float rx, ry, vx, vy, ox, oy, oz;
  int layout, abs_xyz, dist, cols, feat_cols;
};

__global__ __launch_bounds__(PT) void k_pv_feat(const float *__restrict__ pts, PfCfg g, const int *__restrict__ kept_idx,
                                                const int *__restrict__ unq_inv, const int *__restrict__ sizes,
                                                const float *__restrict__ mean, float *__restrict__ feat) {
  const int pos = blockIdx.x * PT + threadIdx.x;
  if (pos >= sizes[0]) return;
  const float *p = pts + (size_t)kept_idx[pos] * g.cols;
  float *o = feat + (size_t)pos * g.feat_cols;
  const float x = p[1], y = p[2], z = p[3];
  const float fx = floorf((x - g.rx) / g.vx), fy = floorf((y - g.ry) / g.vy);
  const float cx = x - (fx * g.vx + g.ox), cy = y - (fy * g.vy + g.oy), cz = z - g.oz;
  const int raw0 = g.abs_xyz ? 1 : 4;
  if (g.layout == DFU3D_VFE_LAYOUT_SIMPLE2D) {
    o[0] = cx; o[1] = cy; o[2] = cz;
    o += 3;
  }
  for (int c = raw0; c < g.cols; c++) *o++ = p[c];
  if (g.layout == DFU3D_VFE_LAYOUT_PILLAR) {
    const float *m = mean + (size_t)unq_inv[pos] * 3;
    o[0] = x - m[0]; o[1] = y - m[1]; o[2] = z - m[2];
    o[3] = cx; o[4] = cy; o[5] = cz;
    o += 6;
  }
  // torch.norm(p=2) over the three columns is a sequential FMA chain (measured bit-exact on golden G13, configuration B)
  if (g.dist) *o = sqrtf(__fmaf_rn(z, z, __fmaf_rn(y, y, x * x)));
}

// ---- per-pillar maximum --------------------------------------------------------------------------------------------
// A lane holds channels lane, lane + 64, ...: a wave-instruction reads one whole row (or 256 bytes of it).
template <int NC>
__device__ __forceinline__ void pm_scan(const float *__restrict__ x, int n_cap, int C, const int *__restrict__ plist,
                                        int b, int e, int lane, float best[NC], int arg[NC]) {
#pragma unroll
  for (int k = 0; k < NC; k++) {
    best[k] = -INFINITY;
    arg[k] = 0x7FFFFFFF;
  }
#pragma unroll 4
  for (int j = b; j < e; j++) {
    const int r = plist[j];
    if ((unsigned)r >= (unsigned)n_cap) continue;
#pragma unroll
    for (int k = 0; k < NC; k++) {
      const int c = lane + 64 * k;
      if (c < C) {
        const float v = x[(size_t)r * C + c];
        if (v > best[k] || (v == best[k] && r < arg[k])) {
          best[k] = v;
          arg[k] = r;
        }
      }
    }
  }
}

template <int NC>
__device__ __forceinline__ void pm_write_concat(const float *__restrict__ x, int n_cap, int C, const int *__restrict__ plist,
                                                int b, int e, int lane, const float best[NC], float *__restrict__ cat) {
#pragma unroll 4
  for (int j = b; j < e; j++) {
    const int r = plist[j];
    if ((unsigned)r >= (unsigned)n_cap) continue;
#pragma unroll
    for (int k = 0; k < NC; k++) {
      const int c = lane + 64 * k;
      if (c < C) {
        cat[(size_t)r * 2 * C + c] = x[(size_t)r * C + c];
        cat[(size_t)r * 2 * C + C + c] = best[k];
      }
    }
  }
}

// A workgroup takes MW consecutive pillars.  A pillar of at most LONG_PILLAR rows is one wave's; the rows of a longer
// one are cut into MW runs, one per wave, and the partial maxima meet in LDS in run order (ties keep the lowest row).
template <int NC>
__global__ __launch_bounds__(MW * 64) void k_pm_fwd(const float *__restrict__ x, int n_cap, int C,
                                                    const int *__restrict__ offsets, const int *__restrict__ plist,
                                                    int p_cap, const int *__restrict__ sizes, float *__restrict__ x_max,
                                                    int *__restrict__ arg_out, float *__restrict__ cat) {
  __shared__ float s_v[MW][NC * 64];
  __shared__ int s_a[MW][NC * 64];
  const int P = sizes[1] < p_cap ? sizes[1] : p_cap;
  const int pb = blockIdx.x * MW;
  if (pb >= P) return;
  const int w = threadIdx.x >> 6, lane = lane_id();
  float best[NC];
  int arg[NC];
  const int p = pb + w;
  if (p < P) {
    const int s = offsets[p], n = offsets[p + 1] - s;
    if (n <= LONG_PILLAR) {
      pm_scan<NC>(x, n_cap, C, plist, s, s + n, lane, best, arg);
#pragma unroll
      for (int k = 0; k < NC; k++) {
        const int c = lane + 64 * k;
        if (c < C) {
          x_max[(size_t)p * C + c] = best[k];
          arg_out[(size_t)p * C + c] = arg[k];
        }
      }
      if (cat) pm_write_concat<NC>(x, n_cap, C, plist, s, s + n, lane, best, cat);
    }
  }
  for (int q = 0; q < MW && pb + q < P; q++) {               // the same trip for every thread of the workgroup
    const int pq = pb + q;
    const int s = offsets[pq], n = offsets[pq + 1] - s;
    if (n <= LONG_PILLAR) continue;
    const int part = (n + MW - 1) / MW;
    const int b = s + (w * part < n ? w * part : n), e = s + ((w + 1) * part < n ? (w + 1) * part : n);
    pm_scan<NC>(x, n_cap, C, plist, b, e, lane, best, arg);
#pragma unroll
    for (int k = 0; k < NC; k++) {
      s_v[w][lane + 64 * k] = best[k];
      s_a[w][lane + 64 * k] = arg[k];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < NC; k++) {
      best[k] = s_v[0][lane + 64 * k];
      arg[k] = s_a[0][lane + 64 * k];
      for (int u = 1; u < MW; u++) {
        const float v = s_v[u][lane + 64 * k];
        const int a = s_a[u][lane + 64 * k];
        if (v > best[k] || (v == best[k] && a < arg[k])) {
          best[k] = v;
          arg[k] = a;
        }
      }
      const int c = lane + 64 * k;
      if (w == 0 && c < C) {
        x_max[(size_t)pq * C + c] = best[k];
        arg_out[(size_t)pq * C + c] = arg[k];
      }
    }
    if (cat) pm_write_concat<NC>(x, n_cap, C, plist, b, e, lane, best, cat);
    __syncthreads();
  }
}

// One wave per pillar.  The sum over the pillar's rows is a chain of float adds in list order by definition; the loads
// that feed it do not depend on one another.
template <int NC>
__global__ __launch_bounds__(MW * 64) void k_pm_bwd(const float *__restrict__ g_max, const float *__restrict__ g_cat,
                                                    int n_cap, int C, const int *__restrict__ arg_in,
                                                    const int *__restrict__ offsets, const int *__restrict__ plist,
                                                    int p_cap, const int *__restrict__ sizes, float *__restrict__ gx) {
  const int P = sizes[1] < p_cap ? sizes[1] : p_cap;
  const int p = blockIdx.x * MW + (threadIdx.x >> 6);
  if (p >= P) return;
  const int lane = lane_id();
  const int s = offsets[p], e = offsets[p + 1];
  float sum[NC];
  int arg[NC];
#pragma unroll
  for (int k = 0; k < NC; k++) {
    const int c = lane + 64 * k;
    arg[k] = c < C ? arg_in[(size_t)p * C + c] : -1;
    sum[k] = (g_max && c < C) ? g_max[(size_t)p * C + c] : 0.0f;
  }
  if (g_cat) {
#pragma unroll 4
    for (int j = s; j < e; j++) {
      const int r = plist[j];
      if ((unsigned)r >= (unsigned)n_cap) continue;
#pragma unroll
      for (int k = 0; k < NC; k++) {
        const int c = lane + 64 * k;
        if (c < C) sum[k] += g_cat[(size_t)r * 2 * C + C + c];
      }
    }
  }
#pragma unroll 4
  for (int j = s; j < e; j++) {
    const int r = plist[j];
    if ((unsigned)r >= (unsigned)n_cap) continue;
#pragma unroll
    for (int k = 0; k < NC; k++) {
      const int c = lane + 64 * k;
      if (c < C) {
        const float routed = arg[k] == r ? sum[k] : 0.0f;
        gx[(size_t)r * C + c] = g_cat ? g_cat[(size_t)r * 2 * C + c] + routed : routed;
      }
    }
  }
}

inline unsigned blocks_for(int64_t n, int per) { return (unsigned)((n + per - 1) / per); }

}  // namespace

extern "C" int32_t dfu3d_vfe_version(void) { return DFU3D_VFE_VERSION; }

extern "C" int64_t dfu3d_vfe_scratch_bytes(int64_t n_points, int64_t n_cells) {
  if (n_points < 0 || n_cells < 0 || n_points > 0x7FFFFFFF || n_cells > DFU3D_VFE_MAX_CELLS) return -1;
  return (int64_t)pv_scratch(n_points, n_cells).bytes;
}

extern "C" int dfu3d_pillar_group(const float *points, int32_t n_points, int32_t point_cols, int32_t batch_size,
                                  float range_x, float range_y, float voxel_x, float voxel_y, int32_t nx, int32_t ny,
                                  int32_t layout, int32_t *kept_idx, int32_t *unq_inv, int32_t *unq_cnt,
                                  int32_t *coords, int32_t *offsets, int32_t *plist, int32_t *sizes, uint32_t *status,
                                  void *scratch, int64_t scratch_bytes, void *stream) {
  DFU3D_CLEAR_STALE_ERROR();
  if (!kept_idx || !unq_inv || !unq_cnt || !coords || !offsets || !plist || !sizes || !status || !scratch)
    return DFU3D_EINVAL;
  if (n_points < 0 || point_cols < 4 || batch_size < 1 || nx < 1 || ny < 1 || !(voxel_x > 0.0f) || !(voxel_y > 0.0f) ||
      !(range_x - range_x == 0.0f) || !(range_y - range_y == 0.0f))
    return DFU3D_EINVAL;
  if (layout != DFU3D_VFE_LAYOUT_PILLAR && layout != DFU3D_VFE_LAYOUT_SIMPLE2D) return DFU3D_EINVAL;
  if (!points && n_points > 0) return DFU3D_EINVAL;
  if (point_cols > DFU3D_VFE_MAX_POINT_COLS) return DFU3D_ERANGE;
  const int64_t cells = (int64_t)batch_size * nx * ny;
  if ((int64_t)nx * ny > DFU3D_VFE_MAX_CELLS || cells > DFU3D_VFE_MAX_CELLS) return DFU3D_ERANGE;
  if ((int64_t)n_points * point_cols > 0x7FFFFFFF) return DFU3D_ERANGE;
  const PvScratch L = pv_scratch(n_points, cells);
  if (((uintptr_t)scratch & 15u) || scratch_bytes < (int64_t)L.bytes) return DFU3D_EINVAL;
  char *S = (char *)scratch;
  int *key = (int *)(S + L.key), *slot = (int *)(S + L.slot), *tmp = (int *)(S + L.tmp);
  int *blk_cnt = (int *)(S + L.blk_cnt), *blk_off = (int *)(S + L.blk_off), *wpre = (int *)(S + L.wpre);
  uint32_t *bitmap = (uint32_t *)(S + L.bitmap);
  hipStream_t st = (hipStream_t)stream;
  const PvGeom g{range_x, range_y, voxel_x, voxel_y, nx, ny, batch_size, layout};
  const int64_t clear_items = n_points == 0 ? 1 : (L.words > L.p_cap ? L.words : L.p_cap);
  const unsigned clear_grid = blocks_for(clear_items, PT) < 2048u ? blocks_for(clear_items, PT) : 2048u;
  hipLaunchKernelGGL(k_pv_clear, dim3(clear_grid), dim3(PT), 0, st, bitmap, n_points == 0 ? (int64_t)0 : L.words,
                     unq_cnt, L.p_cap, offsets, sizes, status);
  DFU3D_LAUNCH_CHECK();
  if (n_points == 0) return DFU3D_OK;
  const unsigned grid = blocks_for(n_points, PT);
  hipLaunchKernelGGL(k_pv_mark, dim3(grid), dim3(PT), 0, st, points, n_points, point_cols, g, key, bitmap, blk_cnt,
                     status);
  DFU3D_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_pv_scan, dim3(1), dim3(ST), 0, st, bitmap, (int)L.words, wpre, blk_cnt, (int)L.blocks, blk_off,
                     sizes);
  DFU3D_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_pv_rank, dim3(grid), dim3(PT), 0, st, key, n_points, g, bitmap, wpre, blk_off, kept_idx, unq_inv,
                     unq_cnt, slot, coords);
  DFU3D_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_pv_offsets, dim3(1), dim3(ST), 0, st, unq_cnt, sizes, offsets);
  DFU3D_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_pv_place, dim3(grid), dim3(PT), 0, st, sizes, unq_inv, slot, offsets, tmp);
  DFU3D_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_pv_sort, dim3(grid), dim3(PT), 0, st, sizes, unq_inv, offsets, tmp, plist);
  DFU3D_LAUNCH_CHECK();
  return DFU3D_OK;
}

extern "C" int dfu3d_pillar_features(const float *points, int32_t n_points, int32_t point_cols, float range_x,
                                     float range_y, float voxel_x, float voxel_y, float offset_x, float offset_y,
                                     float offset_z, int32_t layout, int32_t use_abs_xyz, int32_t with_distance,
                                     const int32_t *kept_idx, const int32_t *unq_inv, const int32_t *offsets,
                                     const int32_t *plist, const int32_t *sizes, float *features, int32_t feat_cols,
                                     void *scratch, int64_t scratch_bytes, void *stream) {
  DFU3D_CLEAR_STALE_ERROR();
  if (!kept_idx || !unq_inv || !offsets || !plist || !sizes || !features || !scratch) return DFU3D_EINVAL;
  if (n_points < 0 || point_cols < 4 || !(voxel_x > 0.0f) || !(voxel_y > 0.0f)) return DFU3D_EINVAL;
  if (layout != DFU3D_VFE_LAYOUT_PILLAR && layout != DFU3D_VFE_LAYOUT_SIMPLE2D) return DFU3D_EINVAL;
  if (!points && n_points > 0) return DFU3D_EINVAL;
  if (point_cols > DFU3D_VFE_MAX_POINT_COLS) return DFU3D_ERANGE;
  const int raw = use_abs_xyz ? point_cols - 1 : point_cols - 4;
  const int want = raw + (layout == DFU3D_VFE_LAYOUT_PILLAR ? 6 : 3) + (with_distance ? 1 : 0);
  if (feat_cols != want) return DFU3D_EINVAL;
  if ((int64_t)n_points * point_cols > 0x7FFFFFFF || (int64_t)n_points * feat_cols > 0x7FFFFFFF) return DFU3D_ERANGE;
  if (((uintptr_t)scratch & 15u) || scratch_bytes < (int64_t)n_points * 12) return DFU3D_EINVAL;
  if (n_points == 0) return DFU3D_OK;
  float *mean = (float *)scratch;                      // over the grouping's key / slot / tmp (pv_scratch)
  hipStream_t st = (hipStream_t)stream;
  if (layout == DFU3D_VFE_LAYOUT_PILLAR) {
    hipLaunchKernelGGL(k_pv_mean, dim3(blocks_for(n_points, PW)), dim3(64), 0, st, points, point_cols, kept_idx, offsets,
                       plist, sizes, mean);
    DFU3D_LAUNCH_CHECK();
  }
  const PfCfg g{range_x, range_y, voxel_x, voxel_y, offset_x, offset_y, offset_z, layout, use_abs_xyz ? 1 : 0,
                with_distance ? 1 : 0, point_cols, feat_cols};
  hipLaunchKernelGGL(k_pv_feat, dim3(blocks_for(n_points, PT)), dim3(PT), 0, st, points, g, kept_idx, unq_inv, sizes, mean,
                     features);
  DFU3D_LAUNCH_CHECK();
  return DFU3D_OK;
}

extern "C" int dfu3d_pillar_max(const float *x, int32_t n_cap, int32_t C, const int32_t *offsets, const int32_t *plist,
                                int32_t p_cap, const int32_t *sizes, float *x_max, int32_t *arg, float *concat,
                                void *stream) {
  DFU3D_CLEAR_STALE_ERROR();
  if (!offsets || !plist || !sizes || !x_max || !arg) return DFU3D_EINVAL;
  if (n_cap < 0 || p_cap < 0 || C < 1) return DFU3D_EINVAL;
  if (C > DFU3D_VFE_MAX_CHANNELS) return DFU3D_ERANGE;
  if (!x && n_cap > 0) return DFU3D_EINVAL;
  if ((int64_t)n_cap * 2 * C > 0x7FFFFFFF) return DFU3D_ERANGE;
  if (n_cap == 0 || p_cap == 0) return DFU3D_OK;
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid(blocks_for(p_cap, MW)), block(MW * 64);
  if (C <= 64)
    hipLaunchKernelGGL(k_pm_fwd<1>, grid, block, 0, st, x, n_cap, C, offsets, plist, p_cap, sizes, x_max, arg, concat);
  else if (C <= 128)
    hipLaunchKernelGGL(k_pm_fwd<2>, grid, block, 0, st, x, n_cap, C, offsets, plist, p_cap, sizes, x_max, arg, concat);
  else
    hipLaunchKernelGGL(k_pm_fwd<4>, grid, block, 0, st, x, n_cap, C, offsets, plist, p_cap, sizes, x_max, arg, concat);
  DFU3D_LAUNCH_CHECK();
  return DFU3D_OK;
}

extern "C" int dfu3d_pillar_max_backward(const float *grad_max, const float *grad_concat, int32_t n_cap, int32_t C,
                                         const int32_t *arg, const int32_t *offsets, const int32_t *plist, int32_t p_cap,
                                         const int32_t *sizes, float *grad_x, void *stream) {
  DFU3D_CLEAR_STALE_ERROR();
  if (!arg || !offsets || !plist || !sizes || !grad_x) return DFU3D_EINVAL;
  if ((grad_max == nullptr) == (grad_concat == nullptr)) return DFU3D_EINVAL;
  if (n_cap < 0 || p_cap < 0 || C < 1) return DFU3D_EINVAL;
  if (C > DFU3D_VFE_MAX_CHANNELS) return DFU3D_ERANGE;
  if ((int64_t)n_cap * 2 * C > 0x7FFFFFFF) return DFU3D_ERANGE;
  if (n_cap == 0 || p_cap == 0) return DFU3D_OK;
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid(blocks_for(p_cap, MW)), block(MW * 64);
  if (C <= 64)
    hipLaunchKernelGGL(k_pm_bwd<1>, grid, block, 0, st, grad_max, grad_concat, n_cap, C, arg, offsets, plist, p_cap, sizes,
                       grad_x);
  else if (C <= 128)
    hipLaunchKernelGGL(k_pm_bwd<2>, grid, block, 0, st, grad_max, grad_concat, n_cap, C, arg, offsets, plist, p_cap, sizes,
                       grad_x);
  else
    hipLaunchKernelGGL(k_pm_bwd<4>, grid, block, 0, st, grad_max, grad_concat, n_cap, C, arg, offsets, plist, p_cap, sizes,
                       grad_x);
  DFU3D_LAUNCH_CHECK();
  return DFU3D_OK;
}
