// hardvoxel_stage.hip -- SURVEY.md §8 row f-19: DataProcessor.transform_points_to_voxels and MeanVFE for a whole batch
// (csrc/dfu3d_hvox.h): per scene at most max_voxels voxels in first-seen order with at most max_points rows each, in
// seven launches, without a read from the device and without anything of the grid's size.
//
// What it stands in for: per scene a sequential pass of a host voxel generator over a dense table of the grid
// (90 million cells at KITTI's 0.05 / 0.05 / 0.1 m), and MeanVFE's sum over the (V, T, C) block it returns.
//
// The rule is sequential in the row index; here it is taken apart into three order-free questions.
//   1. Which row is the first of its cell?  An open-addressing hash over 64-bit (scene, cell) keys (compare-and-swap on
//      the key, linear probing, load at most 1 / DFU3D_HVOX_TABLE_PER_ROW) with an integer atomicMin of the row and an
//      integer count per entry: which entry a cell gets depends on the arrival order, nothing that is kept does.
//   2. Which voxel id does a cell get?  Its rank among the scene's first rows: an ordered scan of the flag "is the first
//      row of its cell" over ALL rows (block counts, one workgroup scans them, every block ranks its own rows), minus the
//      scan's value at the scene's first row.  A rank at or beyond max_voxels makes no voxel.  The same scan carries
//      min(rows of the cell, max_points), which gives every cell a list of exactly that length inside ONE block of R ints.
//   3. Which rows are stored, in which slot?  The len smallest rows of the cell, ascending.  Every row walks its cell's
//      list with atomicMin, keeps the larger value and carries it on: position k ends as the k-th smallest whatever the
//      order of arrival (what is carried out of a position is everything that went in but its minimum).  A row leaves at
//      once when the list's last entry is already below it (entries only fall), skips entries below it with a plain
//      load, and of the rows one wave holds of one cell only the first len start at all: a cell of thousands of rows costs
//      about len * len / 2 atomics, not a sort, and a wave full of one ground cell does not queue 64 deep on one word.
//
//   k_hvox_init     fills: table keys, first rows, counts, the lists, point_voxel = -1; workgroup 0: the scenes' first rows
//   k_hvox_insert   a thread per row: scene, cell, table entry
//   k_hvox_count    a workgroup per 1024 rows: first rows and list lengths of the block
//   k_hvox_offsets  one workgroup: prefix of both over the blocks, the scan's value at every scene's start, voxel_cnt,
//                   every scene's first output row, n_voxels
//   k_hvox_assign   a workgroup per 1024 rows: a first row gives its cell the voxel (or none) and writes voxel_coords
//   k_hvox_place    a thread per row: the slot lists
//   k_hvox_emit     a thread per output element: voxels, voxel_mean, voxel_num_points, point_voxel, the tails
//
// A bad count table (DFU3D_HVOX_ST_BAD_COUNT) reads nothing outside `points`: the scenes are cut at R.
#include <limits.h>

#include "common.hpp"
#include "dfu3d_hvox.h"

namespace {

constexpr int PT = DFU3D_HVOX_ROW_THREADS;              // threads of every kernel but the last; rows of a block
constexpr int PW = PT / 64;                             // its waves
constexpr int OT = DFU3D_HVOX_OUT_THREADS;              // threads of k_hvox_emit
constexpr int LEN_SHIFT = 11;                           // one int of a block's scan: first rows below, list lengths above
constexpr unsigned long long EMPTY = ~0ull;
static_assert(PT == 1024, "a block's count of first rows fills LEN_SHIFT bits; g >> 10 is the block of row g");
static_assert((long long)PT * DFU3D_HVOX_MAX_POINTS < (1ll << (31 - LEN_SHIFT)), "a block's list lengths fit the rest");

// THE layout of the scratch of dfu3d_hard_voxels; the size is its last field
struct HvScratch {
  size_t keys;                                          // uint64 (H)
  size_t first, cnt, vox;                               // int32 (H) each: first row, rows, output row or -1
  size_t row_slot, list;                                // int32 (R) each: the row's table entry or -1; the slot lists
  size_t vox_off, vox_len;                              // int32 (R) each, by output row: its list
  size_t pre1, pre2;                                    // int32 (blocks + 1) each: first rows / list lengths before a block
  size_t scene_first, scene_g1;                         // int32 (B + 1) each: first row of a scene, first rows before it
  size_t vox_base;                                      // int32 (B): output rows before a scene
  size_t bytes;
  long long H;                                          // entries of the table (a valid call's fit an int)
  int blocks;
};

inline size_t up16(size_t v) { return (v + 15u) & ~(size_t)15u; }

HvScratch hv_scratch(int B, int R) {
  HvScratch s;
  long long h = 16;
  while (h < (long long)DFU3D_HVOX_TABLE_PER_ROW * R) h *= 2;
  s.H = h;
  s.blocks = (int)(((long long)R + PT - 1) / PT);
  size_t o = 0;
  s.keys = o; o += up16((size_t)s.H * 8);
  s.first = o; o += up16((size_t)s.H * 4);
  s.cnt = o; o += up16((size_t)s.H * 4);
  s.vox = o; o += up16((size_t)s.H * 4);
  s.row_slot = o; o += up16((size_t)R * 4);
  s.list = o; o += up16((size_t)R * 4);
  s.vox_off = o; o += up16((size_t)R * 4);
  s.vox_len = o; o += up16((size_t)R * 4);
  s.pre1 = o; o += up16(((size_t)s.blocks + 1) * 4);
  s.pre2 = o; o += up16(((size_t)s.blocks + 1) * 4);
  s.scene_first = o; o += up16(((size_t)B + 1) * 4);
  s.scene_g1 = o; o += up16(((size_t)B + 1) * 4);
  s.vox_base = o; o += up16((size_t)B * 4);
  s.bytes = o;
  return s;
}

struct HvGeom {
  float rx, ry, rz, vx, vy, vz;
  int gx, gy, gz;
};

// THE RULE's cell of one row: every operation rounded on its own, the comparisons on floats.  false: OUT
__device__ __forceinline__ bool hv_axis(float p, float rmin, float vs, int grid, int &c) {
  const float q = floorf(__fdiv_rn(__fsub_rn(p, rmin), vs));
  c = 0;
  if (!(q >= 0.0f) || !(q < (float)grid)) return false;
  c = (int)q;
  return true;
}
__device__ __forceinline__ bool hv_cell(const float *__restrict__ row, const HvGeom &G, int &cx, int &cy, int &cz) {
  const bool ox = hv_axis(row[1], G.rx, G.vx, G.gx, cx);
  const bool oy = hv_axis(row[2], G.ry, G.vy, G.gy, cy);
  const bool oz = hv_axis(row[3], G.rz, G.vz, G.gz, cz);
  return ox && oy && oz;
}
__device__ __forceinline__ bool hv_finite(float v) { return (__float_as_uint(v) & 0x7F800000u) != 0x7F800000u; }

__global__ __launch_bounds__(PT) void k_hvox_init(const int *__restrict__ point_cnt, int B, int R, int H,
                                                  unsigned long long *keys, int *first, int *cnt, int *list,
                                                  int *point_voxel, int *scene_first, int *status) {
  __shared__ unsigned long long s_part[PT];
  __shared__ int s_bad;
  const int t = threadIdx.x;
  const size_t tid = (size_t)blockIdx.x * PT + t, nth = (size_t)gridDim.x * PT;
  for (size_t i = tid; i < (size_t)H; i += nth) {
    keys[i] = EMPTY;
    first[i] = INT_MAX;
    cnt[i] = 0;
  }
  for (size_t i = tid; i < (size_t)R; i += nth) {
    list[i] = INT_MAX;
    point_voxel[i] = -1;
  }
  if (blockIdx.x != 0) return;                              // (uniform)
  // the scenes' first rows: thread t sums `per` consecutive counts, then adds the sums of the threads before it
  const int per = (B + PT - 1) / PT;
  const int i0 = min(t * per, B), i1 = min(i0 + per, B);
  unsigned long long sum = 0ull;
  bool bad = false;
  for (int i = i0; i < i1; i++) {
    const int c = point_cnt[i];
    bad |= c < 0;
    sum += (unsigned long long)max(c, 0);
  }
  s_part[t] = sum;
  if (t == 0) s_bad = 0;
  __syncthreads();
  if (i0 < i1) {
    unsigned long long run = 0ull;
    for (int w = 0; w < t; w++) run += s_part[w];
    for (int i = i0; i < i1; i++) {
      scene_first[i] = (int)min(run, (unsigned long long)R);
      run += (unsigned long long)max(point_cnt[i], 0);
    }
    if (i1 == B) {
      scene_first[B] = (int)min(run, (unsigned long long)R);
      bad |= run > (unsigned long long)R;
    }
  }
  if (bad) atomicOr(&s_bad, 1);
  __syncthreads();
  if (t == 0 && s_bad) atomicOr(status, DFU3D_HVOX_ST_BAD_COUNT);
}

__global__ __launch_bounds__(PT) void k_hvox_insert(const float *__restrict__ points, int B, int R, int C, HvGeom G, int H,
                                                    const int *__restrict__ scene_first, unsigned long long *keys,
                                                    int *first, int *cnt, int *row_slot, int *status) {
  const long long gl = (long long)blockIdx.x * PT + threadIdx.x;
  if (gl >= R) return;
  const int g = (int)gl;
  int slot = -1;
  if (g < scene_first[B]) {
    const float *row = points + (size_t)g * (1 + C);
    int cx, cy, cz;
    if (!(hv_finite(row[1]) && hv_finite(row[2]) && hv_finite(row[3]))) {
      atomicOr(status, DFU3D_HVOX_ST_BAD_POINT);
    } else if (hv_cell(row, G, cx, cy, cz)) {
      const int b = last_at_or_below(scene_first, 0, B, g);
      const unsigned long long key =
          ((((unsigned long long)b * G.gz + cz) * (unsigned long long)G.gy + cy) * (unsigned long long)G.gx) + cx;
      unsigned h = (unsigned)mix64(key) & (unsigned)(H - 1);
      for (int probe = 0; probe < H; probe++) {             // (the load is at most 1/2: an empty entry is always met)
        unsigned long long cur = __hip_atomic_load(&keys[h], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (cur == EMPTY) cur = atomicCAS(&keys[h], EMPTY, key);
        if (cur == EMPTY || cur == key) { slot = (int)h; break; }
        h = (h + 1u) & (unsigned)(H - 1);
      }
      if (slot >= 0) {
        atomicMin(&first[slot], g);
        atomicAdd(&cnt[slot], 1);
      }
    }
  }
  row_slot[g] = slot;
}

// is row g the first of its cell, and how long is the cell's list: flag | len << LEN_SHIFT
__device__ __forceinline__ int hv_first_word(long long g, int R, int T, const int *__restrict__ row_slot,
                                             const int *__restrict__ first, const int *__restrict__ cnt, int &slot) {
  slot = g < R ? row_slot[g] : -1;
  if (slot < 0 || first[slot] != (int)g) return 0;
  return 1 | (min(cnt[slot], T) << LEN_SHIFT);
}

__global__ __launch_bounds__(PT) void k_hvox_count(int R, int T, const int *__restrict__ row_slot,
                                                   const int *__restrict__ first, const int *__restrict__ cnt, int *pre1,
                                                   int *pre2) {
  __shared__ int s_w[PW];
  int slot;
  const int word = hv_first_word((long long)blockIdx.x * PT + threadIdx.x, R, T, row_slot, first, cnt, slot);
  const int tot = block_sum_i<PW>(word, s_w);
  if (threadIdx.x == 0) {
    pre1[blockIdx.x] = tot & ((1 << LEN_SHIFT) - 1);
    pre2[blockIdx.x] = tot >> LEN_SHIFT;
  }
}

__global__ __launch_bounds__(PT) void k_hvox_offsets(int B, int R, int blocks, int max_voxels,
                                                     const int *__restrict__ row_slot, const int *__restrict__ first,
                                                     const int *__restrict__ scene_first, int *pre1, int *pre2,
                                                     int *scene_g1, int *vox_base, int *voxel_cnt, int *n_voxels) {
  __shared__ int s_w[PW];
  const int t = threadIdx.x;
  const int tot1 = block_scan_range<PT, 4, int, int>(blocks, [&](int i) { return pre1[i]; },
                                                     [&](int i, int v) { pre1[i] = v; }, s_w);
  const int tot2 = block_scan_range<PT, 4, int, int>(blocks, [&](int i) { return pre2[i]; },
                                                     [&](int i, int v) { pre2[i] = v; }, s_w);
  if (t == 0) {
    pre1[blocks] = tot1;
    pre2[blocks] = tot2;
  }
  __syncthreads();
  // first rows before every scene's first row (and before the end of the last): a wave per scene counts the part of
  // the block the scene starts in
  for (int b = t >> 6; b <= B; b += PW) {                   // (uniform in the wave)
    const int g0 = scene_first[b], blk = g0 >> 10;
    int mine = 0;
    for (int r = blk * PT + (t & 63); r < g0; r += 64) {
      const int slot = row_slot[r];
      mine += (slot >= 0 && first[slot] == r) ? 1 : 0;
    }
    mine = wave_sum_i(mine);
    if ((t & 63) == 0) scene_g1[b] = pre1[blk] + mine;
  }
  __syncthreads();
  auto vcnt = [&](int b) { return min(scene_g1[b + 1] - scene_g1[b], max_voxels); };
  const int total = block_scan_range<PT, 1, int, int>(B, vcnt, [&](int b, int v) { vox_base[b] = v; }, s_w);
  for (int b = t; b < B; b += PT) voxel_cnt[b] = vcnt(b);
  if (t == 0) n_voxels[0] = total;
}

__global__ __launch_bounds__(PT) void k_hvox_assign(const float *__restrict__ points, int B, int R, int C, HvGeom G, int T,
                                                    int max_voxels, const int *__restrict__ row_slot,
                                                    const int *__restrict__ first, const int *__restrict__ cnt,
                                                    const int *__restrict__ pre1, const int *__restrict__ pre2,
                                                    const int *__restrict__ scene_first,
                                                    const int *__restrict__ scene_g1, const int *__restrict__ vox_base,
                                                    int *vox, int *vox_off, int *vox_len, int *voxel_coords) {
  __shared__ int s_w[PW];
  const long long g = (long long)blockIdx.x * PT + threadIdx.x;
  int slot, tot;
  const int word = hv_first_word(g, R, T, row_slot, first, cnt, slot);
  const int ex = block_excl_scan<PW>(word, s_w, tot);
  if (!word) return;
  const int b = last_at_or_below(scene_first, 0, B, (int)g);
  const int rank = pre1[blockIdx.x] + (ex & ((1 << LEN_SHIFT) - 1)) - scene_g1[b];
  if (rank >= max_voxels) {
    vox[slot] = -1;
    return;
  }
  const int v = vox_base[b] + rank;
  vox[slot] = v;
  vox_off[v] = pre2[blockIdx.x] + (ex >> LEN_SHIFT);
  vox_len[v] = word >> LEN_SHIFT;
  int cx, cy, cz;
  hv_cell(points + (size_t)g * (1 + C), G, cx, cy, cz);
  int *out = voxel_coords + (size_t)v * 4;
  out[0] = b;
  out[1] = cz;
  out[2] = cy;
  out[3] = cx;
}

__global__ __launch_bounds__(PT) void k_hvox_place(int R, const int *__restrict__ row_slot, const int *__restrict__ vox,
                                                   const int *__restrict__ vox_off, const int *__restrict__ vox_len,
                                                   int *list) {
  const long long gl = (long long)blockIdx.x * PT + threadIdx.x;
  const int g = (int)gl;
  const int slot = gl < R ? row_slot[g] : -1;
  const int v = slot >= 0 ? vox[slot] : -1;
  bool act = v >= 0;
  const int off = act ? vox_off[v] : 0, len = act ? vox_len[v] : 0;
  // of the rows this wave holds of one cell (ascending with the lane) only the first len can be stored: up to four
  // cells are thinned so, by ballot; what is left of the wave goes on as it is
  unsigned long long rem = __ballot(act);
  const unsigned long long below = (1ull << lane_id()) - 1ull;
  for (int r = 0; r < 4 && rem; r++) {                      // (uniform)
    const int leader = __ffsll((long long)rem) - 1;
    const int lv = __shfl(v, leader, 64);
    const bool same = act && v == lv;
    const unsigned long long sm = __ballot(same);
    if (same && __popcll(sm & below) >= len) act = false;
    rem &= ~sm;
  }
  if (!act) return;
  int *a = list + off;
  if (__hip_atomic_load(&a[len - 1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < g) return;
  int carry = g;
  for (int k = 0; k < len; k++) {
    if (__hip_atomic_load(&a[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < carry) continue;
    const int old = atomicMin(&a[k], carry);
    if (old == INT_MAX) break;
    carry = max(old, carry);
  }
}

__global__ __launch_bounds__(OT) void k_hvox_emit(const uint32_t *__restrict__ points, int R, int C, int T, int out_cols,
                                                  int per_vox, long long total, const int *__restrict__ n_voxels,
                                                  const int *__restrict__ vox_off, const int *__restrict__ vox_len,
                                                  const int *__restrict__ list, int *voxel_coords,
                                                  int *voxel_num_points, uint32_t *voxels, float *voxel_mean,
                                                  int *point_voxel) {
  const long long e = (long long)blockIdx.x * OT + threadIdx.x;
  if (e >= total) return;
  const int v = (int)(e / per_vox), j = (int)(e - (long long)v * per_vox);
  const bool live = v < n_voxels[0];
  const int len = live ? min(vox_len[v], T) : 0;
  const int *rows = list + (live ? vox_off[v] : 0);
  const int W = 1 + C;
  if (voxels && j < T * out_cols) {
    const int s = j / out_cols, c = j - s * out_cols;
    uint32_t val = 0u;
    if (s < len) {
      const int r = rows[s];
      if ((unsigned)r < (unsigned)R) val = points[(size_t)r * W + 1 + c];
    }
    voxels[(size_t)v * T * out_cols + j] = val;
  }
  if (j < T && j < len) {
    const int r = rows[j];
    if ((unsigned)r < (unsigned)R) point_voxel[r] = v;
  }
  if (voxel_mean && j < out_cols) {
    float acc = 0.0f;
    for (int s = 0; s < len; s++) {
      const int r = rows[s];
      if ((unsigned)r < (unsigned)R) acc = __fadd_rn(acc, __uint_as_float(points[(size_t)r * W + 1 + j]));
    }
    voxel_mean[(size_t)v * out_cols + j] = __fdiv_rn(acc, (float)max(len, 1));
  }
  if (j == 0) {
    voxel_num_points[v] = len;
    if (!live) {
      for (int k = 0; k < 4; k++) voxel_coords[(size_t)v * 4 + k] = -1;
    }
  }
}

bool hv_sizes_ok(int B, int R) { return B >= 0 && R >= 0 && B <= DFU3D_HVOX_MAX_BATCH; }

bool hv_finite_host(float v) {
  uint32_t u;
  memcpy(&u, &v, 4);
  return (u & 0x7F800000u) != 0x7F800000u;
}

}  // namespace

static_assert(DFU3D_HVOX_LAUNCHES == 7, "init, insert, count, offsets, assign, place, emit");

extern "C" int32_t dfu3d_hvox_version(void) { return DFU3D_HVOX_VERSION; }

extern "C" size_t dfu3d_hvox_scratch_bytes(int32_t B, int32_t R) {
  if (!hv_sizes_ok(B, R) || B == 0) return 0;
  return hv_scratch(B, R).bytes;
}

extern "C" int dfu3d_hard_voxels(const float *points, const int32_t *point_cnt, int32_t B, int32_t R, int32_t C,
                                 const float *range_min, const float *voxel_size, const int32_t *grid,
                                 int32_t max_points, int32_t max_voxels, int32_t out_cols, void *scratch,
                                 size_t scratch_bytes, int32_t *voxel_cnt, int32_t *n_voxels, int32_t *voxel_coords,
                                 int32_t *voxel_num_points, float *voxels, float *voxel_mean, int32_t *point_voxel,
                                 int32_t *status, void *stream) {
  DFU3D_CLEAR_STALE_ERROR();
  if (!point_cnt || !range_min || !voxel_size || !grid || !scratch || !voxel_cnt || !n_voxels || !status)
    return DFU3D_EINVAL;
  if (!voxels && !voxel_mean) return DFU3D_EINVAL;
  if (B < 0 || R < 0 || C < 3 || out_cols < 3 || out_cols > C || max_points < 1 || max_voxels < 1) return DFU3D_EINVAL;
  for (int j = 0; j < 3; j++) {
    if (grid[j] < 1 || !hv_finite_host(range_min[j]) || !hv_finite_host(voxel_size[j]) || !(voxel_size[j] > 0.0f))
      return DFU3D_EINVAL;
  }
  if (R > 0 && (!points || !point_voxel)) return DFU3D_EINVAL;
  const int64_t v_cap = (int64_t)B * max_voxels < (int64_t)R ? (int64_t)B * max_voxels : (int64_t)R;
  if (v_cap > 0 && (!voxel_coords || !voxel_num_points)) return DFU3D_EINVAL;
  if (max_points > DFU3D_HVOX_MAX_POINTS || B > DFU3D_HVOX_MAX_BATCH) return DFU3D_ERANGE;
  {
    unsigned __int128 cells = (unsigned __int128)(B > 0 ? B : 1);
    for (int j = 0; j < 3; j++) cells *= (unsigned __int128)grid[j];
    if (cells >= ((unsigned __int128)1 << DFU3D_HVOX_KEY_BITS)) return DFU3D_ERANGE;
  }
  if ((int64_t)R * (1 + (int64_t)C) > (int64_t)DFU3D_HVOX_MAX_ELEMS) return DFU3D_ERANGE;
  if (v_cap * 4 > (int64_t)DFU3D_HVOX_MAX_ELEMS) return DFU3D_ERANGE;
  if (v_cap * max_points * out_cols > (int64_t)DFU3D_HVOX_MAX_ELEMS) return DFU3D_ERANGE;
  if (B == 0) return DFU3D_OK;
  const HvScratch S = hv_scratch(B, R);
  if (((uintptr_t)scratch & 15u) || scratch_bytes < S.bytes) return DFU3D_EINVAL;
  char *base = (char *)scratch;
  hipStream_t st = (hipStream_t)stream;
  unsigned long long *keys = (unsigned long long *)(base + S.keys);
  int *first = (int *)(base + S.first), *cnt = (int *)(base + S.cnt), *vox = (int *)(base + S.vox);
  int *row_slot = (int *)(base + S.row_slot), *list = (int *)(base + S.list);
  int *vox_off = (int *)(base + S.vox_off), *vox_len = (int *)(base + S.vox_len);
  int *pre1 = (int *)(base + S.pre1), *pre2 = (int *)(base + S.pre2);
  int *scene_first = (int *)(base + S.scene_first), *scene_g1 = (int *)(base + S.scene_g1);
  int *vox_base = (int *)(base + S.vox_base);
  const HvGeom G = {range_min[0], range_min[1], range_min[2], voxel_size[0], voxel_size[1], voxel_size[2],
                    grid[0], grid[1], grid[2]};
  const unsigned row_grid = (unsigned)(S.blocks > 0 ? S.blocks : 1);
  const long long fill = S.H > (long long)R ? S.H : (long long)R;
  const long long fill_blocks = (fill + PT - 1) / PT;
  hipLaunchKernelGGL(k_hvox_init, dim3((unsigned)(fill_blocks < 2048 ? fill_blocks : 2048)), dim3(PT), 0, st,
                     (const int *)point_cnt, B, R, (int)S.H, keys, first, cnt, list, (int *)point_voxel, scene_first,
                     (int *)status);
  DFU3D_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_hvox_insert, dim3(row_grid), dim3(PT), 0, st, points, B, R, C, G, (int)S.H, (const int *)scene_first,
                     keys, first, cnt, row_slot, (int *)status);
  DFU3D_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_hvox_count, dim3(row_grid), dim3(PT), 0, st, R, max_points, (const int *)row_slot,
                     (const int *)first, (const int *)cnt, pre1, pre2);
  DFU3D_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_hvox_offsets, dim3(1), dim3(PT), 0, st, B, R, S.blocks, max_voxels, (const int *)row_slot,
                     (const int *)first, (const int *)scene_first, pre1, pre2, scene_g1, vox_base, (int *)voxel_cnt,
                     (int *)n_voxels);
  DFU3D_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_hvox_assign, dim3(row_grid), dim3(PT), 0, st, points, B, R, C, G, max_points, max_voxels,
                     (const int *)row_slot, (const int *)first, (const int *)cnt, (const int *)pre1, (const int *)pre2,
                     (const int *)scene_first, (const int *)scene_g1, (const int *)vox_base, vox, vox_off, vox_len,
                     (int *)voxel_coords);
  DFU3D_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_hvox_place, dim3(row_grid), dim3(PT), 0, st, R, (const int *)row_slot, (const int *)vox,
                     (const int *)vox_off, (const int *)vox_len, list);
  DFU3D_LAUNCH_CHECK();
  const int per_vox = voxels ? max_points * out_cols : (max_points > out_cols ? max_points : out_cols);
  const long long total = v_cap * per_vox;
  const long long out_blocks = (total + OT - 1) / OT;
  hipLaunchKernelGGL(k_hvox_emit, dim3((unsigned)(out_blocks > 0 ? out_blocks : 1)), dim3(OT), 0, st,
                     (const uint32_t *)points, R, C, max_points, out_cols, per_vox, total, (const int *)n_voxels,
                     (const int *)vox_off, (const int *)vox_len, (const int *)list, (int *)voxel_coords,
                     (int *)voxel_num_points, (uint32_t *)voxels, voxel_mean, (int *)point_voxel);
  DFU3D_LAUNCH_CHECK();
  return DFU3D_OK;
}
