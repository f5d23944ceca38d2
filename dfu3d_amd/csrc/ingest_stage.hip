// ingest_stage.hip -- SURVEY.md §8 row f-13: the batched FOV ingest (include/dfu3d_ingest.h).
//
// What it stands in for in the reference: KittiDataset.__getitem__'s FOV_POINTS_ONLY cut (kitti_dataset.py:480-486 over
// get_fov_flag :140-156 and calibration_kitti.py lidar_to_rect / rect_to_img) and get_infos' count of the kept points
// inside every labelled box (:262-275), one frame at a time in NumPy there, a whole batch of frames here.
//
//   k_ing_flag   the flat point array in chunks of DFU3D_ING_CHUNK rows, one row per thread (a C = 4 row is one 16-byte
//                load per lane, lane after lane): the row's scene from point_off, the scene's record and image shape,
//                the keep rule; the flag as one byte per row and the chunk's number of kept rows.  Block 0 checks the
//                offset tables and the image shapes.
//   k_ing_scan   one exclusive scan over the chunk counts; then out_off[b] for every b, one wave each: the prefix of the
//                chunk that holds row point_off[b] plus the flags of that chunk in front of the row.
//   k_ing_write  the flags again, a block rank, the kept rows to their place: all C columns, bit for bit.
//   k_ing_boxes  one workgroup per box: the kept rows of the box's scene through pt_in_box, one workgroup sum.
// The flat array is in scene order, so the one stable compaction is the scenes' concatenation.  The keep rule -- its
// arithmetic and its five comparisons, in_image_f32 -- and the search of a row's scene are common.hpp's, the box rule is
// pt_in_box.hpp's: nothing of them is restated here.
#include "common.hpp"
#include "dfu3d_ingest.h"
#include "pt_in_box.hpp"

namespace {

constexpr int PT = DFU3D_ING_CHUNK;                 // threads per workgroup = rows per chunk
constexpr int NW = PT / 64;
static_assert(PT == 4 * 64, "chunk: k_ing_scan reads a chunk's flags as one word per lane of one wave");

__global__ __launch_bounds__(PT) void k_ing_flag(const float *__restrict__ pts, long long n_rows, int C, bool vec4,
                                                 const long long *__restrict__ point_off, int B,
                                                 const ViewCalib *__restrict__ calib, const int *__restrict__ shape,
                                                 const int *__restrict__ box_off, int n_boxes, bool with_boxes,
                                                 unsigned char *__restrict__ keep, int *__restrict__ cnt,
                                                 uint32_t *__restrict__ status) {
  __shared__ int s_w[NW];
  const long long n_valid = valid_rows(point_off, B, n_rows);
  if (blockIdx.x == 0) {                             // the tables, once
    uint32_t bad = 0u;
    for (int b = threadIdx.x; b < B; b += PT) {
      const long long p0 = point_off[b], p1 = point_off[b + 1];
      if (!offsets_ok(p0, p1, n_rows, b)) bad |= (uint32_t)DFU3D_ING_ST_OFFSETS;
      const int h = shape[2 * b], w = shape[2 * b + 1];
      if (h < 0 || w < 0 || h > DFU3D_ING_MAX_SIDE || w > DFU3D_ING_MAX_SIDE) bad |= (uint32_t)DFU3D_ING_ST_SHAPE;
      if (with_boxes) {
        const int q0 = box_off[b], q1 = box_off[b + 1];
        if (q0 > q1 || q0 < 0 || q1 > n_boxes || (b == 0 && q0 != 0) || (b == B - 1 && q1 != n_boxes))
          bad |= (uint32_t)DFU3D_ING_ST_OFFSETS;
      }
    }
    if (bad) atomicOr(status, bad);
  }
  const long long c0 = (long long)blockIdx.x * PT;
  const long long c1 = (c0 + PT < n_valid ? c0 + PT : n_valid) - 1;
  int s_lo, s_hi;                                    // uniform over the workgroup
  scenes_of_chunk(point_off, B, c0, c1, s_lo, s_hi);
  const long long i = c0 + threadIdx.x;
  bool k = false;
  if (i < n_valid) {
    const int s = (s_lo == s_hi) ? s_lo : last_at_or_below(point_off, s_lo, s_hi + 1, i);
    const int h = shape[2 * s], w = shape[2 * s + 1];
    float x, y, z;
    if (vec4) {                                        // uniform: C = 4 and both arrays 16-byte aligned
      const float4 p = ((const float4 *)pts)[i];
      x = p.x; y = p.y; z = p.z;
    } else {
      const float *q = pts + (size_t)i * C;
      x = q[0]; y = q[1]; z = q[2];
    }
    const bool shape_ok = h >= 0 && w >= 0 && h <= DFU3D_ING_MAX_SIDE && w <= DFU3D_ING_MAX_SIDE;
    k = shape_ok && i >= point_off[s] && in_image_f32(calib[s].M43, calib[s].P2, x, y, z, (float)h, (float)w);
  }
  if (i < n_rows) keep[i] = k ? 1 : 0;
  const int tot = block_sum_i<NW>(k ? 1 : 0, s_w);
  if (threadIdx.x == 0) cnt[blockIdx.x] = tot;
}

__global__ __launch_bounds__(1024) void k_ing_scan(int n_chunks, const int *__restrict__ cnt, int *off,
                                                   const unsigned char *__restrict__ keep, long long n_rows,
                                                   const long long *__restrict__ point_off, int B,
                                                   long long *__restrict__ out_off) {
  __shared__ int s_w[16];
  const int total = block_scan_range<1024, 1, int, int>(
      n_chunks, [&](int c) { return cnt[c]; }, [&](int c, int ex) { off[c] = ex; }, s_w);
  __syncthreads();                                   // off[] is read below by other threads than its writers
  const long long n_valid = valid_rows(point_off, B, n_rows);
  // one wave per frame: the chunk's PT flag bytes are four per lane, one word each (the flag array is 8-byte aligned and a
  // chunk starts at a multiple of PT; the scratch has slack behind the last row), the bytes at or beyond the row masked off
  const int lane = lane_id();
  for (int b = threadIdx.x >> 6; b <= B; b += 1024 / 64) {           // uniform over the wave
    long long r = point_off[b];
    r = r < 0 ? 0 : (r < n_valid ? r : n_valid);     // a bad table (flagged by k_ing_flag) reads nothing outside
    const long long c = r / PT, j = c * PT + 4 * lane;
    int mine = 0;
    if (j < r) {
      uint32_t w = *(const uint32_t *)(keep + j);
      if (r - j < 4) w &= (1u << (8 * (int)(r - j))) - 1u;
      mine = __popc(w);                              // a flag byte is 0 or 1
    }
    const int before = wave_sum_i(mine);
    if (lane == 0) out_off[b] = (long long)(c < n_chunks ? off[c] : total) + before;
  }
}

__global__ __launch_bounds__(PT) void k_ing_write(const float *__restrict__ pts, long long n_rows, int C, bool vec4,
                                                  const unsigned char *__restrict__ keep,
                                                  const int *__restrict__ off, float *__restrict__ out) {
  __shared__ int s_w[NW];
  const long long i = (long long)blockIdx.x * PT + threadIdx.x;
  const bool k = i < n_rows && keep[i] != 0;
  int tot;
  const int r = block_rank<NW>(k, s_w, tot);
  if (!k) return;
  const long long d = (long long)off[blockIdx.x] + r;
  if (d > i) return;                                 // holds by construction (a compaction); never a store outside
  if (vec4) {                                        // uniform: C = 4 and both arrays 16-byte aligned
    ((float4 *)out)[d] = ((const float4 *)pts)[i];
  } else {
    const float *q = pts + (size_t)i * C;
    float *dst = out + (size_t)d * C;
    for (int c = 0; c < C; c++) dst[c] = q[c];
  }
}

__global__ __launch_bounds__(PT) void k_ing_boxes(const float *__restrict__ pts, long long n_rows, int C,
                                                  const long long *__restrict__ point_off, int B,
                                                  const unsigned char *__restrict__ keep,
                                                  const double *__restrict__ boxes, const int *__restrict__ box_off,
                                                  int *__restrict__ box_cnt) {
  __shared__ int s_w[NW];
  const int kb = blockIdx.x;
  const int s = last_at_or_below(box_off, 0, B, kb);     // uniform
  const bool owned = box_off[s] <= kb && kb < box_off[s + 1];
  const long long n_valid = valid_rows(point_off, B, n_rows);
  long long p0 = point_off[s], p1 = point_off[s + 1];
  p0 = p0 < 0 ? 0 : p0;
  p1 = p1 > n_valid ? n_valid : p1;
  if (!owned) p1 = p0;
  const BoxF q = load_box(boxes + (size_t)kb * 7);
  int mine = 0;
  for (long long i = p0 + threadIdx.x; i < p1; i += PT) {
    if (keep[i]) {
      const float *p = pts + (size_t)i * C;
      mine += pt_in_box(q, p[0], p[1], p[2]) ? 1 : 0;
    }
  }
  const int tot = block_sum_i<NW>(mine, s_w);
  if (threadIdx.x == 0) box_cnt[kb] = tot;
}

int64_t ing_chunks(int64_t n_rows) { return (n_rows + DFU3D_ING_CHUNK - 1) / DFU3D_ING_CHUNK; }

}  // namespace

extern "C" int32_t dfu3d_ing_version(void) { return DFU3D_ING_VERSION; }

extern "C" size_t dfu3d_fov_ingest_scratch_bytes(int64_t n_rows) {
  if (n_rows < 0 || n_rows > DFU3D_ING_MAX_ROWS) return 0;
  // at least one chunk: the launches have a fixed shape, an empty batch included
  const int64_t n_chunks = ing_chunks(n_rows) > 0 ? ing_chunks(n_rows) : 1;
  return (size_t)n_chunks * 2 * sizeof(int) + (size_t)((n_rows + 15) / 16) * 16 + 16;
}

extern "C" int dfu3d_fov_ingest(const float *points, int64_t n_rows, int32_t C, const int64_t *point_off, int32_t B,
                                const float *calib, const int32_t *image_shape, const double *boxes, int32_t n_boxes,
                                const int32_t *box_off, int32_t mode, float *points_out, int64_t *out_off,
                                int32_t *box_cnt, void *scratch, size_t scratch_bytes, uint32_t *status, void *stream) {
  DFU3D_CLEAR_STALE_ERROR();
  const bool emit = (mode & DFU3D_ING_EMIT) != 0, count = (mode & DFU3D_ING_COUNT) != 0;
  if (B < 1 || n_rows < 0 || C < 3 || n_boxes < 0) return DFU3D_EINVAL;
  if ((mode & ~(DFU3D_ING_EMIT | DFU3D_ING_COUNT)) || !(emit || count)) return DFU3D_EINVAL;
  if (!point_off || !calib || !image_shape || !status || !scratch || ((uintptr_t)scratch & 7u)) return DFU3D_EINVAL;
  if (((uintptr_t)point_off & 7u) || ((uintptr_t)calib & 3u) || ((uintptr_t)image_shape & 3u) || ((uintptr_t)status & 3u))
    return DFU3D_EINVAL;
  if (n_rows > 0 && (!points || ((uintptr_t)points & 3u))) return DFU3D_EINVAL;
  if (emit && (!out_off || ((uintptr_t)out_off & 7u))) return DFU3D_EINVAL;
  if (emit && n_rows > 0 && (!points_out || points_out == points || ((uintptr_t)points_out & 3u))) return DFU3D_EINVAL;
  if (count && (!box_off || ((uintptr_t)box_off & 3u))) return DFU3D_EINVAL;
  if (count && n_boxes > 0 && (!boxes || !box_cnt || ((uintptr_t)boxes & 7u) || ((uintptr_t)box_cnt & 3u)))
    return DFU3D_EINVAL;
  if (n_rows > DFU3D_ING_MAX_ROWS || B > DFU3D_ING_MAX_SCENES || C > DFU3D_ING_MAX_POINT_COLS ||
      n_boxes > DFU3D_ING_MAX_BOXES)
    return DFU3D_ERANGE;
  if (scratch_bytes < dfu3d_fov_ingest_scratch_bytes(n_rows)) return DFU3D_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  const int n_chunks = (int)ing_chunks(n_rows);
  const unsigned grid = (unsigned)(n_chunks > 0 ? n_chunks : 1);          // an empty batch: one workgroup with no row
  int *cnt = (int *)scratch, *off = cnt + grid;
  unsigned char *keep = (unsigned char *)(off + grid);
  const ViewCalib *cal = (const ViewCalib *)calib;
  const long long *poff = (const long long *)point_off;
  const bool vec4 = C == 4 && !((uintptr_t)points & 15u) && !((uintptr_t)points_out & 15u);
  hipLaunchKernelGGL(k_ing_flag, dim3(grid), dim3(PT), 0, st, points, (long long)n_rows, C, vec4, poff, B, cal,
                     image_shape, box_off, n_boxes, count, keep, cnt, status);
  DFU3D_LAUNCH_CHECK();
  if (emit) {
    hipLaunchKernelGGL(k_ing_scan, dim3(1), dim3(1024), 0, st, (int)grid, (const int *)cnt, off,
                       (const unsigned char *)keep, (long long)n_rows, poff, B, (long long *)out_off);
    DFU3D_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_ing_write, dim3(grid), dim3(PT), 0, st, points, (long long)n_rows, C, vec4,
                       (const unsigned char *)keep, (const int *)off, points_out);
    DFU3D_LAUNCH_CHECK();
  }
  if (count && n_boxes > 0) {
    hipLaunchKernelGGL(k_ing_boxes, dim3((unsigned)n_boxes), dim3(PT), 0, st, points, (long long)n_rows, C, poff, B,
                       (const unsigned char *)keep, boxes, box_off, box_cnt);
    DFU3D_LAUNCH_CHECK();
  }
  return DFU3D_OK;
}
