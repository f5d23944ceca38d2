// worldaug_stage.hip -- SURVEY.md §8 row f-10: everything OpenPCDet does to a scene between the ground-truth sampler and
// the model's batch_dict, for a whole batch (include/dfu3d_aug.h).
//
// What it stands in for in the reference: data_augmentor.py:56-156 (random_world_flip / _rotation / _scaling /
// _translation over augmentor_utils.py:8-92), the heading wrap of DataAugmentor.forward (:304), the class filter and
// the class column of dataset.py:194-200, mask_points_and_boxes_outside_range (data_processor.py:79-93,
// common_utils.mask_points_by_range, box_utils.mask_boxes_outside_range_numpy with the centre test) and
// dataset.py collate_batch (:237-250).  The host has drawn every scene's values already (one dfu3d_aug_params each).
//
//   k_wa_boxes  one workgroup per scene: the scene's boxes in their own type (float32 or float64; the rotation of the
//               centre and of the velocity and the heading wrap in float32, where the reference goes through torch),
//               class filter, centre test, ordered compaction into the scene's padded float32 block, zeros behind.
//               It also zeroes the scene's point counter and checks the scene's offsets.
//   k_wa_count  the flat point array in chunks of DFU3D_AUG_CHUNK rows (4 consecutive rows per thread): transform,
//               range test, the chunk's number of kept rows.  A chunk that straddles scenes finds each row's scene
//               in point_off.
//   k_wa_scan   one exclusive scan over the chunk counts; n_kept.
//   k_wa_write  the same transform and test again (the same function on the same inputs: the same decisions), a block
//               scan, the kept rows to their place with the scene's index in column 0; the scene's point counter
//               (integer atomics); the rows of the chunk's own index range at or beyond n_kept get (-1, 0, ...).
// The flat array is in scene order, so the one stable compaction is collate_batch's concatenation.
#include "common.hpp"
#include "dfu3d_aug.h"

namespace {

constexpr int PT = 256;                             // threads per workgroup
constexpr int PE = 4;                               // consecutive rows per thread
static_assert(PT * PE == DFU3D_AUG_CHUNK, "chunk");

// The rotation chain this stage defines: what torch's float32 matmul gives from 64 rows on.
// The matmul accumulates onto +0, so a zero result is +0 there whatever the signs of the terms: `+ 0.0f` does that
// (-0 + 0 = +0, every other value unchanged; the build has no fast-math, so the addition stays).
__device__ __forceinline__ void rot_z(float c, float s, float &x, float &y, float &z) {
  const float nx = __fmaf_rn(y, -s, x * c) + 0.0f;
  const float ny = __fmaf_rn(y, c, x * s) + 0.0f;
  x = nx;
  y = ny;
  z = z + 0.0f;
}

__device__ __forceinline__ void xf_point(const dfu3d_aug_params &p, float &x, float &y, float &z) {
  const uint32_t f = p.flags;
  if (f & DFU3D_AUG_FLIP_X) y = -y;
  if (f & DFU3D_AUG_FLIP_Y) x = -x;
  if (f & DFU3D_AUG_ROTATE) rot_z(p.cos_a, p.sin_a, x, y, z);
  if (f & DFU3D_AUG_SCALE) { x *= p.scale_f; y *= p.scale_f; z *= p.scale_f; }
  if (f & DFU3D_AUG_TRANSLATE) { x += p.tx; y += p.ty; z += p.tz; }
}

__device__ __forceinline__ bool in_range_xy(const float *__restrict__ range, float x, float y) {
  return x >= range[0] && x <= range[3] && y >= range[1] && y <= range[4];
}

template <class T> struct BoxK;
template <> struct BoxK<float> {
  static __device__ __forceinline__ float pi() { return 3.14159274101257324f; }
  static __device__ __forceinline__ float rot(const dfu3d_aug_params &p) { return p.noise_rot_f; }
  static __device__ __forceinline__ float scale(const dfu3d_aug_params &p) { return p.scale_f; }
};
template <> struct BoxK<double> {
  static __device__ __forceinline__ double pi() { return 3.141592653589793; }
  static __device__ __forceinline__ double rot(const dfu3d_aug_params &p) { return p.noise_rot; }
  static __device__ __forceinline__ double scale(const dfu3d_aug_params &p) { return p.scale; }
};

// named members, never an indexed array: an index the compiler cannot resolve would put the box into scratch memory
template <class T>
struct Box9 { T x, y, z, dx, dy, dz, h, vx, vy; };

// value selects, not conditional stores: the compiler merges `v.y = -v.y` and `v.x = -v.x` under different conditions
// into one store through a selected address, and the record lands in scratch
template <class T>
__device__ __forceinline__ T flip_h_x(bool on, T h) { return on ? -h : h; }
template <class T>
__device__ __forceinline__ T flip_h_y(bool on, T h) { return on ? -(h + BoxK<T>::pi()) : h; }

// vx, vy are zero for boxes of 7 columns and never stored then
template <class T>
__device__ __forceinline__ void xf_box(const dfu3d_aug_params &p, Box9<T> &v) {
  const uint32_t f = p.flags;
  const bool fx = (f & DFU3D_AUG_FLIP_X) != 0, fy = (f & DFU3D_AUG_FLIP_Y) != 0;
  v.y = fx ? -v.y : v.y;
  v.vy = fx ? -v.vy : v.vy;
  v.x = fy ? -v.x : v.x;
  v.vx = fy ? -v.vx : v.vx;
  const T h_xy = flip_h_y<T>(fy, flip_h_x<T>(fx, v.h)), h_yx = flip_h_x<T>(fx, flip_h_y<T>(fy, v.h));
  v.h = (f & DFU3D_AUG_FLIP_Y_FIRST) ? h_yx : h_xy;
  if (f & DFU3D_AUG_ROTATE) {
    float x = (float)v.x, y = (float)v.y, z = (float)v.z;
    rot_z(p.cos_a, p.sin_a, x, y, z);
    v.x = (T)x; v.y = (T)y; v.z = (T)z;
    v.h += BoxK<T>::rot(p);
    float vx = (float)v.vx, vy = (float)v.vy, vz = 0.0f;
    rot_z(p.cos_a, p.sin_a, vx, vy, vz);
    v.vx = (T)vx; v.vy = (T)vy;
  }
  if (f & DFU3D_AUG_SCALE) {
    const T s = BoxK<T>::scale(p);
    v.x *= s; v.y *= s; v.z *= s; v.dx *= s; v.dy *= s; v.dz *= s; v.vx *= s; v.vy *= s;
  }
  if (f & DFU3D_AUG_TRANSLATE) { v.x += (T)p.tx; v.y += (T)p.ty; v.z += (T)p.tz; }
  if (f & DFU3D_AUG_WRAP) {
    const float two_pi = 6.28318548202514648f;
    const float h = (float)v.h;
    v.h = (T)(h - floorf(h / two_pi + 0.5f) * two_pi);
  }
}

template <class T>
__global__ __launch_bounds__(PT) void k_wa_boxes(const T *__restrict__ boxes, int nc, long long n_box_rows,
                                                 const int *__restrict__ box_off, const int *__restrict__ box_cnt,
                                                 const int *__restrict__ box_cls,
                                                 const dfu3d_aug_params *__restrict__ params,
                                                 const float *__restrict__ range, int mode, float *__restrict__ out,
                                                 int box_cap, int *__restrict__ gt_cnt, T *__restrict__ aug,
                                                 int *__restrict__ keep_out, const long long *__restrict__ point_off,
                                                 long long n_rows, int B, int *__restrict__ point_cnt,
                                                 uint32_t *__restrict__ status) {
  __shared__ int s_w[PT / 64];
  const int b = blockIdx.x, t = threadIdx.x;
  const long long r0 = box_off[b];
  int n = box_cnt[b];
  if (t == 0) {
    point_cnt[b] = 0;
    const long long p0 = point_off[b], p1 = point_off[b + 1];
    if (!offsets_ok(p0, p1, n_rows, b)) atomicOr(status, (uint32_t)DFU3D_AUG_ST_OFFSETS);
  }
  if (r0 < 0 || n < 0 || r0 + n > n_box_rows || (long long)n > (long long)box_off[b + 1] - r0) {
    if (t == 0) atomicOr(status, (uint32_t)DFU3D_AUG_ST_OFFSETS);
    n = 0;                                           // nothing outside the arrays is ever read
  }
  const dfu3d_aug_params &p = params[b];
  const int W = nc + 1;
  float *ob = out + (size_t)b * box_cap * W;
  const bool vel = nc > 7;
  int kept = 0;
  for (int i0 = 0; i0 < n; i0 += PT) {
    const int i = i0 + t;
    bool keep = false;
    Box9<T> v = {};
    int cls = 0;
    if (i < n) {
      const T *src = boxes + (size_t)(r0 + i) * nc;
      v.x = src[0]; v.y = src[1]; v.z = src[2]; v.dx = src[3]; v.dy = src[4]; v.dz = src[5]; v.h = src[6];
      if (vel) { v.vx = src[7]; v.vy = src[8]; }
      cls = box_cls[r0 + i];
      xf_box<T>(p, v);
      keep = !(mode & DFU3D_AUG_FILTER_CLASS) || cls > 0;
      if (mode & DFU3D_AUG_MASK_BOXES)
        keep = keep && v.x >= (T)range[0] && v.x <= (T)range[3] && v.y >= (T)range[1] && v.y <= (T)range[4] &&
               v.z >= (T)range[2] && v.z <= (T)range[5];
      if (aug) {
        T *dst = aug + (size_t)(r0 + i) * nc;
        dst[0] = v.x; dst[1] = v.y; dst[2] = v.z; dst[3] = v.dx; dst[4] = v.dy; dst[5] = v.dz; dst[6] = v.h;
        if (vel) { dst[7] = v.vx; dst[8] = v.vy; }
      }
      if (keep_out) keep_out[r0 + i] = keep ? 1 : 0;
    }
    int tot;
    const int r = block_rank<PT / 64>(keep, s_w, tot);
    if (keep && kept + r < box_cap) {
      float *dst = ob + (size_t)(kept + r) * W;
      dst[0] = (float)v.x; dst[1] = (float)v.y; dst[2] = (float)v.z; dst[3] = (float)v.dx; dst[4] = (float)v.dy;
      dst[5] = (float)v.dz; dst[6] = (float)v.h;
      if (vel) { dst[7] = (float)v.vx; dst[8] = (float)v.vy; }
      dst[nc] = (float)cls;
    }
    kept += tot;
  }
  if (kept > box_cap) {
    if (t == 0) atomicOr(status, (uint32_t)DFU3D_AUG_ST_BOX_CAP);
    kept = box_cap;
  }
  for (int idx = kept * W + t; idx < box_cap * W; idx += PT) ob[idx] = 0.0f;
  if (t == 0) gt_cnt[b] = kept;
}

// The rows of chunk `chunk` this thread owns: transform and test.  x, y, z: the transformed coordinates; sc: the scene.
struct RowSet {
  float x[PE], y[PE], z[PE];
  int sc[PE];
  bool keep[PE];
  int n;
};

template <bool WITH_Z>
__device__ __forceinline__ int rows_of(const float *__restrict__ pts, long long n_rows, int C,
                                       const long long *__restrict__ point_off, int B,
                                       const dfu3d_aug_params *__restrict__ params, const float *__restrict__ range,
                                       int mode, long long chunk, RowSet &R, bool &nonfinite, int &s_lo, int &s_hi) {
  // the array may be longer than the scenes it holds (a capacity): rows at or beyond point_off[B] are never read
  const long long n_valid = valid_rows(point_off, B, n_rows);
  const long long c0 = chunk * DFU3D_AUG_CHUNK;
  const long long c1 = (c0 + DFU3D_AUG_CHUNK < n_valid ? c0 + DFU3D_AUG_CHUNK : n_valid) - 1;
  scenes_of_chunk(point_off, B, c0, c1, s_lo, s_hi);   // uniform over the workgroup
  const long long i0 = c0 + (long long)threadIdx.x * PE;
  int mine = 0;
  nonfinite = false;
#pragma unroll
  for (int k = 0; k < PE; k++) {
    R.keep[k] = false;
    R.sc[k] = s_lo;
    R.x[k] = R.y[k] = R.z[k] = 0.0f;
    if (i0 + k < n_valid) {
      const int s = (s_lo == s_hi) ? s_lo : last_at_or_below(point_off, s_lo, s_hi + 1, i0 + k);
      const float *q = pts + (size_t)(i0 + k) * C;
      float x = q[0], y = q[1], z = WITH_Z ? q[2] : 0.0f;
      xf_point(params[s], x, y, z);
      bool keep = true;
      if (mode & DFU3D_AUG_MASK_POINTS) {
        keep = in_range_xy(range, x, y);
        if (!(isfinite(x) && isfinite(y))) nonfinite = true;
      }
      R.x[k] = x; R.y[k] = y; R.z[k] = z; R.sc[k] = s; R.keep[k] = keep;
      mine += keep ? 1 : 0;
    }
  }
  return mine;
}

__global__ __launch_bounds__(PT) void k_wa_count(const float *__restrict__ pts, long long n_rows, int C,
                                                 const long long *__restrict__ point_off, int B,
                                                 const dfu3d_aug_params *__restrict__ params,
                                                 const float *__restrict__ range, int mode, int *__restrict__ cnt,
                                                 uint32_t *__restrict__ status) {
  __shared__ int s_w[PT / 64];
  RowSet R;
  bool nonfinite;
  int s_lo, s_hi;
  int mine = rows_of<false>(pts, n_rows, C, point_off, B, params, range, mode, blockIdx.x, R, nonfinite, s_lo, s_hi);
  if (nonfinite) atomicOr(status, (uint32_t)DFU3D_AUG_ST_NONFINITE);
  mine = block_sum_i<PT / 64>(mine, s_w);
  if (threadIdx.x == 0) cnt[blockIdx.x] = mine;
}

__global__ __launch_bounds__(1024) void k_wa_scan(int n_chunks, const int *__restrict__ cnt, int *__restrict__ off,
                                                  int *__restrict__ n_kept) {
  __shared__ int s_w[16];
  const int total = block_scan_range<1024, 1, int, int>(
      n_chunks, [&](int c) { return cnt[c]; }, [&](int c, int ex) { off[c] = ex; }, s_w);
  if (threadIdx.x == 0) n_kept[0] = total;
}

__global__ __launch_bounds__(PT) void k_wa_write(const float *__restrict__ pts, long long n_rows, int C,
                                                 const long long *__restrict__ point_off, int B,
                                                 const dfu3d_aug_params *__restrict__ params,
                                                 const float *__restrict__ range, int mode,
                                                 const int *__restrict__ off, const int *__restrict__ n_kept,
                                                 float *__restrict__ out, int *__restrict__ point_cnt) {
  __shared__ int s_w[PT / 64];
  RowSet R;
  bool nonfinite;
  int s_lo, s_hi;
  const int mine = rows_of<true>(pts, n_rows, C, point_off, B, params, range, mode, blockIdx.x, R, nonfinite, s_lo, s_hi);
  int tot;
  int r = block_excl_scan<PT / 64>(mine, s_w, tot);
  const long long o = off[blockIdx.x];
  const long long total = n_kept[0];
  const int W = C + 1;
  const long long i0 = (long long)blockIdx.x * DFU3D_AUG_CHUNK + (long long)threadIdx.x * PE;
#pragma unroll
  for (int k = 0; k < PE; k++) {
    if (R.keep[k]) {
      const long long d = o + r;
      if (d < total && d < n_rows) {                 // holds by construction; never a store outside the array
        const float *q = pts + (size_t)(i0 + k) * C;
        float *dst = out + (size_t)d * W;
        dst[0] = (float)R.sc[k];
        dst[1] = R.x[k]; dst[2] = R.y[k]; dst[3] = R.z[k];
        for (int c = 3; c < C; c++) dst[c + 1] = q[c];
      }
      if (s_lo != s_hi) atomicAdd(&point_cnt[R.sc[k]], 1);
      r++;
    }
  }
  if (s_lo == s_hi && threadIdx.x == 0 && tot > 0) atomicAdd(&point_cnt[s_lo], tot);
  // the padded tail: the rows of this chunk's own index range that no kept row lands on
#pragma unroll
  for (int k = 0; k < PE; k++) {
    const long long i = i0 + k;
    if (i < n_rows && i >= total) {
      float *dst = out + (size_t)i * W;
      dst[0] = -1.0f;
      for (int c = 1; c < W; c++) dst[c] = 0.0f;
    }
  }
}

template <class T>
int launch_boxes(const void *boxes, int32_t box_cols, int64_t n_box_rows, const int32_t *box_off, const int32_t *box_cnt,
                 const int32_t *box_cls, const dfu3d_aug_params *params, const float *range, int32_t mode,
                 float *gt_boxes_out, int32_t box_cap, int32_t *gt_cnt, void *boxes_aug, int32_t *box_keep,
                 const int64_t *point_off, int64_t n_rows, int32_t B, int32_t *point_cnt, uint32_t *status,
                 hipStream_t st) {
  hipLaunchKernelGGL(k_wa_boxes<T>, dim3((unsigned)B), dim3(PT), 0, st, (const T *)boxes, box_cols,
                     (long long)n_box_rows, box_off, box_cnt, box_cls, params, range, mode, gt_boxes_out, box_cap, gt_cnt,
                     (T *)boxes_aug, box_keep, (const long long *)point_off, (long long)n_rows, B, point_cnt, status);
  DFU3D_LAUNCH_CHECK();
  return DFU3D_OK;
}

int64_t wa_chunks(int64_t n_rows) { return (n_rows + DFU3D_AUG_CHUNK - 1) / DFU3D_AUG_CHUNK; }

}  // namespace

extern "C" int32_t dfu3d_aug_version(void) { return DFU3D_AUG_VERSION; }

extern "C" size_t dfu3d_world_aug_scratch_bytes(int64_t n_rows) {
  if (n_rows < 0 || n_rows > DFU3D_AUG_MAX_ROWS) return 0;
  return (size_t)wa_chunks(n_rows) * 2 * sizeof(int) + 16;
}

extern "C" int dfu3d_world_aug_collate(const float *points, int64_t n_rows, int32_t C, const int64_t *point_off,
                                       int32_t B, const void *boxes, int32_t box_f64, int32_t box_cols,
                                       int64_t n_box_rows, const int32_t *box_off, const int32_t *box_cnt,
                                       const int32_t *box_cls, const dfu3d_aug_params *params, const float *range,
                                       int32_t mode, float *points_out, int32_t *n_kept, int32_t *point_cnt,
                                       float *gt_boxes_out, int32_t box_cap, int32_t *gt_cnt, void *boxes_aug,
                                       int32_t *box_keep, void *scratch, size_t scratch_bytes, uint32_t *status,
                                       void *stream) {
  DFU3D_CLEAR_STALE_ERROR();
  if (B < 0 || n_rows < 0 || n_box_rows < 0 || C < 3 || box_cap < 0) return DFU3D_EINVAL;
  if (box_cols != 7 && box_cols != 9) return DFU3D_EINVAL;
  if (mode & ~(DFU3D_AUG_MASK_POINTS | DFU3D_AUG_MASK_BOXES | DFU3D_AUG_FILTER_CLASS)) return DFU3D_EINVAL;
  if (!n_kept || !status || !scratch || ((uintptr_t)scratch & 7u)) return DFU3D_EINVAL;
  if (B == 0 && (n_rows != 0 || n_box_rows != 0)) return DFU3D_EINVAL;
  if (B > 0 && (!point_off || !box_off || !box_cnt || !params || !range || !point_cnt || !gt_cnt)) return DFU3D_EINVAL;
  if (n_rows > 0 && (!points || !points_out || points == points_out)) return DFU3D_EINVAL;
  if (n_box_rows > 0 && (!boxes || !box_cls || boxes == boxes_aug)) return DFU3D_EINVAL;
  if (B > 0 && box_cap > 0 && !gt_boxes_out) return DFU3D_EINVAL;
  if (n_rows > DFU3D_AUG_MAX_ROWS || B > DFU3D_AUG_MAX_SCENES || C > DFU3D_AUG_MAX_POINT_COLS ||
      box_cap > DFU3D_AUG_MAX_BOX_CAP || n_box_rows > 0x7FFFFFFF)
    return DFU3D_ERANGE;
  if (scratch_bytes < dfu3d_world_aug_scratch_bytes(n_rows)) return DFU3D_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  const int n_chunks = (int)wa_chunks(n_rows);
  int *cnt = (int *)scratch, *off = cnt + n_chunks;
  if (B > 0) {
    const int rc = box_f64 ? launch_boxes<double>(boxes, box_cols, n_box_rows, box_off, box_cnt, box_cls, params, range,
                                                  mode, gt_boxes_out, box_cap, gt_cnt, boxes_aug, box_keep, point_off,
                                                  n_rows, B, point_cnt, status, st)
                           : launch_boxes<float>(boxes, box_cols, n_box_rows, box_off, box_cnt, box_cls, params, range,
                                                 mode, gt_boxes_out, box_cap, gt_cnt, boxes_aug, box_keep, point_off,
                                                 n_rows, B, point_cnt, status, st);
    if (rc != DFU3D_OK) return rc;
  }
  if (n_chunks > 0) {
    hipLaunchKernelGGL(k_wa_count, dim3((unsigned)n_chunks), dim3(PT), 0, st, points, (long long)n_rows, C,
                       (const long long *)point_off, B, params, range, mode, cnt, status);
    DFU3D_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(k_wa_scan, dim3(1), dim3(1024), 0, st, n_chunks, (const int *)cnt, off, n_kept);
  DFU3D_LAUNCH_CHECK();
  if (n_chunks > 0) {
    hipLaunchKernelGGL(k_wa_write, dim3((unsigned)n_chunks), dim3(PT), 0, st, points, (long long)n_rows, C,
                       (const long long *)point_off, B, params, range, mode, (const int *)off, (const int *)n_kept,
                       points_out, point_cnt);
    DFU3D_LAUNCH_CHECK();
  }
  return DFU3D_OK;
}
