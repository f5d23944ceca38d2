// rcnntarget_stage.hip -- SURVEY.md §8 row f-16: the two target-assignment steps of PointRCNN's training, each for the
// whole batch in one launch and without a read from the device (include/dfu3d_tgt.h).
//
// What they stand in for in the reference: PointHeadTemplate.assign_stack_targets -- per sample a boolean mask over all
// points, two points_in_boxes_gpu calls, three boolean-indexed scatters and an encode on a host-sized subset -- and
// ProposalTargetLayer.sample_rois_for_rcnn -- per sample a host read per trimmed box, per class an IoU launch between
// .item() / .sum() > 0 / nonzero, then nonzero, np.random.permutation and torch.randint on the host.
//
//   k_tg_point_targets  one thread per point.  The sample's boxes pass through LDS in tiles of 64, each staged once per
//                       workgroup as the constants of both in-box tests (the trig of a box is evaluated once per
//                       workgroup, not once per point); a thread walks a tile until it has its first ground-truth hit, a
//                       wave skips the tiles left once all its points have one.  The encode reads the hit row again.
//   k_tg_roi_max_iou    one wave per RoI, lanes over the ground-truth rows, a butterfly on (IoU, lowest row) at the end:
//                       B * M waves instead of B * M threads (4 096 threads would fill 64 waves of the 1 024 SIMDs).  With
//                       by_class a lane whose row has another class idles through the overlap; rows are few (tens).
//   k_tg_roi_sample     one workgroup per sample: three ordered lists by the workgroup scan, the foreground prefix of a
//                       random permutation as a rank by counting over (rand_key, index) in LDS, the draws with
//                       replacement straight from rand_u.
#include "common.hpp"
#include "dfu3d_tgt.h"
#include "pt_in_box.hpp"
#include "rect_overlap.hpp"

#include <math.h>

namespace {

constexpr int PT = 256;                              // threads per workgroup of k_tg_point_targets
constexpr int TILE = 64;                             // boxes of one LDS tile
constexpr int ST = 256;                              // threads of k_tg_roi_sample's workgroup
constexpr float MARGIN = 1e-5f;                      // check_pt_in_box3d of the reference's point-in-box ops
constexpr float MIN_DIM = 1e-5f;                     // the coder's clamp of the dims

__global__ __launch_bounds__(PT) void k_tg_point_targets(const float *__restrict__ pts, int stride,
                                                         const float *__restrict__ gt, const float *__restrict__ mean,
                                                         int N, int G, int K, int num_class, float ex, float ey, float ez,
                                                         long long *__restrict__ cls, float *__restrict__ box,
                                                         int *__restrict__ gidx) {
  __shared__ float s_f[TILE][5];                     // cx, cy, cz, cosa, sina
  __shared__ double s_d[TILE][6];                    // hz, hx, hy of the box, then of the enlarged box
  const int b = blockIdx.y, n = blockIdx.x * PT + threadIdx.x;
  const bool live = n < N;
  const size_t row = (size_t)b * N + (live ? n : N - 1);
  const float *boxes = gt + (size_t)b * G * 8;
  const float x = pts[row * stride], y = pts[row * stride + 1], z = pts[row * stride + 2];
  int k = -1, e = -1;
  for (int g0 = 0; g0 < G; g0 += TILE) {
    const int cnt = min(TILE, G - g0);
    if (threadIdx.x < cnt) {
      const float *r = boxes + (size_t)(g0 + threadIdx.x) * 8;
      const BoxF q = load_box_f32(r, MARGIN, 0.0f, 0.0f, 0.0f), w = load_box_f32(r, MARGIN, ex, ey, ez);
      float *f = s_f[threadIdx.x];
      double *d = s_d[threadIdx.x];
      f[0] = q.cx; f[1] = q.cy; f[2] = q.cz; f[3] = q.cosa; f[4] = q.sina;
      d[0] = q.hz; d[1] = q.hx; d[2] = q.hy; d[3] = w.hz; d[4] = w.hx; d[5] = w.hy;
    }
    __syncthreads();
    if (!__all(k >= 0)) {                            // (per wave)
      for (int t = 0; t < cnt && k < 0; t++) {
        BoxF q;
        q.cx = s_f[t][0]; q.cy = s_f[t][1]; q.cz = s_f[t][2]; q.cosa = s_f[t][3]; q.sina = s_f[t][4];
        q.hz = s_d[t][0]; q.hx = s_d[t][1]; q.hy = s_d[t][2];
        if (pt_in_box(q, x, y, z)) k = g0 + t;
        if (e < 0) {
          q.hz = s_d[t][3]; q.hx = s_d[t][4]; q.hy = s_d[t][5];
          if (pt_in_box(q, x, y, z)) e = g0 + t;
        }
      }
    }
    __syncthreads();
  }
  if (!live) return;
  float code[8] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
  long long label = (k < 0 && e >= 0) ? -1 : 0;
  if (k >= 0) {
    const float *r = boxes + (size_t)k * 8;
    const float c = r[7];
    if (c >= 1.0f && c < 2147483648.0f && (K == 0 || c <= (float)K)) {
      const int ci = (int)c;
      label = num_class == 1 ? 1 : (long long)ci;
      float d0 = r[3], d1 = r[4], d2 = r[5];
      d0 = d0 < MIN_DIM ? MIN_DIM : d0;              // (a NaN stays one, as clamp_min leaves it)
      d1 = d1 < MIN_DIM ? MIN_DIM : d1;
      d2 = d2 < MIN_DIM ? MIN_DIM : d2;
      if (K > 0) {
        const float s0 = mean[(size_t)(ci - 1) * 3], s1 = mean[(size_t)(ci - 1) * 3 + 1], s2 = mean[(size_t)(ci - 1) * 3 + 2];
        const float diag = sqrtf(s0 * s0 + s1 * s1);
        code[0] = (r[0] - x) / diag;
        code[1] = (r[1] - y) / diag;
        code[2] = (r[2] - z) / s2;
        code[3] = (float)log((double)(d0 / s0));
        code[4] = (float)log((double)(d1 / s1));
        code[5] = (float)log((double)(d2 / s2));
      } else {
        code[0] = r[0] - x;
        code[1] = r[1] - y;
        code[2] = r[2] - z;
        code[3] = (float)log((double)d0);
        code[4] = (float)log((double)d1);
        code[5] = (float)log((double)d2);
      }
      code[6] = (float)cos((double)r[6]);
      code[7] = (float)sin((double)r[6]);
    }
  }
  cls[row] = label;
  float4 *o = reinterpret_cast<float4 *>(box + row * 8);      // rows of 32 bytes; the base is checked on the host
  o[0] = make_float4(code[0], code[1], code[2], code[3]);
  o[1] = make_float4(code[4], code[5], code[6], code[7]);
  if (gidx) gidx[row] = k;
}

// torch.minimum / torch.maximum / clamp(min=): a NaN is handed on, a zero keeps its sign
__device__ __forceinline__ float min_nan(float a, float b) { return (a != a || b != b) ? a + b : (b < a ? b : a); }
__device__ __forceinline__ float max_nan(float a, float b) { return (a != a || b != b) ? a + b : (b > a ? b : a); }
__device__ __forceinline__ float at_least(float v, float lo) { return v < lo ? lo : v; }

__global__ __launch_bounds__(IB) void k_tg_roi_max_iou(const float *__restrict__ rois, const long long *__restrict__ labels,
                                                       const float *__restrict__ gt, int M, int G, int by_class,
                                                       float *__restrict__ ov, int *__restrict__ asg) {
  __shared__ float s_poly[4][MAXV * IB];
  const int lane = lane_id(), b = blockIdx.y, m = blockIdx.x * (IB / 64) + (threadIdx.x >> 6);
  if (m >= M) return;                                // a whole wave; the kernel has no barrier
  const size_t bm = (size_t)b * M + m;
  const float *boxes = gt + (size_t)b * G * 8;
  int last = -1;                                     // the reference's trim of trailing zero rows, in both modes
  for (int g = lane; g < G; g += 64) {
    const float *r = boxes + (size_t)g * 8;
    float s = r[0];
#pragma unroll
    for (int c = 1; c < 8; c++) s += r[c];
    if (s != 0.0f) last = g;
  }
  last = -wave_min_i_dpp(-last);
  const float *a = rois + bm * 7;
  const long long want = labels[bm];
  const Rect A = make_rect(a, 7);
  const float a_half = 0.5f * a[5], a_lo = a[2] - a_half, a_hi = a[2] + a_half, va = a[3] * a[4] * a[5];
  float best = 0.0f;
  int best_g = -1;
  for (int g = lane; g <= last; g += 64) {
    const float *r = boxes + (size_t)g * 8;
    if (by_class) {
      const float c = r[7];
      if (!(fabsf(c) < 9.0e18f) || (long long)c != want) continue;
    }
    const Rect Bx = make_rect(r, 7);
    const float over = overlap_area(A, Bx, s_poly[0] + threadIdx.x, s_poly[1] + threadIdx.x, s_poly[2] + threadIdx.x,
                                    s_poly[3] + threadIdx.x);
    const float b_half = 0.5f * r[5], b_lo = r[2] - b_half, b_hi = r[2] + b_half, vb = r[3] * r[4] * r[5];
    const float common_z = at_least(min_nan(a_hi, b_hi) - max_nan(a_lo, b_lo), 0.0f);
    const float inter = over * common_z;
    const float iou = inter / at_least((va + vb) - inter, 1e-6f);
    if (iou == iou && (best_g < 0 || iou > best)) { best = iou; best_g = g; }     // ascending g: the lowest row stays
  }
#pragma unroll
  for (int s = 32; s >= 1; s >>= 1) {
    const float v = __shfl_xor(best, s, 64);
    const int g = __shfl_xor(best_g, s, 64);
    if (g >= 0 && (best_g < 0 || v > best || (v == best && g < best_g))) { best = v; best_g = g; }
  }
  if (lane == 0) {
    ov[bm] = best_g < 0 ? 0.0f : best;
    asg[bm] = best_g < 0 ? 0 : best_g;
  }
}

__device__ __forceinline__ int draw(const int *list, int n, float u) {
  const double v = floor((double)u * (double)n);
  return list[v >= 0.0 ? (v < (double)n ? (int)v : n - 1) : 0];      // (no number, negative: 0)
}

__global__ __launch_bounds__(ST) void k_tg_roi_sample(const float *__restrict__ ov, const int *__restrict__ key,
                                                      const float *__restrict__ rand_u, int M, int R, int fg_per,
                                                      float fg_t, float reg_t, float lo_t, double ratio,
                                                      int *__restrict__ out, uint32_t *status) {
  __shared__ int s_fg[DFU3D_TGT_MAX_ROIS], s_hard[DFU3D_TGT_MAX_ROIS], s_easy[DFU3D_TGT_MAX_ROIS], s_key[DFU3D_TGT_MAX_ROIS];
  __shared__ int s_w[ST / 64];
  const int b = blockIdx.x;
  const float *o = ov + (size_t)b * M;
  const float *u = rand_u + (size_t)b * R;
  int *so = out + (size_t)b * R;
  auto is_fg = [&](int i) { return o[i] >= fg_t; };
  auto is_hard = [&](int i) { const float v = o[i]; return v < reg_t && v >= lo_t; };
  auto is_easy = [&](int i) { return o[i] < lo_t; };
  const int nf = block_scan_range<ST, 4, int, int>(M, [&](int i) { return is_fg(i) ? 1 : 0; },
                                                   [&](int i, int p) { if (is_fg(i)) s_fg[p] = i; }, s_w);
  const int nh = block_scan_range<ST, 4, int, int>(M, [&](int i) { return is_hard(i) ? 1 : 0; },
                                                   [&](int i, int p) { if (is_hard(i)) s_hard[p] = i; }, s_w);
  const int ne = block_scan_range<ST, 4, int, int>(M, [&](int i) { return is_easy(i) ? 1 : 0; },
                                                   [&](int i, int p) { if (is_easy(i)) s_easy[p] = i; }, s_w);
  __syncthreads();                                   // the lists are whole
  const int nb = nh + ne;
  if (nf == 0 && nb == 0) {
    for (int j = threadIdx.x; j < R; j += ST) so[j] = 0;
    if (threadIdx.x == 0) atomicOr(status, (uint32_t)DFU3D_TGT_STATUS_NO_ROI);
    return;
  }
  if (nb == 0) {                                     // foreground only: R draws with replacement
    for (int j = threadIdx.x; j < R; j += ST) so[j] = draw(s_fg, nf, u[j]);
    return;
  }
  int take = 0;
  if (nf > 0) {                                      // the first `take` of a random permutation of fg
    take = min(fg_per, nf);
    for (int t = threadIdx.x; t < nf; t += ST) s_key[t] = key[(size_t)b * M + s_fg[t]];
    __syncthreads();
    for (int t = threadIdx.x; t < nf; t += ST) {
      const int mine = s_key[t];
      int rank = 0;
      for (int q = 0; q < nf; q++) {                 // (every thread reads the same word: a broadcast)
        const int other = s_key[q];
        rank += (other < mine || (other == mine && q < t)) ? 1 : 0;
      }
      if (rank < take) so[rank] = s_fg[t];
    }
  }
  const int need = R - take;
  const int h = (nh > 0 && ne > 0) ? min((int)((double)need * ratio), nh) : (nh > 0 ? need : 0);
  for (int j = take + threadIdx.x; j < R; j += ST)
    so[j] = (j - take < h) ? draw(s_hard, nh, u[j]) : draw(s_easy, ne, u[j]);
}

// DFU3D_OK, or DFU3D_ERANGE for a tensor of DFU3D_TGT_MAX_ELEMS elements or more
int range_of(double elems) { return elems >= (double)DFU3D_TGT_MAX_ELEMS ? DFU3D_ERANGE : DFU3D_OK; }

}  // namespace

extern "C" int32_t dfu3d_tgt_version(void) { return DFU3D_TGT_VERSION; }

extern "C" int dfu3d_tgt_point_targets(const float *points, int32_t pts_stride, const float *gt_boxes,
                                       const float *mean_size, int32_t B, int32_t N, int32_t G, int32_t K,
                                       int32_t num_class, float extra_x, float extra_y, float extra_z,
                                       int64_t *cls_labels, float *box_labels, int32_t *gt_idx, void *stream) {
  DFU3D_CLEAR_STALE_ERROR();
  if (!points || !gt_boxes || !cls_labels || !box_labels) return DFU3D_EINVAL;
  if (B < 1 || N < 1 || G < 1 || K < 0 || num_class < 1 || pts_stride < 3 || pts_stride > 64) return DFU3D_EINVAL;
  if ((K > 0) != (mean_size != nullptr)) return DFU3D_EINVAL;
  if (reinterpret_cast<uintptr_t>(box_labels) & 15) return DFU3D_EINVAL;           // the rows are stored as two float4
  if (extra_x != extra_x || extra_y != extra_y || extra_z != extra_z) return DFU3D_EINVAL;
  int rc = range_of((double)B * N * (double)(pts_stride > 8 ? pts_stride : 8));
  if (rc == DFU3D_OK) rc = range_of((double)B * G * 8.0);
  if (rc != DFU3D_OK) return rc;
  if (B > DFU3D_TGT_MAX_BATCH || K > DFU3D_TGT_MAX_CLASSES) return DFU3D_ERANGE;
  hipLaunchKernelGGL(k_tg_point_targets, dim3((unsigned)((N + PT - 1) / PT), (unsigned)B), dim3(PT), 0,
                     (hipStream_t)stream, points, pts_stride, gt_boxes, mean_size, N, G, K, num_class, extra_x, extra_y,
                     extra_z, (long long *)cls_labels, box_labels, gt_idx);
  DFU3D_LAUNCH_CHECK();
  return DFU3D_OK;
}
static_assert(DFU3D_TGT_POINT_LAUNCHES == 1 && DFU3D_TGT_IOU_LAUNCHES == 1 && DFU3D_TGT_SAMPLE_LAUNCHES == 1, "one each");

extern "C" int dfu3d_tgt_roi_max_iou(const float *rois, const int64_t *roi_labels, const float *gt_boxes, int32_t B,
                                     int32_t M, int32_t G, int32_t by_class, float *max_overlaps, int32_t *gt_assignment,
                                     void *stream) {
  DFU3D_CLEAR_STALE_ERROR();
  if (!rois || !roi_labels || !gt_boxes || !max_overlaps || !gt_assignment) return DFU3D_EINVAL;
  if (B < 1 || M < 1 || G < 1 || (by_class != 0 && by_class != 1)) return DFU3D_EINVAL;
  int rc = range_of((double)B * M * 7.0);
  if (rc == DFU3D_OK) rc = range_of((double)B * G * 8.0);
  if (rc != DFU3D_OK) return rc;
  if (B > DFU3D_TGT_MAX_BATCH) return DFU3D_ERANGE;
  hipLaunchKernelGGL(k_tg_roi_max_iou, dim3((unsigned)((M + IB / 64 - 1) / (IB / 64)), (unsigned)B), dim3(IB), 0,
                     (hipStream_t)stream, rois, (const long long *)roi_labels, gt_boxes, M, G, by_class, max_overlaps,
                     gt_assignment);
  DFU3D_LAUNCH_CHECK();
  return DFU3D_OK;
}

extern "C" int dfu3d_tgt_roi_sample(const float *max_overlaps, const int32_t *rand_key, const float *rand_u, int32_t B,
                                    int32_t M, int32_t R, int32_t fg_per, float fg_thresh, float reg_fg_thresh,
                                    float bg_thresh_lo, double hard_ratio, int32_t *sampled_inds, uint32_t *status,
                                    void *stream) {
  DFU3D_CLEAR_STALE_ERROR();
  if (!max_overlaps || !rand_key || !rand_u || !sampled_inds || !status) return DFU3D_EINVAL;
  if (B < 1 || M < 1 || R < 1 || fg_per < 0 || fg_per > R) return DFU3D_EINVAL;
  if (!(hard_ratio >= 0.0 && hard_ratio <= 1.0)) return DFU3D_EINVAL;
  if (M > DFU3D_TGT_MAX_ROIS || R > DFU3D_TGT_MAX_SAMPLED || B > DFU3D_TGT_MAX_BATCH) return DFU3D_ERANGE;
  hipLaunchKernelGGL(k_tg_roi_sample, dim3((unsigned)B), dim3(ST), 0, (hipStream_t)stream, max_overlaps, rand_key, rand_u,
                     M, R, fg_per, fg_thresh, reg_fg_thresh, bg_thresh_lo, hard_ratio, sampled_inds, status);
  DFU3D_LAUNCH_CHECK();
  return DFU3D_OK;
}
