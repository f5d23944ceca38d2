// roipoint_stage.hip -- SURVEY.md §8 row f-15: RoI-point pooling, the native op of PointRCNN's second stage
// (include/dfu3d_roi.h).
//
// What it stands in for in the reference: pcdet/ops/roipoint_pool3d (CUDA only) -- a (B, N, M) int assignment matrix
// filled by one thread per (point, box), one thread per box walking it over all N points, a gather -- and, in the fused
// form, the concatenation and the five torch ops PointRCNNHead.roipool3d_gpu puts around it.
//
//   k_rp_search       one wave per (sample, RoI), k_pn_ball's walk with longer trips: 1024 points per trip (the loads of
//                     sixteen 64-point tiles in flight: at the configuration's shapes there is one wave per SIMD and
//                     nothing else hides a trip's latency), per tile a ballot and a prefix count keep the ascending
//                     order; the walk ends after the trip in which S points are found.  Writes the first min(cnt, S) slots of pooled_idx and the empty flag; the
//                     slots k >= cnt take -cnt (cnt >= 1) or 0 (cnt = 0) -- the wave never reads back what its other
//                     lanes stored, the wrap k % cnt is resolved after the kernel boundary.
//   k_rp_gather<F>    four waves per (RoI, 64 slots), a wave per pooled row: the slot's index (a slot holding -cnt reads
//                     slot k % cnt, which the search wrote, and stores it), the point, the prefix columns -- F = 0:
//                     x, y, z; F = 1: the canonical x', y', z', the score and the depth -- then the feature row: as float4
//                     where C is a multiple of 4 and the rows start on 16 bytes (a lane loads four floats and stores
//                     four dwords: the pooled row itself never starts on 16 bytes), else lanes run over the row's
//                     columns, consecutive dwords on both sides.  The rows of an empty RoI are stored as +0.0f.
#include "common.hpp"
#include "dfu3d_roi.h"
#include "pt_in_box.hpp"

#include <math.h>

namespace {

constexpr int BT = 256;                              // threads per workgroup of both kernels
constexpr int ROWS_WG = 64, ROWS_WAVE = ROWS_WG / (BT / 64);   // pooled rows of a gather workgroup, of one of its waves
constexpr int TILES = 16, TRIP = TILES * 64;         // 64-point tiles, points of one trip of the search
constexpr float MARGIN = 1e-5f;                      // check_pt_in_box3d of roipoint_pool3d_kernel.cu

__global__ __launch_bounds__(BT) void k_rp_search(const float *__restrict__ pts, int stride, const float *__restrict__ boxes,
                                                  int N, int M, int S, float ex, float ey, float ez, int *__restrict__ idx,
                                                  int *__restrict__ empty) {
  const int lane = lane_id(), b = blockIdx.y, m = blockIdx.x * (BT / 64) + (threadIdx.x >> 6);
  if (m >= M) return;                                // a whole wave; the kernel has no barrier
  const size_t bm = (size_t)b * M + m;
  const BoxF q = load_box_f32(boxes + bm * 7, MARGIN, ex, ey, ez);
  const float *p = pts + (size_t)b * N * stride;
  int *o = idx + bm * S;
  int cnt = 0;
  for (int base = 0; base < N && cnt < S; base += TRIP) {
    float x[TILES], y[TILES], z[TILES];
#pragma unroll
    for (int u = 0; u < TILES; u++) {                // every load of the trip before the first use: one round trip
      const int k = base + u * 64 + lane;
      const float *c = p + (size_t)(k < N ? k : N - 1) * stride;
      x[u] = c[0]; y[u] = c[1]; z[u] = c[2];
    }
#pragma unroll
    for (int u = 0; u < TILES; u++) {
      const int k = base + u * 64 + lane;
      const bool in = k < N && pt_in_box(q, x[u], y[u], z[u]);
      const unsigned long long hits = __ballot(in);
      const int rank = cnt + __popcll(hits & ((1ull << lane) - 1ull));
      if (in && rank < S) o[rank] = k;
      cnt += __popcll(hits);                         // (less than a trip past S)
    }
  }
  cnt = cnt < S ? cnt : S;
  for (int i = cnt + lane; i < S; i += 64) o[i] = -cnt;
  if (lane == 0) empty[bm] = cnt == 0 ? 1 : 0;
}

template <int FUSED>
__global__ __launch_bounds__(BT) void k_rp_gather(const float *__restrict__ pts, int stride, const float *__restrict__ feat,
                                                  const float *__restrict__ scores, const float *__restrict__ boxes,
                                                  const int *__restrict__ empty, int N, int M, int C, int S, int chunks,
                                                  float normalizer, int *idx, float *__restrict__ out) {
  constexpr int P = FUSED ? DFU3D_ROI_PREFIX_FUSED : DFU3D_ROI_PREFIX_PLAIN;
  const int lane = lane_id(), W = P + C;
  const size_t bm = blockIdx.x / (unsigned)chunks;   // < B * M
  const int k0 = (int)(blockIdx.x % (unsigned)chunks) * ROWS_WG + (threadIdx.x >> 6) * ROWS_WAVE;
  const size_t bn0 = bm / (unsigned)M * (size_t)N;   // the sample's first point
  int *slots = idx + bm * S;
  const bool none = empty[bm] != 0;
  const bool vec4 = (C & 3) == 0 && (reinterpret_cast<size_t>(feat) & 15) == 0;     // every feature row on 16 bytes
  float cx = 0.0f, cy = 0.0f, cz = 0.0f, cosa = 1.0f, sina = 0.0f;
  if (FUSED && !none) {
    const BoxF q = load_box_f32(boxes + bm * 7, MARGIN, 0.0f, 0.0f, 0.0f);
    cx = q.cx; cy = q.cy; cz = q.cz; cosa = q.cosa; sina = q.sina;
  }
  for (int j = 0; j < ROWS_WAVE; j++) {
    const int k = k0 + j;
    if (k >= S) break;                               // wave-uniform
    float *o = out + (bm * S + k) * W;
    if (none) {
      for (int col = lane; col < W; col += 64) o[col] = 0.0f;
      continue;
    }
    int i = slots[k];
    if (i < 0) {                                     // -cnt: the slot repeats slot k % cnt, which the search filled
      i = slots[k % -i];
      if (lane == 0) slots[k] = i;
    }
    i = readlane_i(i, 0);
    if ((unsigned)i >= (unsigned)N) i = 0;           // (never, for the slots the search wrote)
    const size_t src = bn0 + i;
    const float *c = pts + src * stride;
    const float x = c[0], y = c[1], z = c[2];
    float v0 = x, v1 = y, v2 = z, v3 = 0.0f, v4 = 0.0f;
    if (FUSED) {
      const float sx = x - cx, sy = y - cy;
      v0 = sx * cosa + sy * (-sina);
      v1 = sx * sina + sy * cosa;
      v2 = z - cz;
      v3 = scores[src];
      v4 = sqrtf(x * x + y * y + z * z) / normalizer - 0.5f;
    }
    const float *f = feat + src * C;                 // the point's feature row: columns P .. W - 1 of the pooled row
    if (vec4) {                                      // wave-uniform: a lane loads four floats and stores four dwords
      if (lane < P) o[lane] = lane == 0 ? v0 : lane == 1 ? v1 : lane == 2 ? v2 : lane == 3 ? v3 : v4;
      const float4 *f4 = reinterpret_cast<const float4 *>(f);
      for (int q = lane; q < (C >> 2); q += 64) {
        const float4 v = f4[q];
        float *d = o + P + 4 * q;                    // (a pooled row of P + C floats never starts on 16 bytes)
        d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w;
      }
      continue;
    }
    for (int col = lane; col < W; col += 64) {
      float v;
      if (col >= P) v = f[col - P];
      else v = col == 0 ? v0 : col == 1 ? v1 : col == 2 ? v2 : col == 3 ? v3 : v4;
      o[col] = v;
    }
  }
}

// DFU3D_OK, or DFU3D_ERANGE for a tensor of DFU3D_ROI_MAX_ELEMS elements or more
int range_of(double elems) { return elems >= (double)DFU3D_ROI_MAX_ELEMS ? DFU3D_ERANGE : DFU3D_OK; }

}  // namespace

extern "C" int32_t dfu3d_roi_version(void) { return DFU3D_ROI_VERSION; }

extern "C" int dfu3d_roi_pool(const float *points, int32_t pts_stride, const float *features, const float *scores,
                              const float *boxes3d, int32_t B, int32_t N, int32_t M, int32_t C, int32_t S, float extra_x,
                              float extra_y, float extra_z, int32_t fused, float depth_normalizer, float *pooled,
                              int32_t *pooled_empty_flag, int32_t *pooled_idx, void *stream) {
  DFU3D_CLEAR_STALE_ERROR();
  if (!points || !boxes3d || !pooled || !pooled_empty_flag || !pooled_idx) return DFU3D_EINVAL;
  if (B < 1 || N < 1 || M < 1 || S < 1 || C < 0 || pts_stride < 3 || pts_stride > DFU3D_ROI_MAX_PTS_STRIDE)
    return DFU3D_EINVAL;
  if ((C > 0 && !features) || (fused != 0 && fused != 1)) return DFU3D_EINVAL;
  if (fused && (!scores || !(depth_normalizer > 0.0f))) return DFU3D_EINVAL;
  const int W = (fused ? DFU3D_ROI_PREFIX_FUSED : DFU3D_ROI_PREFIX_PLAIN) + C;
  int rc = range_of((double)B * N * (double)pts_stride);
  if (rc == DFU3D_OK) rc = range_of((double)B * N * (double)C);
  if (rc == DFU3D_OK) rc = range_of((double)B * M * 7.0);
  if (rc == DFU3D_OK) rc = range_of((double)B * M * (double)S * (double)W);
  if (rc != DFU3D_OK) return rc;
  if (B > DFU3D_ROI_MAX_BATCH) return DFU3D_ERANGE;  // (the search's grid)
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(k_rp_search, dim3((unsigned)((M + BT / 64 - 1) / (BT / 64)), (unsigned)B), dim3(BT), 0, st, points,
                     pts_stride, boxes3d, N, M, S, extra_x, extra_y, extra_z, pooled_idx, pooled_empty_flag);
  DFU3D_LAUNCH_CHECK();
  const int chunks = (S + ROWS_WG - 1) / ROWS_WG;
  const dim3 grid((unsigned)((int64_t)B * M * chunks));           // < 2^31: B * M * S is
  if (fused)
    hipLaunchKernelGGL(k_rp_gather<1>, grid, dim3(BT), 0, st, points, pts_stride, features, scores, boxes3d,
                       (const int *)pooled_empty_flag, N, M, C, S, chunks, depth_normalizer, pooled_idx, pooled);
  else
    hipLaunchKernelGGL(k_rp_gather<0>, grid, dim3(BT), 0, st, points, pts_stride, features, scores, boxes3d,
                       (const int *)pooled_empty_flag, N, M, C, S, chunks, depth_normalizer, pooled_idx, pooled);
  DFU3D_LAUNCH_CHECK();
  return DFU3D_OK;
}
static_assert(DFU3D_ROI_LAUNCHES == 2, "the search and the gather");
