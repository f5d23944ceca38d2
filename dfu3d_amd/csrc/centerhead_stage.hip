// centerhead_stage.hip -- SURVEY.md §8 row f-6: the geometry at the detector's head, where boxes meet the network.
//
// dfu3d_center_assign = CenterHead.assign_targets (pcdet/models/dense_heads/center_head.py:106-227) for all heads and all
// samples of a batch.  Both kernels walk a sample's boxes in chunks of CT and rank the ones whose class belongs to the
// head with a block scan (slot k = the k-th such box in input order); cell, radius and regression target are computed
// in the reference's float32 operation order (add / sub / mul / div / sqrt only, no contraction: bit-equal).
// k_ca_slots, one workgroup per (head, sample), writes the slots -- all num_max_objs of them, the unused ones as zeros, so
// that no output but the heat maps needs a fill; k_ca_transc adds the log / cos / sin columns, evaluated in fp64 and
// rounded, one thread per slot.  k_ca_draw, CDS workgroups per (head, sample): the chunk's drawable boxes
// go to LDS as (plane, cx, cy, radius) and the waves share them: one wave per record over its clipped
// (2r + 1)^2 footprint, the Gaussian exp(-(x^2 + y^2) / (2 sigma^2)), sigma = (2r + 1) / 6, evaluated in fp64 and rounded to
// float32 (centernet_utils.py:38-69), combined with an unsigned atomic max on the bit pattern: all values are
// non-negative floats, for which the integer order is the float order, and max does not depend on the order of the draws.
//
// dfu3d_center_decode = decode_bbox_from_heatmap (centernet_utils.py:155-241), k_cd_decode, one workgroup per sample.
// The workgroup radix select of common.hpp (block_select, the one the plane medians and the repair use) over the
// complemented 32 score bits at rank K - 1 finds the K-th largest score T and how many ties at T are kept; one more
// pass collects the scores above T in any order and, by an ordered block scan, the first ties at T by ascending flat index.
// The candidates are sorted in LDS as 64-bit keys (score bits, ~flat index): descending score, ties by ascending index,
// NaN first.  Every thread then gathers and decodes one row, and a block scan compacts the rows that pass the range and
// score tests, in order.
#include <math.h>

#include "common.hpp"

namespace {

constexpr int CT = 256;                      // threads of an assign workgroup = boxes per chunk
constexpr int CDS = 4;                       // workgroups per (head, sample) that share the drawing
constexpr int DT = 1024;                     // threads of a decode workgroup
constexpr int DK = DFU3D_CENTER_MAX_K;

struct CaCfg {
  float rx, ry, vx, vy, stride, hi_x, hi_y;  // hi = feature_map_size - 0.5
  float k1, k2, a34, b3k, c3k;               // 1 - o, 1 + o, 4 * (4 * o), -2 * o, o - 1 of GAUSSIAN_OVERLAP o, as float32
  int W, H, nmax, min_radius;
};

__device__ __forceinline__ float clampf(float v, float lo, float hi) { return v < lo ? lo : (v > hi ? hi : v); }

// centernet_utils.py:9-35 with height = dx, width = dy (center_head.py:138), float32, the operations as written there
__device__ __forceinline__ float gaussian_radius_f32(float h, float w, const CaCfg &g) {
  const float b1 = h + w;
  const float c1 = w * h * g.k1 / g.k2;
  const float r1 = (b1 + sqrtf(b1 * b1 - 4.0f * c1)) / 2.0f;
  const float b2 = 2.0f * b1;
  const float c2 = g.k1 * w * h;
  const float r2 = (b2 + sqrtf(b2 * b2 - 16.0f * c2)) / 2.0f;
  const float b3 = g.b3k * b1;
  const float c3 = g.c3k * w * h;
  const float r3 = (b3 + sqrtf(b3 * b3 - g.a34 * c3)) / 2.0f;        // r3 is not divided by a3, as in the reference
  return fminf(fminf(r1, r2), r3);
}

// One box of a chunk: its 0-based class within head h (-1: not this head's) and, by a block scan, its slot.
struct CaBox { int local, k; float cx, cy, dx, dy; int cxi, cyi; bool valid; };
__device__ __forceinline__ CaBox ca_box(const float *__restrict__ gt, int b, int M, int C, int i, int h, int ncls_h,
                                        const int *__restrict__ cls_tab, int n_cls, const CaCfg &g, int base, int *s_w,
                                        int &tot) {
  CaBox x;
  const float *row = gt + ((size_t)b * M + (i < M ? i : 0)) * C;
  x.local = -1;
  if (i < M) {
    const int cls = (int)row[C - 1];
    if (cls >= 1 && cls <= n_cls && cls_tab[2 * cls] == h) x.local = cls_tab[2 * cls + 1];
    if (x.local >= ncls_h) x.local = -1;                    // a table that contradicts head_plane: never index beyond the head
  }
  x.k = base + block_rank<CT / 64>(x.local >= 0, s_w, tot);
  x.valid = false;
  x.cx = x.cy = x.dx = x.dy = 0.0f;
  x.cxi = x.cyi = 0;
  if (x.local >= 0 && x.k < g.nmax) {
    x.cx = clampf((row[0] - g.rx) / g.vx / g.stride, 0.0f, g.hi_x);
    x.cy = clampf((row[1] - g.ry) / g.vy / g.stride, 0.0f, g.hi_y);
    x.cxi = min(max((int)x.cx, 0), g.W - 1);
    x.cyi = min(max((int)x.cy, 0), g.H - 1);
    x.dx = row[3] / g.vx / g.stride;
    x.dy = row[4] / g.vy / g.stride;
    x.valid = x.dx > 0.0f && x.dy > 0.0f;
  }
  return x;
}

// slots: one workgroup per (head, sample) writes all num_max_objs slots of its four outputs
__global__ __launch_bounds__(CT) void k_ca_slots(const float *__restrict__ gt, int B, int M, int C,
                                                 const int *__restrict__ cls_tab, int n_cls,
                                                 const int *__restrict__ head_plane, CaCfg g, float *__restrict__ tgt,
                                                 long long *__restrict__ inds, long long *__restrict__ masks,
                                                 float *__restrict__ src) {
  __shared__ int s_w[CT / 64];
  const int h = blockIdx.x / B, b = blockIdx.x % B, t = threadIdx.x;
  const int ncls_h = head_plane[h + 1] - head_plane[h];
  const size_t slot0 = (size_t)blockIdx.x * g.nmax;         // blockIdx.x = h * B + b
  tgt += slot0 * C;
  src += slot0 * C;
  inds += slot0;
  masks += slot0;
  int base = 0;
  for (int i0 = 0; i0 < M; i0 += CT) {
    int tot;
    const CaBox x = ca_box(gt, b, M, C, i0 + t, h, ncls_h, cls_tab, n_cls, g, base, s_w, tot);
    if (x.local >= 0 && x.k < g.nmax) {
      const float *row = gt + ((size_t)b * M + i0 + t) * C;
      float *s = src + x.k * C, *q = tgt + x.k * C;          // num_max_objs * C < 2^31 (host check)
#pragma unroll 1
      for (int c = 0; c < C - 1; c++) s[c] = row[c];
      s[C - 1] = (float)(x.local + 1);
#pragma unroll 1
      for (int c = 0; c < C; c++) q[c] = 0.0f;              // columns 3..7 of a valid slot: k_ca_transc
      if (x.valid) {
        q[0] = x.cx - (float)x.cxi;
        q[1] = x.cy - (float)x.cyi;
        q[2] = row[2];
#pragma unroll 1
        for (int c = 8; c < C; c++) q[c] = row[c - 1];
      }
      inds[x.k] = x.valid ? (long long)x.cyi * g.W + x.cxi : 0;
      masks[x.k] = x.valid ? 1 : 0;
    }
    base += tot;
  }
  const int k0 = min(base, g.nmax);
  for (int e = k0 * C + t; e < g.nmax * C; e += CT) {
    tgt[e] = 0.0f;
    src[e] = 0.0f;
  }
  for (int e = k0 + t; e < g.nmax; e += CT) {
    inds[e] = 0;
    masks[e] = 0;
  }
}

// log(dx dy dz), cos(yaw), sin(yaw) of the filled slots, evaluated in fp64 and rounded: one thread per slot, a kernel of its
// own so that the long fp64 routines run with few values live (inside k_ca_slots they spilled scalar registers)
__global__ __launch_bounds__(CT) void k_ca_transc(const float *__restrict__ src, const long long *__restrict__ masks,
                                                  int C, size_t n_slots, float *__restrict__ tgt) {
  const size_t e = (size_t)blockIdx.x * CT + threadIdx.x;
  if (e >= n_slots || masks[e] == 0) return;
  const float *s = src + e * C;
  float *q = tgt + e * C;
#pragma unroll 1
  for (int c = 3; c < 6; c++) q[c] = (float)log((double)s[c]);
  double sn, cs;
  sincos((double)s[6], &sn, &cs);
  q[6] = (float)cs;
  q[7] = (float)sn;
}

// draw: CDS workgroups per (head, sample) rank the boxes again (a few loads and one scan per chunk: cheaper than a
// record buffer between two kernels, and the library needs no scratch) and share the chunk's Gaussians wave by wave
__global__ __launch_bounds__(CT) void k_ca_draw(const float *__restrict__ gt, int B, int M, int C,
                                                const int *__restrict__ cls_tab, int n_cls,
                                                const int *__restrict__ head_plane, CaCfg g, float *__restrict__ heat,
                                                uint32_t *__restrict__ status) {
  __shared__ int4 s_rec[CT];
  __shared__ int s_w[CT / 64];
  const int h = blockIdx.x / B, b = blockIdx.x % B, t = threadIdx.x;
  const int p0 = head_plane[h], ncls_h = head_plane[h + 1] - p0;
  const size_t HW = (size_t)g.W * g.H;
  float *hm = heat + ((size_t)B * p0 + (size_t)b * ncls_h) * HW;
  int base = 0;
  for (int i0 = 0; i0 < M; i0 += CT) {
    int tot;
    const CaBox x = ca_box(gt, b, M, C, i0 + t, h, ncls_h, cls_tab, n_cls, g, base, s_w, tot);
    s_rec[t] = x.valid ? make_int4(x.local, x.cxi, x.cyi, max((int)gaussian_radius_f32(x.dx, x.dy, g), g.min_radius))
                       : make_int4(0, 0, 0, -1);
    __syncthreads();
    for (int j = blockIdx.y * (CT / 64) + (t >> 6); j < CT; j += CDS * (CT / 64)) {
      const int4 r = s_rec[j];
      if (r.w < 0) continue;
      const int rad = min(r.w, 1 << 20);                    // the footprint is clipped to the map anyway
      const int left = min(r.y, rad), right = min(g.W - r.y, rad + 1);
      const int top = min(r.z, rad), bottom = min(g.H - r.z, rad + 1);
      const int fw = left + right, n = fw * (top + bottom);
      const double sigma = (2.0 * (double)r.w + 1.0) / 6.0, den = 2.0 * sigma * sigma;
      uint32_t *plane = (uint32_t *)(hm + (size_t)r.x * HW);
      for (int e = lane_id(); e < n; e += 64) {
        const int oy = e / fw - top, ox = e % fw - left;
        double v = exp(-(double)(ox * ox + oy * oy) / den);
        if (v < 2.220446049250313e-16) v = 0.0;             // h[h < eps * h.max()] = 0, h.max() = 1 at the centre
        atomicMax(plane + (size_t)(r.z + oy) * g.W + (r.y + ox), __float_as_uint((float)v));
      }
    }
    __syncthreads();
    base += tot;
  }
  if (blockIdx.y == 0 && t == 0 && base > g.nmax) atomicOr(status, DFU3D_ST_CENTER_OVERFLOW);   // k_ca_slots cut them
}

// ---- decode -----------------------------------------------------------------------------------------------------------
struct CdCfg {
  float rx, ry, vx, vy, stride, thresh;
  int use_thresh, n_cls, H, W, K;
};

// monotone map float -> uint32 for the order of torch.topk: NaN above everything, -0 == +0
__device__ __forceinline__ uint32_t score_key(float v) {
  uint32_t b = __float_as_uint(v);
  if (v != v) return 0xFFFFFFFFu;
  if (b == 0x80000000u) b = 0u;
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

__global__ __launch_bounds__(DT) void k_cd_decode(const float *__restrict__ heat, const float *__restrict__ rot_cos,
                                                  const float *__restrict__ rot_sin, const float *__restrict__ center,
                                                  const float *__restrict__ center_z, const float *__restrict__ dim,
                                                  const float *__restrict__ vel, const float *__restrict__ iou, CdCfg g,
                                                  const float *__restrict__ limit, float *__restrict__ boxes,
                                                  float *__restrict__ scores, int *__restrict__ labels,
                                                  float *__restrict__ iou_out, int *__restrict__ count) {
  __shared__ unsigned long long s_key[DK];
  __shared__ int s_hist[256];
  __shared__ int s_w[DT / 64];
  __shared__ unsigned long long s_sel[3];
  __shared__ int s_cnt;
  const int b = blockIdx.x, t = threadIdx.x;
  const int HW = g.H * g.W, N = g.n_cls * HW, K = g.K;
  const float *hp = heat + (size_t)b * N;

  // the K-th largest key is the complement of the key with ascending rank K - 1 among the complements (K <= N: host check)
  const auto sel = block_select<DT, 32, uint32_t>(N, K - 1, [&](int i) { return ~score_key(hp[i]); }, s_hist, s_sel);
  // keys above T in any order into [0, G), the first `need` keys equal to T by ascending index into [G, K)
  const uint32_t T = ~sel.key;
  const int need = sel.rank + 1, G = K - need;
  if (t == 0) s_cnt = 0;
  for (int i = t; i < DK; i += DT) s_key[i] = 0ull;      // padding sorts last: no real key is 0
  __syncthreads();
  int eq_base = 0;
  for (int i0 = 0; i0 < N; i0 += DT) {
    const int i = i0 + t;
    const uint32_t key = i < N ? score_key(hp[i]) : 0u;
    const unsigned long long kk = ((unsigned long long)key << 32) | (uint32_t)~(uint32_t)i;
    if (i < N && key > T) {
      const int pos = atomicAdd(&s_cnt, 1);
      if (pos < G) s_key[pos] = kk;
    }
    if (eq_base < need) {                                  // uniform: eq_base is a block total
      const bool eq = i < N && key == T;
      int tot;
      const int r = eq_base + block_rank<DT / 64>(eq, s_w, tot);
      if (eq && r < need) s_key[G + r] = kk;
      eq_base += tot;
    }
  }
  __syncthreads();
  // bitonic sort, descending, of the smallest power of two >= K
  int n2 = 1;
  while (n2 < K) n2 <<= 1;
  for (int k = 2; k <= n2; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      const int o = t ^ j;
      if (t < n2 && o > t) {
        const unsigned long long a = s_key[t], c = s_key[o];
        const bool desc = (t & k) == 0;
        if (desc ? a < c : a > c) {
          s_key[t] = c;
          s_key[o] = a;
        }
      }
      __syncthreads();
    }
  }
  // gather, decode, mask, ordered compaction
  const int nb = vel ? 9 : 7;
  bool keep = false;
  float bx[9], sc = 0.0f, io = 0.0f;
  int cls = 0;
  if (t < K) {
    const uint32_t idx = ~(uint32_t)s_key[t];
    cls = (int)(idx / (uint32_t)HW);
    const int cell = (int)(idx % (uint32_t)HW);
    const float ys = (float)(cell / g.W), xs = (float)(cell % g.W);
    sc = hp[idx];
    const size_t o1 = (size_t)b * HW + cell, o2 = (size_t)b * 2 * HW + cell, o3 = (size_t)b * 3 * HW + cell;
    bx[0] = (xs + center[o2]) * g.stride * g.vx + g.rx;
    bx[1] = (ys + center[o2 + HW]) * g.stride * g.vy + g.ry;
    bx[2] = center_z[o1];
    bx[3] = dim[o3];
    bx[4] = dim[o3 + HW];
    bx[5] = dim[o3 + 2 * (size_t)HW];
    bx[6] = (float)atan2((double)rot_sin[o1], (double)rot_cos[o1]);
    bx[7] = vel ? vel[o2] : 0.0f;
    bx[8] = vel ? vel[o2 + HW] : 0.0f;
    io = iou ? iou[o1] : 0.0f;
    keep = bx[0] >= limit[0] && bx[1] >= limit[1] && bx[2] >= limit[2] && bx[0] <= limit[3] && bx[1] <= limit[4] &&
           bx[2] <= limit[5] && (!g.use_thresh || sc > g.thresh);
  }
  int tot;
  const int r = block_rank<DT / 64>(keep, s_w, tot);
  if (keep) {
    float *q = boxes + ((size_t)b * K + r) * nb;
#pragma unroll
    for (int c = 0; c < 7; c++) q[c] = bx[c];
    if (vel) {
      q[7] = bx[7];
      q[8] = bx[8];
    }
    scores[(size_t)b * K + r] = sc;
    labels[(size_t)b * K + r] = cls;
    if (iou) iou_out[(size_t)b * K + r] = io;
  }
  if (t == 0) count[b] = tot;
}

}  // namespace

extern "C" int dfu3d_center_assign(const float *gt_boxes, int32_t B, int32_t M, int32_t C, const int32_t *cls_tab,
                                   int32_t n_cls, const int32_t *head_plane, int32_t n_heads, int32_t W, int32_t H,
                                   float range_x, float range_y, float voxel_x, float voxel_y, int32_t stride,
                                   int32_t num_max_objs, double gaussian_overlap, int32_t min_radius, float *heat,
                                   float *target_boxes, int64_t *inds, int64_t *masks, float *target_boxes_src,
                                   uint32_t *status, void *stream) {
  DFU3D_CLEAR_STALE_ERROR();
  if (!cls_tab || !head_plane || !heat || !target_boxes || !inds || !masks || !target_boxes_src || !status)
    return DFU3D_EINVAL;
  if (B < 0 || M < 0 || C < 8 || n_cls < 1 || n_heads < 1 || W < 1 || H < 1 || stride < 1 || num_max_objs < 1 ||
      min_radius < 0 || !(voxel_x > 0.0f) || !(voxel_y > 0.0f))
    return DFU3D_EINVAL;
  if (!gt_boxes && (int64_t)B * M > 0) return DFU3D_EINVAL;
  if (W > 16384 || H > 16384 || (int64_t)B * n_heads * num_max_objs > 0x7FFFFFFF ||
      (int64_t)num_max_objs * C > 0x7FFFFFFF)
    return DFU3D_ERANGE;
  if (B == 0) return DFU3D_OK;
  CaCfg g;
  g.rx = range_x; g.ry = range_y; g.vx = voxel_x; g.vy = voxel_y; g.stride = (float)stride;
  g.hi_x = (float)((double)W - 0.5); g.hi_y = (float)((double)H - 0.5);
  const double o = gaussian_overlap;                      // the reference's Python scalars, each rounded to float32 once
  g.k1 = (float)(1 - o); g.k2 = (float)(1 + o); g.a34 = (float)(4 * (4 * o)); g.b3k = (float)(-2 * o); g.c3k = (float)(o - 1);
  g.W = W; g.H = H; g.nmax = num_max_objs; g.min_radius = min_radius;
  hipStream_t st = (hipStream_t)stream;
  if (dfu3d_fill_async(heat, 0, (size_t)B * n_cls * W * H * 4, st) != hipSuccess) return DFU3D_ELAUNCH;
  hipLaunchKernelGGL(k_ca_slots, dim3((unsigned)(B * n_heads)), dim3(CT), 0, st, gt_boxes, B, M, C, cls_tab, n_cls,
                     head_plane, g, target_boxes, (long long *)inds, (long long *)masks, target_boxes_src);
  DFU3D_LAUNCH_CHECK();
  const size_t n_slots = (size_t)B * n_heads * num_max_objs;
  hipLaunchKernelGGL(k_ca_transc, dim3((unsigned)((n_slots + CT - 1) / CT)), dim3(CT), 0, st, target_boxes_src,
                     (const long long *)masks, C, n_slots, target_boxes);
  DFU3D_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_ca_draw, dim3((unsigned)(B * n_heads), CDS), dim3(CT), 0, st, gt_boxes, B, M, C, cls_tab, n_cls,
                     head_plane, g, heat, status);
  DFU3D_LAUNCH_CHECK();
  return DFU3D_OK;
}

extern "C" int dfu3d_center_decode(const float *heat, const float *rot_cos, const float *rot_sin, const float *center,
                                   const float *center_z, const float *dim, const float *vel, const float *iou,
                                   int32_t B, int32_t n_cls, int32_t H, int32_t W, int32_t K, float range_x,
                                   float range_y, float voxel_x, float voxel_y, int32_t stride, const float *limit,
                                   int32_t use_thresh, float score_thresh, float *boxes, float *scores, int32_t *labels,
                                   float *iou_out, int32_t *count, void *stream) {
  DFU3D_CLEAR_STALE_ERROR();
  if (!heat || !rot_cos || !rot_sin || !center || !center_z || !dim || !limit || !boxes || !scores || !labels || !count)
    return DFU3D_EINVAL;
  if (iou && !iou_out) return DFU3D_EINVAL;
  if (B < 0 || n_cls < 1 || H < 1 || W < 1 || K < 1 || stride < 1) return DFU3D_EINVAL;
  if ((int64_t)n_cls * H * W > (1 << 30)) return DFU3D_ERANGE;
  if (K > n_cls * H * W) return DFU3D_EINVAL;
  if (K > DFU3D_CENTER_MAX_K) return DFU3D_ERANGE;
  if (B == 0) return DFU3D_OK;
  CdCfg g;
  g.rx = range_x; g.ry = range_y; g.vx = voxel_x; g.vy = voxel_y; g.stride = (float)stride; g.thresh = score_thresh;
  g.use_thresh = use_thresh; g.n_cls = n_cls; g.H = H; g.W = W; g.K = K;
  hipLaunchKernelGGL(k_cd_decode, dim3((unsigned)B), dim3(DT), 0, (hipStream_t)stream, heat, rot_cos, rot_sin, center,
                     center_z, dim, vel, iou, g, limit, boxes, scores, labels, iou_out, count);
  DFU3D_LAUNCH_CHECK();
  return DFU3D_OK;
}
