// anchor_stage.hip -- the anchor target assignment of AnchorHeadSingle for a whole batch (C ABI: dfu3d_anc.h).
//
//   k_anc_prep   one workgroup per sample: cuts the trailing zero rows, and writes per class set the list of the sample's
//                boxes in row order -- BEV rectangle, row, class -- with every box's top IoU cleared
//   k_anc_top    one thread per (sample, anchor): the IoU with the boxes of its set; the per-box maximum through integer
//                atomics on the float's bits (IoU >= 0: the bits are ordered), first in LDS, then one per box and workgroup
//   k_anc_emit   one thread per (sample, anchor): the same IoUs again (the same device function: the same bits), best and
//                lowest arg, forced or not, the label, the encoded target, the weight; targets leave through LDS so that
//                the (A, 7) block is written in whole lines
//
// The stage is a streaming write of B * A * 9 words next to a read of A * 7; the boxes of a sample are a small table
// every workgroup stages in LDS.  Threads of a wave belong to different class sets (the sets alternate inside a
// location), so a wave walks the lists of all sets, each under the mask of its own lanes.
#include "common.hpp"
#include "dfu3d_anc.h"

namespace {

constexpr int AT = DFU3D_ANC_THREADS;
constexpr int MB = DFU3D_ANC_MAX_BOXES;
constexpr int MS = DFU3D_ANC_MAX_SETS;

struct AncSets {
  int n;
  int begin[MS + 1];
  float matched[MS], unmatched[MS];
  int class_id[MS];
};

struct AncScratch { size_t off, rect, row, cls, top, bytes; };
__host__ inline size_t anc_up16(size_t v) { return (v + 15u) & ~(size_t)15u; }
__host__ inline AncScratch anc_scratch(int B, int M) {
  AncScratch s;
  const size_t rows = (size_t)B * (size_t)M;
  s.off = 0;
  s.rect = s.off + anc_up16((size_t)B * (MS + 1) * 4);
  s.row = s.rect + rows * 16;
  s.cls = s.row + anc_up16(rows * 4);
  s.top = s.cls + anc_up16(rows * 4);
  s.bytes = s.top + anc_up16(rows * 4);
  return s;
}

// ---- the one statement of the IoU ------------------------------------------------------------------------------------
// boxes3d_lidar_to_aligned_bev_boxes, float32, operation by operation (x1, y1, x2, y2)
__device__ __forceinline__ float4 anc_bev_rect(float x, float y, float dx, float dy, float heading) {
  const float PI_F = 3.14159274101257324219f;            // (float)pi
  const float QUARTER = 0.785398185253143310547f;        // (float)(pi / 4)
  float t = heading / PI_F;
  t = t + 0.5f;
  t = floorf(t);
  t = t * PI_F;
  const float r = fabsf(heading - t);
  const bool keep = r < QUARTER;
  const float hx = (keep ? dx : dy) / 2.0f, hy = (keep ? dy : dx) / 2.0f;
  return make_float4(x - hx, y - hy, x + hx, y + hy);
}
// boxes_iou_normal of two rectangles.  Without overlap the quotient is 0 / union = 0: the division is left out.
__device__ __forceinline__ float anc_iou(const float4 a, const float4 b) {
  const float x_min = fmaxf(a.x, b.x), x_max = fminf(a.z, b.z);
  const float y_min = fmaxf(a.y, b.y), y_max = fminf(a.w, b.w);
  const float x_len = fmaxf(x_max - x_min, 0.0f), y_len = fmaxf(y_max - y_min, 0.0f);
  const float area_a = (a.z - a.x) * (a.w - a.y), area_b = (b.z - b.x) * (b.w - b.y);
  const float inter = x_len * y_len;
  if (!(inter > 0.0f)) return 0.0f;
  const float uni = fmaxf((area_a + area_b) - inter, 1e-6f);
  return inter / uni;
}

// the class set of the slot k of a location
__device__ __forceinline__ int anc_set_of(const AncSets &S, int k) {
  int s = 0;
#pragma unroll
  for (int i = 1; i < MS; i++) s += (i < S.n && k >= S.begin[i]) ? 1 : 0;
  return s;
}

__global__ __launch_bounds__(MB) void k_anc_prep(const float *__restrict__ gt, int M, const AncSets S,
                                                 int *__restrict__ set_off, float4 *__restrict__ rect,
                                                 int *__restrict__ row, int *__restrict__ cls,
                                                 uint32_t *__restrict__ top) {
  __shared__ int s_last;
  __shared__ int s_w[MB / 64];
  const int b = blockIdx.x, j = threadIdx.x;
  if (j == 0) s_last = 0;
  __syncthreads();
  float v[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  if (j < M) {
    const float *p = gt + ((size_t)b * M + j) * 8;
#pragma unroll
    for (int c = 0; c < 8; c++) v[c] = p[c];
    const float sum = (((((v[0] + v[1]) + v[2]) + v[3]) + v[4]) + v[5]) + v[6];
    if (!(sum == 0.0f)) atomicMax(&s_last, j);
  }
  __syncthreads();
  const int n = M > 0 ? s_last + 1 : 0;                  // row 0 always stays
  const bool live = j < n;
  const int c = live ? (int)v[7] : -1;
  int mine = -1;
#pragma unroll
  for (int s = 0; s < MS; s++)
    if (s < S.n && live && (c == S.class_id[s] || (c == 0 && s == S.n - 1))) mine = s;
  int *off = set_off + (size_t)b * (MS + 1);
  int base = 0;
  if (j == 0) off[0] = 0;
  for (int s = 0; s < MS; s++) {                         // uniform: barriers inside
    int tot;
    const int r = block_rank<MB / 64>(mine == s, s_w, tot);
    if (mine == s) {
      const size_t o = (size_t)b * M + base + r;
      rect[o] = anc_bev_rect(v[0], v[1], v[3], v[4], v[6]);
      row[o] = j;
      cls[o] = c;
      top[o] = 0u;
    }
    base += tot;
    if (j == 0) off[s + 1] = base;
  }
}

// the lists of sample b into LDS; returns the number of entries (<= M <= MB)
__device__ __forceinline__ int anc_stage_lists(const int *__restrict__ set_off, const float4 *__restrict__ rect, int b, int M,
                                               int *s_off, float4 *s_rect) {
  if (threadIdx.x <= MS) s_off[threadIdx.x] = set_off[(size_t)b * (MS + 1) + threadIdx.x];
  __syncthreads();
  const int n = min(max(s_off[MS], 0), min(M, MB));
  for (int i = threadIdx.x; i < n; i += AT) s_rect[i] = rect[(size_t)b * M + i];
  return n;
}

__global__ __launch_bounds__(AT) void k_anc_top(const float *__restrict__ anchors, int A, int per_loc, const AncSets S,
                                                int M, const int *__restrict__ set_off,
                                                const float4 *__restrict__ rect, uint32_t *__restrict__ top) {
  __shared__ int s_off[MS + 1];
  __shared__ float4 s_rect[MB];
  __shared__ uint32_t s_top[MB];
  const int b = blockIdx.y;
  const int n = anc_stage_lists(set_off, rect, b, M, s_off, s_rect);
  if (n == 0) return;                                    // uniform
  for (int i = threadIdx.x; i < n; i += AT) s_top[i] = 0u;
  __syncthreads();
  const long long a = (long long)blockIdx.x * AT + threadIdx.x;
  if (a < A) {
    const float *p = anchors + (size_t)a * 7;
    const float4 ra = anc_bev_rect(p[0], p[1], p[3], p[4], p[6]);
    const int s = anc_set_of(S, (int)(a % per_loc));
    const int g0 = min(max(s_off[s], 0), n), g1 = min(max(s_off[s + 1], g0), n);
    for (int g = g0; g < g1; g++) {
      const float v = anc_iou(ra, s_rect[g]);
      if (v > 0.0f) {
        const uint32_t bits = __float_as_uint(v);
        if (bits > ((volatile uint32_t *)s_top)[g]) atomicMax(&s_top[g], bits);
      }
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < n; i += AT)
    if (s_top[i]) atomicMax(&top[(size_t)b * M + i], s_top[i]);
}

__global__ __launch_bounds__(AT) void k_anc_emit(const float *__restrict__ anchors, int A, int per_loc, const AncSets S,
                                                 const float *__restrict__ gt, int M, const int *__restrict__ set_off,
                                                 const float4 *__restrict__ rect, const int *__restrict__ row,
                                                 const int *__restrict__ cls, const uint32_t *__restrict__ top,
                                                 int *__restrict__ labels, float *__restrict__ targets,
                                                 float *__restrict__ weights) {
  __shared__ int s_off[MS + 1];
  __shared__ float4 s_rect[MB];
  __shared__ float s_top[MB];
  __shared__ int s_cls[MB];
  __shared__ float s_out[AT * 7];
  const int b = blockIdx.y;
  const int n = anc_stage_lists(set_off, rect, b, M, s_off, s_rect);
  for (int i = threadIdx.x; i < n; i += AT) {
    s_top[i] = __uint_as_float(top[(size_t)b * M + i]);
    s_cls[i] = cls[(size_t)b * M + i];
  }
  __syncthreads();
  const long long a0 = (long long)blockIdx.x * AT;
  const long long a = a0 + threadIdx.x;
  float t[7] = {0, 0, 0, 0, 0, 0, 0};
  if (a < A) {
    const float *p = anchors + (size_t)a * 7;
    float an[7];
#pragma unroll
    for (int c = 0; c < 7; c++) an[c] = p[c];
    const float4 ra = anc_bev_rect(an[0], an[1], an[3], an[4], an[6]);
    const int s = anc_set_of(S, (int)(a % per_loc));
    float matched = S.matched[0], unmatched = S.unmatched[0];
#pragma unroll
    for (int i = 1; i < MS; i++)
      if (s == i) { matched = S.matched[i]; unmatched = S.unmatched[i]; }
    const int g0 = min(max(s_off[s], 0), n), g1 = min(max(s_off[s + 1], g0), n);
    int label = 0, arg = -1;
    if (g1 > g0) {
      float best = anc_iou(ra, s_rect[g0]);
      arg = g0;
      bool forced = best > 0.0f && best == s_top[g0];
      for (int g = g0 + 1; g < g1; g++) {
        const float v = anc_iou(ra, s_rect[g]);
        if (v > best) { best = v; arg = g; }
        forced = forced || (v > 0.0f && v == s_top[g]);
      }
      const int c = s_cls[arg];
      label = forced ? c : (best < unmatched ? 0 : (best >= matched ? c : -1));
    }
    if (label > 0) {
      const int r = min(max(row[(size_t)b * M + arg], 0), M - 1);
      const float *q = gt + ((size_t)b * M + r) * 8;
      const float dxa = fmaxf(an[3], 1e-5f), dya = fmaxf(an[4], 1e-5f), dza = fmaxf(an[5], 1e-5f);
      const float dxg = fmaxf(q[3], 1e-5f), dyg = fmaxf(q[4], 1e-5f), dzg = fmaxf(q[5], 1e-5f);
      const float diag = sqrtf(dxa * dxa + dya * dya);
      t[0] = (q[0] - an[0]) / diag;
      t[1] = (q[1] - an[1]) / diag;
      t[2] = (q[2] - an[2]) / dza;
      t[3] = logf(dxg / dxa);
      t[4] = logf(dyg / dya);
      t[5] = logf(dzg / dza);
      t[6] = q[6] - an[6];
    }
    labels[(size_t)b * A + a] = label;
    weights[(size_t)b * A + a] = label > 0 ? 1.0f : 0.0f;
  }
#pragma unroll
  for (int c = 0; c < 7; c++) s_out[threadIdx.x * 7 + c] = t[c];
  __syncthreads();
  const long long left = (long long)A - a0;
  const int words = (int)(left < AT ? left : AT) * 7;
  float *out = targets + ((size_t)b * A + (size_t)a0) * 7;
  for (int i = threadIdx.x; i < words; i += AT) out[i] = s_out[i];
}

bool anc_sizes_ok(int B, int A, int M) {
  return B >= 0 && A >= 0 && M >= 0 && M <= DFU3D_ANC_MAX_BOXES && B <= DFU3D_ANC_MAX_BATCH;
}

}  // namespace

static_assert(DFU3D_ANC_LAUNCHES == 3, "k_anc_prep, k_anc_top, k_anc_emit");
static_assert(DFU3D_ANC_MAX_BOXES % 64 == 0 && DFU3D_ANC_MAX_BOXES <= 1024 && DFU3D_ANC_THREADS % 64 == 0 &&
              DFU3D_ANC_THREADS > DFU3D_ANC_MAX_SETS, "workgroup shapes");

extern "C" int32_t dfu3d_anc_version(void) { return DFU3D_ANC_VERSION; }

extern "C" size_t dfu3d_anc_scratch_bytes(int32_t B, int32_t A, int32_t M) {
  if (!anc_sizes_ok(B, A, M) || B == 0) return 0;
  return anc_scratch(B, M).bytes;
}

extern "C" int dfu3d_anchor_targets(const float *anchors, int32_t A, int32_t per_loc, const int32_t *set_begin,
                                    const float *matched, const float *unmatched, const int32_t *class_id, int32_t S,
                                    const float *gt_boxes, int32_t B, int32_t M, void *scratch, size_t scratch_bytes,
                                    int32_t *box_cls_labels, float *box_reg_targets, float *reg_weights, void *stream) {
  DFU3D_CLEAR_STALE_ERROR();
  if (!anchors || !set_begin || !matched || !unmatched || !class_id || !scratch || !box_cls_labels || !box_reg_targets ||
      !reg_weights)
    return DFU3D_EINVAL;
  if (A < 0 || B < 0 || M < 0 || S < 1 || per_loc < 1 || (M > 0 && !gt_boxes)) return DFU3D_EINVAL;
  if (S > DFU3D_ANC_MAX_SETS) return DFU3D_ERANGE;
  if (A % per_loc != 0 || set_begin[0] != 0 || set_begin[S] != per_loc) return DFU3D_EINVAL;
  AncSets sets;
  memset(&sets, 0, sizeof(sets));
  sets.n = S;
  for (int s = 0; s < S; s++) {
    if (set_begin[s + 1] <= set_begin[s]) return DFU3D_EINVAL;
    if (!(matched[s] - matched[s] == 0.0f) || !(unmatched[s] - unmatched[s] == 0.0f)) return DFU3D_EINVAL;   // finite
    if (unmatched[s] > matched[s] || class_id[s] < 1) return DFU3D_EINVAL;
    for (int o = 0; o < s; o++)
      if (class_id[o] == class_id[s]) return DFU3D_EINVAL;
    sets.begin[s] = set_begin[s];
    sets.matched[s] = matched[s];
    sets.unmatched[s] = unmatched[s];
    sets.class_id[s] = class_id[s];
  }
  for (int s = S; s <= MS; s++) sets.begin[s] = per_loc;
  if (M > DFU3D_ANC_MAX_BOXES || B > DFU3D_ANC_MAX_BATCH) return DFU3D_ERANGE;
  if ((int64_t)B * A * 7 > (int64_t)DFU3D_ANC_MAX_ELEMS) return DFU3D_ERANGE;
  if (B == 0 || A == 0) return DFU3D_OK;
  const AncScratch L = anc_scratch(B, M);
  if (((uintptr_t)scratch & 15u) || scratch_bytes < L.bytes) return DFU3D_EINVAL;
  char *base = (char *)scratch;
  hipStream_t st = (hipStream_t)stream;
  int *set_off = (int *)(base + L.off), *row = (int *)(base + L.row), *cls = (int *)(base + L.cls);
  float4 *rect = (float4 *)(base + L.rect);
  uint32_t *top = (uint32_t *)(base + L.top);
  const dim3 grid((unsigned)(((int64_t)A + AT - 1) / AT), (unsigned)B);
  hipLaunchKernelGGL(k_anc_prep, dim3((unsigned)B), dim3(MB), 0, st, gt_boxes, M, sets, set_off, rect, row, cls, top);
  DFU3D_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_anc_top, grid, dim3(AT), 0, st, anchors, A, per_loc, sets, M, (const int *)set_off,
                     (const float4 *)rect, top);
  DFU3D_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_anc_emit, grid, dim3(AT), 0, st, anchors, A, per_loc, sets, gt_boxes, M, (const int *)set_off,
                     (const float4 *)rect, (const int *)row, (const int *)cls, (const uint32_t *)top,
                     (int *)box_cls_labels, box_reg_targets, reg_weights);
  DFU3D_LAUNCH_CHECK();
  return DFU3D_OK;
}
