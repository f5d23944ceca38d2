// postproc_stage.hip -- SURVEY.md §8 row f-9: the inference end of the CenterPoint head for a whole batch.  Rotated NMS
// of S = heads x samples box lists ("segments") in two launches, and the gather of the survivors of all heads into
// one padded block per sample in a third (include/dfu3d_post.h).
//
// What it stands in for in the reference: the per-(head, sample) loop of center_head.py:297-364 over
// model_nms_utils.class_agnostic_nms (topk, gathers, iou3d_nms nms_gpu with its host walk over the mask) and the
// torch.cat of the heads.  The decode (centerhead_stage.hip) returns its rows in descending score order already, so
// nothing is sorted here.
//
//   k_pp_mask     one wave per row i of a segment: the wave goes over the 64-box blocks from i's own to the segment's last;
//                 lane l tests box 64 cb + l against box i and the ballot is the word, as in k_suppress_mask
//                 (iou_stage.hip); both decide a pair with nms_suppresses (rect_overlap.hpp): the same bits.
//   k_pp_walk     one workgroup per segment.  The mask rows are staged in LDS where they fit (up to 704 rows; 500 rows x 8 words
//                 = 32 KB), then wave 0 walks 64 rows at a time: lane l holds the diagonal word of row 64 blk + l, the
//                 greedy chain inside the block runs on wave-uniform values (a find-first-zero and a lane read per KEPT
//                 row, no memory access), and the words of the kept rows are OR-ed into the running set by 16 independent
//                 loads (4 rows x 16 words per step).  cap <= 1024: the running set is one word in each of 16 lanes.
//   k_pp_collect  one workgroup per (sample, head): kept rows to their place behind the earlier heads' rows, class map,
//                 zeros behind the last row.
#include "common.hpp"
#include "rect_overlap.hpp"
#include "dfu3d_post.h"

namespace {

constexpr int PP_MAXW = DFU3D_POST_MAX_CAP / 64;        // words of a mask row at most
constexpr int PP_LDS_WORDS = 8000;                      // staged mask rows: 64000 bytes of the 64 KiB
constexpr int PT = 256;

// THE layout of the scratch of dfu3d_nms_bev_segments; the size is its last field
struct PpScratch {
  size_t mask;                                          // uint64 (S, cap, wcap), wcap = ceil(cap / 64)
  size_t bytes;
};

PpScratch pp_scratch(int S, int cap) {
  PpScratch s;
  size_t o = 0;
  s.mask = o; o += (size_t)S * cap * ((cap + 63) / 64) * sizeof(unsigned long long);
  s.bytes = o + 16;
  return s;
}

__device__ __forceinline__ int seg_rows(const int *__restrict__ count, int s, int cap, int pre_max) {
  int n = count[s];
  n = n < 0 ? 0 : (n > cap ? cap : n);
  return (pre_max > 0 && pre_max < n) ? pre_max : n;
}

__global__ __launch_bounds__(IB) void k_pp_mask(const float *__restrict__ boxes, int cap, int C,
                                                const int *__restrict__ count, float thresh, int pre_max, int normal,
                                                int wcap, unsigned long long *__restrict__ mask) {
  __shared__ float s_poly[4][MAXV * IB];
  const int s = blockIdx.x;
  const int n = seg_rows(count, s, cap, pre_max);
  const int i = blockIdx.y * (IB / 64) + (threadIdx.x >> 6);
  if (i >= n) return;                                        // uniform per wave (no barrier in this kernel)
  const int lane = lane_id();
  const float *seg = boxes + (size_t)s * cap * C;
  const Rect A = make_rect(seg + (size_t)i * C, 7);
  const int nblk = (n + 63) >> 6;
  unsigned long long *row = mask + ((size_t)s * cap + i) * wcap;
  for (int cb = i >> 6; cb < nblk; cb++) {
    const int j = cb * 64 + lane;
    bool over = false;
    if (j < n && j > i) {
      const Rect B = make_rect(seg + (size_t)j * C, 7);
      over = nms_suppresses(A, B, normal, thresh, s_poly[0] + threadIdx.x, s_poly[1] + threadIdx.x,
                            s_poly[2] + threadIdx.x, s_poly[3] + threadIdx.x);
    }
    const unsigned long long word = __ballot(over);
    if (lane == 0) row[cb] = word;
  }
}

__global__ __launch_bounds__(PT) void k_pp_walk(const unsigned long long *__restrict__ mask,
                                                const int *__restrict__ count, int cap, int wcap, int pre_max,
                                                int post_max, int *__restrict__ keep, int *__restrict__ num_keep) {
  __shared__ unsigned long long s_rows[PP_LDS_WORDS];
  __shared__ unsigned long long s_kept[PP_MAXW];
  const int s = blockIdx.x, t = threadIdx.x;
  const int n = seg_rows(count, s, cap, pre_max);
  const int wn = (n + 63) >> 6;
  const unsigned long long *g = mask + (size_t)s * cap * wcap;
  const bool staged = n * wn <= PP_LDS_WORDS;
  if (staged) {
    for (int idx = t; idx < n * wn; idx += PT) {
      const int i = idx / wn, w = idx - i * wn;
      s_rows[idx] = (w >= (i >> 6)) ? g[(size_t)i * wcap + w] : 0ull;      // words before the row's block were never written
    }
  }
  if (t < PP_MAXW) s_kept[t] = 0ull;
  __syncthreads();
  if (t < 64) {
    const int lane = t, w = lane & 15, quarter = lane >> 4;
    const int limit = post_max > 0 ? post_max : 0x7FFFFFFF;
    unsigned long long remv = 0ull;                          // lane l (and l + 16, ...) holds word l & 15 of the suppressed set
    int nk = 0;
    for (int blk = 0; blk < wn && nk < limit; blk++) {
      const int r0 = blk * 64;
      unsigned long long diag = 0ull;
      if (r0 + lane < n) diag = staged ? s_rows[(r0 + lane) * wn + blk] : g[(size_t)(r0 + lane) * wcap + blk];
      unsigned long long cur = readlane_u64(remv, blk);      // bit set: suppressed, walked or beyond the segment
      if (n - r0 < 64) cur |= ~0ull << (n - r0);
      unsigned long long kept = 0ull;
      while (~cur != 0ull && nk < limit) {
        const int b = __ffsll((long long)~cur) - 1;
        kept |= 1ull << b;
        nk++;
        cur |= readlane_u64(diag, b) | (1ull << b);
      }
      if (lane == 0) s_kept[blk] = kept;
      if (blk + 1 < wn) {
        unsigned long long acc = 0ull;
        const bool mine = w > blk && w < wn;
#pragma unroll
        for (int q = 0; q < 16; q++) {
          const int r = q * 4 + quarter;
          if (mine && ((kept >> r) & 1ull))
            acc |= staged ? s_rows[(r0 + r) * wn + w] : g[(size_t)(r0 + r) * wcap + w];
        }
        acc |= shfl_xor_u64(acc, 16);
        acc |= shfl_xor_u64(acc, 32);
        remv |= acc;
      }
    }
  }
  __syncthreads();
  int total = 0;
#pragma unroll
  for (int k = 0; k < PP_MAXW; k++) total += __popcll(s_kept[k]);
  int *out = keep + (size_t)s * cap;
  for (int i = t; i < cap; i += PT) {
    const int blk = i >> 6, bit = i & 63;
    const unsigned long long word = s_kept[blk];
    if ((word >> bit) & 1ull) {
      int rank = __popcll(word & ((1ull << bit) - 1ull));
      for (int k = 0; k < blk; k++) rank += __popcll(s_kept[k]);
      out[rank] = i;
    }
    if (i >= total) out[i] = -1;
  }
  if (t == 0) num_keep[s] = total;
}

__global__ __launch_bounds__(PT) void k_pp_collect(const float *__restrict__ boxes, const float *__restrict__ scores,
                                                   const int *__restrict__ labels, const int *__restrict__ keep,
                                                   const int *__restrict__ num_keep, int n_heads, int B, int cap, int C,
                                                   const int *__restrict__ cls_map, int max_cls, int out_cap,
                                                   float *__restrict__ out_boxes, float *__restrict__ out_scores,
                                                   long long *__restrict__ out_labels, int *__restrict__ out_count) {
  const int b = blockIdx.x, h = blockIdx.y, t = threadIdx.x;
  int base = 0, total = 0, mine = 0;
  for (int k = 0; k < n_heads; k++) {                        // uniform: every thread reads the same few counts
    int c = num_keep[(size_t)k * B + b];
    c = c < 0 ? 0 : (c > cap ? cap : c);
    if (k < h) base += c;
    if (k == h) mine = c;
    total += c;
  }
  const int filled = total < out_cap ? total : out_cap;
  const size_t seg = (size_t)h * B + b;
  float *ob = out_boxes + (size_t)b * out_cap * C;
  float *os = out_scores + (size_t)b * out_cap;
  long long *ol = out_labels + (size_t)b * out_cap;
  int rows = out_cap - base;                                 // rows of this head that fit
  rows = rows < 0 ? 0 : (rows < mine ? rows : mine);
  for (int idx = t; idx < rows * C; idx += PT) {
    const int r = idx / C, c = idx - r * C;
    const int k = keep[seg * cap + r];
    ob[(size_t)(base + r) * C + c] = (k >= 0 && k < cap) ? boxes[(seg * cap + k) * C + c] : 0.0f;
  }
  for (int r = t; r < rows; r += PT) {
    const int k = keep[seg * cap + r];
    const bool ok = k >= 0 && k < cap;
    const int l = ok ? labels[seg * cap + k] : -1;
    os[base + r] = ok ? scores[seg * cap + k] : 0.0f;
    ol[base + r] = (l >= 0 && l < max_cls) ? (long long)cls_map[(size_t)h * max_cls + l] + 1 : 0ll;
  }
  // the tail of the sample's block, shared out over the heads' workgroups
  const int tail = out_cap - filled;
  const int per = (tail + n_heads - 1) / n_heads;
  const int t0 = filled + h * per, t1 = (t0 + per < out_cap) ? t0 + per : out_cap;
  for (int idx = t0 * C + t; idx < t1 * C; idx += PT) ob[idx] = 0.0f;
  for (int r = t0 + t; r < t1; r += PT) {
    os[r] = 0.0f;
    ol[r] = 0ll;
  }
  if (h == 0 && t == 0) out_count[b] = filled;
}

}  // namespace

extern "C" size_t dfu3d_nms_segments_scratch_bytes(int32_t S, int32_t cap) {
  if (S < 0 || cap < 0 || cap > DFU3D_POST_MAX_CAP) return 0;
  return pp_scratch(S, cap).bytes;
}

extern "C" int dfu3d_nms_bev_segments(const float *boxes, int32_t S, int32_t cap, int32_t C, const int32_t *count,
                                      float thresh, int32_t pre_max, int32_t post_max, int32_t normal, void *scratch,
                                      size_t scratch_bytes, int32_t *keep, int32_t *num_keep, void *stream) {
  DFU3D_CLEAR_STALE_ERROR();
  if (!boxes || !count || !keep || !num_keep) return DFU3D_EINVAL;
  if (S < 0 || cap < 0 || C < 7) return DFU3D_EINVAL;
  if (cap > DFU3D_POST_MAX_CAP) return DFU3D_ERANGE;
  if (S == 0 || cap == 0) return DFU3D_OK;
  const PpScratch L = pp_scratch(S, cap);
  if (!scratch || ((uintptr_t)scratch & 7u) || scratch_bytes < L.bytes) return DFU3D_EINVAL;
  unsigned long long *mask = (unsigned long long *)((char *)scratch + L.mask);
  const int wcap = (cap + 63) / 64;
  const int rows = (pre_max > 0 && pre_max < cap) ? pre_max : cap;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(k_pp_mask, dim3((unsigned)S, (unsigned)((rows + IB / 64 - 1) / (IB / 64))), dim3(IB), 0, st, boxes,
                     cap, C, count, thresh, pre_max, normal, wcap, mask);
  DFU3D_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_pp_walk, dim3((unsigned)S), dim3(PT), 0, st, (const unsigned long long *)mask, count, cap, wcap,
                     pre_max, post_max, keep, num_keep);
  DFU3D_LAUNCH_CHECK();
  return DFU3D_OK;
}

extern "C" int dfu3d_center_collect(const float *boxes, const float *scores, const int32_t *labels, const int32_t *keep,
                                    const int32_t *num_keep, int32_t n_heads, int32_t B, int32_t cap, int32_t C,
                                    const int32_t *cls_map, int32_t max_cls, int32_t out_cap, float *out_boxes,
                                    float *out_scores, int64_t *out_labels, int32_t *out_count, void *stream) {
  DFU3D_CLEAR_STALE_ERROR();
  if (!boxes || !scores || !labels || !keep || !num_keep || !cls_map || !out_boxes || !out_scores || !out_labels ||
      !out_count)
    return DFU3D_EINVAL;
  if (n_heads < 1 || B < 0 || cap < 0 || C < 1 || max_cls < 1 || out_cap < 0) return DFU3D_EINVAL;
  if (n_heads > 65535 || (int64_t)cap * C > 0x7FFFFFFF || (int64_t)out_cap * C > 0x7FFFFFFF) return DFU3D_ERANGE;
  if (B == 0) return DFU3D_OK;
  hipLaunchKernelGGL(k_pp_collect, dim3((unsigned)B, (unsigned)n_heads), dim3(PT), 0, (hipStream_t)stream, boxes, scores,
                     labels, keep, num_keep, n_heads, B, cap, C, cls_map, max_cls, out_cap, out_boxes, out_scores,
                     (long long *)out_labels, out_count);
  DFU3D_LAUNCH_CHECK();
  return DFU3D_OK;
}
