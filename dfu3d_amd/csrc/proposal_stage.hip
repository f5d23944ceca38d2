// proposal_stage.hip -- SURVEY.md §8 row f-17: PointRCNN's proposal stage for a whole batch (csrc/dfu3d_prop.h): the
// NMS_PRE_MAXSIZE best points of every sample by score, their rotated NMS cut at NMS_POST_MAXSIZE, and the padded RoI
// block, in two launches and without a read from the device.
//
// What it stands in for: the per-sample loop of PointRCNNHead.proposal_layer over class_agnostic_nms -- torch.topk, an
// argsort of the sorted scores, a gather of the box rows, the whole upper triangle of the pre_max x pre_max decision
// matrix (k_suppress_mask), one wave walking all of its rows (k_nms_reduce), a read of the count, four index assignments.
//
//   k_pr_order   one workgroup of 1024 threads per sample: the stable radix sort of block_sort.hpp, of (key, point index)
//                under THE ORDER RULE of dfu3d_prop.h (the key here is the rule's key inverted, so ascending = best
//                first).  Pass 0 reads the scores, the passes between alternate between two buffers in the caller's
//                scratch, pass 3 writes the first K indices.  Equal keys never change places: ascending point index
//                among them.
//   k_pr_nms     one workgroup of IB = 256 threads per sample.  A row is suppressed only by a KEPT earlier row and at most
//                post_max rows are kept, so the kept boxes live in LDS as Rects (make_rect's sincosf once per box, not
//                once per pair) and the candidates are taken 64 at a time, read through `order`:
//                  1. every candidate (one per lane, the same in all four waves) against the kept list, 40 kept boxes a
//                     phase, dealt out over the waves: the circle test of overlap_area for every pair, the pairs it
//                     leaves queued in LDS; as soon as 256 are queued, and after the last phase, they are clipped on
//                     full waves and the hits OR-ed into one LDS word (a candidate already hit queues nothing more);
//                  2. the 64 x 64 diagonal words (bit c of row r: r suppresses c > r) the same way, only for rows and
//                     columns still standing;
//                  3. the greedy chain inside the block on wave-uniform values, the inner loop of k_pp_walk (every wave
//                     runs it: nobody waits for a broadcast), stopped at post_max;
//                  4. wave 0 appends the kept Rects and writes their point indices.
//                It stops at K or as soon as post_max are kept; the tail writes every other element of the five outputs.
//                Every pair is decided by nms_suppresses(A, B) with the EARLIER row as A, as in k_suppress_mask and
//                k_pp_mask: the same bits (a pair the circle test removes has overlap 0 there as here).
#include "common.hpp"
#include "block_sort.hpp"
#include "rect_overlap.hpp"
#include "dfu3d_prop.h"

namespace {

constexpr int OT = DFU3D_PROP_SORT_THREADS;             // threads of k_pr_order
constexpr int OW = OT / 64;                             // its waves
constexpr int PR_CAND = DFU3D_PROP_BLOCK_ROWS;          // candidates of a block of k_pr_nms: one per lane
constexpr int PR_CHUNK = 40;                            // kept boxes of one phase of step 1: it queues PR_CHUNK * PR_CAND pairs at most
constexpr int PR_QUEUE = DFU3D_PROP_QUEUE_PAIRS;        // pairs the queue holds: what is left of 64 KiB of LDS (the diagonal's
                                                        // phase queues 63 * 64 / 2 at most)
// (fewer than IB entries stay pending after a phase: IB - 1 + PR_CHUNK * PR_CAND fit)
static_assert(IB == 256 && PR_CHUNK % (IB / 64) == 0 && PR_CAND == 64 && IB - 1 + PR_CHUNK * PR_CAND <= PR_QUEUE &&
              PR_QUEUE >= PR_CAND * (PR_CAND - 1) / 2 && DFU3D_PROP_MAX_POST * PR_CAND <= 65536, "k_pr_nms");

// THE layout of the scratch of dfu3d_proposals; the size is its last field
struct PrScratch {
  size_t key0, idx0, key1, idx1;                        // uint32 / int32 (B, N) each: the sort's two buffers
  size_t order;                                         // int32 (B, K)
  size_t bytes;
};

PrScratch pr_scratch(int B, int N, int K) {
  PrScratch s;
  size_t o = 0;
  const size_t plane = (size_t)B * N * sizeof(uint32_t);
  s.key0 = o; o += plane;
  s.idx0 = o; o += plane;
  s.key1 = o; o += plane;
  s.idx1 = o; o += plane;
  s.order = o; o += (size_t)B * K * sizeof(int32_t);
  s.bytes = (o + 15) / 16 * 16;
  return s;
}

// THE ORDER RULE's key, inverted: ascending = best first (a NaN first of all, then +inf)
__device__ __forceinline__ uint32_t pr_sort_key(float s) {
  uint32_t u = __float_as_uint(s);
  if ((u & 0x7FFFFFFFu) > 0x7F800000u) return 0u;       // every NaN: key 0xFFFFFFFF
  if (u == 0x80000000u) u = 0u;                         // -0.0 is +0.0
  const uint32_t key = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
  return ~key;
}

__global__ __launch_bounds__(OT) void k_pr_order(const float *__restrict__ scores, int N, int K, uint32_t *key0,
                                                 int *idx0, uint32_t *key1, int *idx1, int *order) {
  __shared__ int s_cnt[256 * OW];
  __shared__ int s_w[OW];
  const int b = blockIdx.x;
  const size_t o = (size_t)b * N;
  const float *sc = scores + o;
  block_radix_sort<OT>(N, K, [&](int i) { return pr_sort_key(sc[i]); }, key0 + o, idx0 + o, key1 + o, idx1 + o,
                       order + (size_t)b * K, s_cnt, s_w);
}

// The pairs that need the polygon clip, queued in LDS so that the clips run on full waves.  With a pair per lane and the
// circle test in front, the few lanes whose circles meet held their whole wave in the clipper at almost every step; with
// a queue emptied after every chunk of kept boxes, most clip rounds ran on a quarter of the threads (both measured:
// DESIGN.md row f-17).  An entry is (a << 6) | c: candidate c of the block against row a (a kept box, or a candidate of
// the block).  Pushes go through one of two counters that are never reset and take turns from phase to phase: the
// counter of a phase is read after the barrier that ends it and next changed two phases on, so a read never races.
//
// pr_push: bit j of flags: this lane queues (a0 + j * step, c).  One scan and one LDS atomic per wave and call.
// PRECONDITION: all 64 lanes, wave-uniform control flow (wave_incl_scan).  off: the counter's value at the start of the
// phase minus the entries already pending.
template <int NJ>
__device__ __forceinline__ void pr_push(unsigned short *item, int *count, int off, unsigned flags, int a0, int step, int c) {
  const int mine = __popc(flags);
  const int incl = wave_incl_scan(mine);
  const int total = readlane_i(incl, 63);
  if (total == 0) return;                                   // uniform
  int base = 0;
  if (lane_id() == 0) base = atomicAdd(count, total);
  int at = readlane_i(base, 0) - off + incl - mine;
#pragma unroll
  for (int j = 0; j < NJ; j++) {
    if ((flags >> j) & 1u) {
      if ((unsigned)at < (unsigned)PR_QUEUE) item[at] = (unsigned short)(((a0 + j * step) << 6) | c);   // (never beyond it)
      at++;
    }
  }
}

__global__ __launch_bounds__(IB) void k_pr_nms(const float *__restrict__ scores, const long long *__restrict__ labels,
                                               const float *__restrict__ boxes, int N, int C, int K, float thresh,
                                               int post_max, const int *__restrict__ order, float *__restrict__ rois,
                                               float *__restrict__ roi_scores, long long *__restrict__ roi_labels,
                                               long long *roi_point_idx, int *__restrict__ num_rois) {
  __shared__ float s_poly[4][MAXV * IB];
  __shared__ Rect s_kept[DFU3D_PROP_MAX_POST];
  __shared__ Rect s_cand[PR_CAND];
  __shared__ int s_cpos[PR_CAND];
  __shared__ unsigned long long s_diag[PR_CAND];
  __shared__ unsigned short s_item[PR_QUEUE];
  __shared__ unsigned long long s_gone;
  __shared__ int s_count[2];
  const int b = blockIdx.x, t = threadIdx.x, w = t >> 6, lane = t & 63;
  float *pu = s_poly[0] + t, *pv = s_poly[1] + t, *qu = s_poly[2] + t, *qv = s_poly[3] + t;
  const float *bx = boxes + (size_t)b * N * C;
  const int *ord = order + (size_t)b * K;
  const size_t ro = (size_t)b * post_max;
  volatile unsigned long long *gone_now = &s_gone;
  volatile int *count_now = s_count;
  if (t < 2) s_count[t] = 0;
  int nk = 0;                                                // kept so far
  int seen0 = 0, seen1 = 0, turn = 0, pend = 0;              // the counters as last read, whose turn it is, entries queued
  // (all five are uniform over the workgroup)
  for (int c0 = 0; c0 < K && nk < post_max; c0 += PR_CAND) {
    const int nc = min(PR_CAND, K - c0);
    if (t < PR_CAND) {
      Rect r = {0.0f, 0.0f, 0.0f, 0.0f, 1.0f, 0.0f};
      int p = -1;
      if (t < nc) {
        p = min(max(ord[c0 + t], 0), N - 1);
        r = make_rect(bx + (size_t)p * C, 7);
      }
      s_cand[t] = r;
      s_cpos[t] = p;
      s_diag[t] = 0ull;
      if (t == 0) s_gone = nc < PR_CAND ? ~0ull << nc : 0ull;      // bit set: suppressed, or beyond the last candidate
    }
    __syncthreads();
    const Rect me = s_cand[lane];
    // 1. against the kept list, PR_CHUNK kept boxes a phase; kept box a is the earlier row.  Under a negative threshold
    // a pair with overlap 0 suppresses too, so every pair is queued and nms_suppresses says so itself.
    const bool every_pair = thresh < 0.0f;
    for (int k0 = 0; k0 < nk; k0 += PR_CHUNK) {
      const unsigned long long gone = *gone_now;             // (uniform: it changes between two barriers of a flush only)
      if (gone == ~0ull) {                                   // nothing left to decide in this block
        pend = 0;
        break;
      }
      const bool live = !((gone >> lane) & 1ull);
      unsigned flags = 0u;
#pragma unroll
      for (int j = 0; j < PR_CHUNK / (IB / 64); j++) {
        const int a = k0 + j * (IB / 64) + w;
        if (live && a < nk) {
          const Rect A = s_kept[a];
          if (every_pair || !circles_apart(A, me)) flags |= 1u << j;
        }
      }
      pr_push<PR_CHUNK / (IB / 64)>(s_item, s_count + turn, (turn ? seen1 : seen0) - pend, flags, k0 + w, IB / 64, lane);
      __syncthreads();
      const int now = count_now[turn];
      pend += now - (turn ? seen1 : seen0);
      if (turn) seen1 = now; else seen0 = now;
      turn ^= 1;
      const bool last = k0 + PR_CHUNK >= nk;
      if (pend >= IB || last) {
        // full rounds only, so that what they find spares the later phases their work; everything after the last phase
        const int full = last ? pend : pend / IB * IB;
        for (int q = t; q < full; q += IB) {
          const int item = s_item[q], a = item >> 6, c = item & 63;
          if ((*gone_now >> c) & 1ull) continue;             // (a hit another thread has found meanwhile: the same result)
          const Rect A = s_kept[a], Bc = s_cand[c];
          if (nms_suppresses(A, Bc, 0, thresh, pu, pv, qu, qv)) atomicOr(&s_gone, 1ull << c);
        }
        // the rest moves to the front: slot t < IB <= full was read by this thread alone, in its first round
        const int rest = pend - full;
        if (t < rest) s_item[t] = s_item[full + t];
        pend = rest;
        __syncthreads();
      }
    }
    const unsigned long long gone = *gone_now;
    // 2. the diagonal words, bit c of row r: candidate r suppresses candidate c > r; only for rows and columns still standing
    {
      const bool live = !((gone >> lane) & 1ull);
      unsigned flags = 0u;
#pragma unroll 2
      for (int j = 0; j < PR_CAND / (IB / 64); j++) {
        const int r = j * (IB / 64) + w;
        if (live && r < lane && !((gone >> r) & 1ull)) {
          const Rect A = s_cand[r];
          if (every_pair || !circles_apart(A, me)) flags |= 1u << j;
        }
      }
      pr_push<PR_CAND / (IB / 64)>(s_item, s_count + turn, (turn ? seen1 : seen0) - pend, flags, w, IB / 64, lane);   // (pend is 0)
      __syncthreads();
      const int now = count_now[turn];
      pend += now - (turn ? seen1 : seen0);
      if (turn) seen1 = now; else seen0 = now;
      turn ^= 1;
      for (int q = t; q < pend; q += IB) {
        const int item = s_item[q], r = item >> 6, c = item & 63;
        const Rect A = s_cand[r], Bc = s_cand[c];
        if (nms_suppresses(A, Bc, 0, thresh, pu, pv, qu, qv)) atomicOr(&s_diag[r], 1ull << c);
      }
      pend = 0;
      __syncthreads();
    }
    // 3. the chain inside the block, in every wave
    const unsigned long long diag = s_diag[lane];
    unsigned long long cur = gone, kept = 0ull;
    int add = 0;
    while (~cur != 0ull && nk + add < post_max) {
      const int f = __ffsll((long long)~cur) - 1;
      kept |= 1ull << f;
      add++;
      cur |= readlane_u64(diag, f) | (1ull << f);
    }
    // 4. the kept Rects to the list; their points straight to roi_point_idx, where the tail finds them
    if (w == 0 && ((kept >> lane) & 1ull)) {
      const int at = nk + __popcll(kept & ((1ull << lane) - 1ull));      // < post_max
      s_kept[at] = me;
      roi_point_idx[ro + at] = (long long)s_cpos[lane];
    }
    nk += add;
    __syncthreads();                                          // (orders the stores to roi_point_idx before the tail's loads, too)
  }
  // eight threads a row, 32 rows a sweep: the row's point is read once, its columns are dealt out over the eight
  const int g = t >> 3, l = t & 7;
  for (int r = g; r < post_max; r += IB / 8) {
    float *orow = rois + (ro + r) * C;
    if (r < nk) {
      const int p = min(max((int)roi_point_idx[ro + r], 0), N - 1);
      const float *irow = bx + (size_t)p * C;
      for (int c = l; c < C; c += 8) orow[c] = irow[c];
      if (l == 0) {
        roi_scores[ro + r] = scores[(size_t)b * N + p];
        roi_labels[ro + r] = labels[(size_t)b * N + p] + 1ll;
      }
    } else {
      for (int c = l; c < C; c += 8) orow[c] = 0.0f;
      if (l == 0) {
        roi_scores[ro + r] = 0.0f;
        roi_labels[ro + r] = 1ll;
        roi_point_idx[ro + r] = -1ll;
      }
    }
  }
  if (t == 0) num_rois[b] = nk;
}

bool pr_sizes_ok(int B, int N, int pre_max) {
  return B >= 0 && N >= 0 && pre_max >= 1 && N <= DFU3D_PROP_MAX_POINTS && B <= DFU3D_PROP_MAX_BATCH;
}

}  // namespace

static_assert(DFU3D_PROP_LAUNCHES == 2, "k_pr_order, k_pr_nms");

extern "C" int32_t dfu3d_prop_version(void) { return DFU3D_PROP_VERSION; }

extern "C" size_t dfu3d_prop_scratch_bytes(int32_t B, int32_t N, int32_t pre_max) {
  if (!pr_sizes_ok(B, N, pre_max)) return 0;
  return pr_scratch(B, N, pre_max < N ? pre_max : N).bytes;
}

extern "C" int dfu3d_proposals(const float *scores, const int64_t *labels, const float *boxes, int32_t B, int32_t N,
                               int32_t C, float thresh, int32_t pre_max, int32_t post_max, void *scratch,
                               size_t scratch_bytes, float *rois, float *roi_scores, int64_t *roi_labels,
                               int64_t *roi_point_idx, int32_t *num_rois, void *stream) {
  DFU3D_CLEAR_STALE_ERROR();
  if (!scores || !labels || !boxes || !scratch || !rois || !roi_scores || !roi_labels || !roi_point_idx || !num_rois)
    return DFU3D_EINVAL;
  if (B < 0 || N < 0 || C < 7 || pre_max < 1) return DFU3D_EINVAL;
  if (post_max < 1 || post_max > DFU3D_PROP_MAX_POST) return DFU3D_ERANGE;
  if (N > DFU3D_PROP_MAX_POINTS || B > DFU3D_PROP_MAX_BATCH) return DFU3D_ERANGE;
  if ((int64_t)B * N * C > (int64_t)DFU3D_PROP_MAX_ELEMS) return DFU3D_ERANGE;
  if ((int64_t)(B > 0 ? B : 1) * post_max * C > (int64_t)DFU3D_PROP_MAX_ELEMS) return DFU3D_ERANGE;
  if (B == 0 || N == 0) return DFU3D_OK;
  const int K = pre_max < N ? pre_max : N;
  const PrScratch L = pr_scratch(B, N, K);
  if (((uintptr_t)scratch & 15u) || scratch_bytes < L.bytes) return DFU3D_EINVAL;
  char *base = (char *)scratch;
  int *order = (int *)(base + L.order);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(k_pr_order, dim3((unsigned)B), dim3(OT), 0, st, scores, N, K, (uint32_t *)(base + L.key0),
                     (int *)(base + L.idx0), (uint32_t *)(base + L.key1), (int *)(base + L.idx1), order);
  DFU3D_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_pr_nms, dim3((unsigned)B), dim3(IB), 0, st, scores, (const long long *)labels, boxes, N, C, K,
                     thresh, post_max, (const int *)order, rois, roi_scores, (long long *)roi_labels,
                     (long long *)roi_point_idx, num_rois);
  DFU3D_LAUNCH_CHECK();
  return DFU3D_OK;
}
