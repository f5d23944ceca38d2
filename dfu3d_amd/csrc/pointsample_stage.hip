// pointsample_stage.hip -- SURVEY.md §8 row f-18: DataProcessor.sample_points for a whole batch (csrc/dfu3d_smp.h): per
// scene a cloud of exactly K rows out of n, the far rows kept, in a shuffled order, in three launches and without a read
// from the device.
//
// What it stands in for: per scene np.linalg.norm, two np.where, np.random.choice without replacement (a permutation of
// all n rows on the host), a concatenation, np.random.shuffle and a fancy-indexed copy.
//
//   k_smp_order   one workgroup of 1024 threads per scene sorts its K shuffle words: the stable radix sort of
//                 block_sort.hpp, (ord, slot).
//   k_smp_list    one workgroup of 1024 threads per scene makes its list L (THE RULE of the header): the scene's first row
//                 is the sum of the counts before it; for n > K one sweep computes the far flags (a byte per row in the
//                 scratch) and F; the "m smallest by (sel, row)" of every branch is ONE radix select (block_select of
//                 common.hpp) of the m-th key -- 40 bits: the far flag above the word where the far rows are kept
//                 anyway, so that the select runs among the near rows -- and one ordered compaction: a row is taken when
//                 its key is below the selected one, or equal to it and among the first rank + 1 such rows; both counts
//                 ride in one workgroup scan per 1024 rows.  No sort of the n rows, and n has no cap.
//                 (One kernel for both, 2 B workgroups side by side, is one launch less, but its scalar registers spill:
//                 the sort alone takes 104 of them.)
//   k_smp_gather  a thread per output element: out[b * K + t] = (b, row L[order[t]] of the scene), zeros for an empty scene.
//
// A bad count table (DFU3D_SMP_BAD_COUNT) reads nothing outside `points`: a scene is cut at R.  What the gather reads
// from the scratch is clamped, so that no content of it can lead outside the input.
#include "common.hpp"
#include "block_sort.hpp"
#include "dfu3d_smp.h"

namespace {

constexpr int PT = DFU3D_SMP_SCENE_THREADS;             // threads of k_smp_order and of k_smp_list
constexpr int PW = PT / 64;                             // its waves
constexpr int GT = DFU3D_SMP_GATHER_THREADS;            // threads of k_smp_gather
static_assert(PT % 64 == 0 && PT <= 65535, "k_smp_list: two counts of a sweep share one int of the scan");

// THE layout of the scratch of dfu3d_sample_points; the size is its last field
struct SmpScratch {
  size_t far;                                           // uint8 (R), rounded up to 16
  size_t key0, idx0, key1, idx1;                        // uint32 / int32 (B, K) each: the sort's two buffers
  size_t order, list;                                   // int32 (B, K) each
  size_t first, rows;                                   // int32 (B) each
  size_t bytes;
};

SmpScratch smp_scratch(int B, int R, int K) {
  SmpScratch s;
  size_t o = 0;
  const size_t plane = (size_t)B * K * sizeof(uint32_t);
  s.far = o; o += ((size_t)R + 15) / 16 * 16;
  s.key0 = o; o += plane;
  s.idx0 = o; o += plane;
  s.key1 = o; o += plane;
  s.idx1 = o; o += plane;
  s.order = o; o += plane;
  s.list = o; o += plane;
  s.first = o; o += (size_t)B * sizeof(int32_t);
  s.rows = o; o += (size_t)B * sizeof(int32_t);
  s.bytes = (o + 15) / 16 * 16;
  return s;
}

// THE RULE's depth test: every product and sum rounded on its own, the square root correctly rounded; NaN is not near
__device__ __forceinline__ bool smp_far(const float *__restrict__ row) {
  const float x = row[1], y = row[2], z = row[3];
  const float d = __fsqrt_rn(__fadd_rn(__fadd_rn(__fmul_rn(x, x), __fmul_rn(y, y)), __fmul_rn(z, z)));
  return !(d < 40.0f);
}

__global__ __launch_bounds__(PT) void k_smp_order(int K, const uint32_t *__restrict__ ord, uint32_t *key0, int *idx0,
                                                  uint32_t *key1, int *idx1, int *order) {
  __shared__ int s_cnt[256 * PW];
  __shared__ int s_w[PW];
  const size_t o = (size_t)blockIdx.x * K;
  const uint32_t *words = ord + o;
  block_radix_sort<PT>(K, K, [&](int i) { return words[i]; }, key0 + o, idx0 + o, key1 + o, idx1 + o, order + o, s_cnt, s_w);
}

__global__ __launch_bounds__(PT) void k_smp_list(const float *__restrict__ points, const int *__restrict__ point_cnt,
                                                 int R, int C, int K, const uint32_t *__restrict__ sel,
                                                 const uint32_t *__restrict__ rep, uint8_t *far, int *list, int *first,
                                                 int *rows, int *status) {
  __shared__ unsigned long long s_sum[PW];
  __shared__ unsigned long long s_sel[3];
  __shared__ int s_hist[256];
  __shared__ int s_w[PW];
  __shared__ int s_bad;
  const int t = threadIdx.x, b = blockIdx.x;
  // the scene's first row: the counts before it (a negative one counts 0)
  if (t == 0) s_bad = 0;
  __syncthreads();
  unsigned long long before = 0ull;
  for (int i = t; i < b; i += PT) {
    const int c = point_cnt[i];
    if (c < 0) atomicOr(&s_bad, 1);
    before += (unsigned long long)(c < 0 ? 0 : c);
  }
  before = wave_sum_u64(before);
  if ((t & 63) == 0) s_sum[t >> 6] = before;
  __syncthreads();
  before = 0ull;
#pragma unroll
  for (int w = 0; w < PW; w++) before += s_sum[w];
  const int own = point_cnt[b];
  const int start = (int)(before < (unsigned long long)R ? before : (unsigned long long)R);
  const int n = min(max(own, 0), R - start);
  int word = (s_bad || own < 0 || before + (unsigned long long)max(own, 0) > (unsigned long long)R) ? DFU3D_SMP_BAD_COUNT : 0;
  if (n == 0) word |= DFU3D_SMP_EMPTY_SCENE;
  if (t == 0) {
    first[b] = start;
    rows[b] = n;
    if (word) atomicOr(status, word);
  }
  int *L = list + (size_t)b * K;
  if (n == 0) {                                             // (uniform, as every branch below)
    for (int j = t; j < K; j += PT) L[j] = -1;
    return;
  }
  const int head = n > K ? 0 : n;                           // rows 0 .. head - 1 come first, as they are
  for (int j = t; j < head; j += PT) L[j] = j;
  const int m = K - head;                                   // rows still to choose
  if (m == 0) return;
  if (m > n) {                                              // K > 2n: with replacement
    const uint32_t *words = rep + (size_t)b * K;
    for (int j = t; j < m; j += PT) L[head + j] = (int)(((unsigned long long)words[j] * (unsigned long long)n) >> 32);
    return;
  }
  // the m smallest by (sel, row) in ascending row order; with n > K and fewer than K far rows, all far rows and the
  // K - F smallest near ones.  Every sweep below gives row i to thread i % PT: a thread reads back its own far flags.
  const uint32_t *words = sel + start;
  uint8_t *flag = far + start;
  bool split = false;
  int need = m;
  if (n > K) {
    int mine = 0;
    for (int i = t; i < n; i += PT) {
      const bool f = smp_far(points + (size_t)(start + i) * (1 + C));
      flag[i] = f ? 1 : 0;
      mine += f ? 1 : 0;
    }
    const int F = block_sum_i<PW>(mine, s_w);               // (s_w is next written behind block_select's barriers)
    split = F < K;
    if (split) need = K - F;
  }
  auto keyfn = [&](int i) {
    return ((unsigned long long)(split ? flag[i] : 0) << 32) | (unsigned long long)words[i];
  };
  const Selected<unsigned long long> cut = block_select<PT, 40, unsigned long long>(n, need - 1, keyfn, s_hist, s_sel);
  int run_lt = 0, run_eq = 0;                               // rows taken for good / rows with the cut's key, so far
  for (int base = 0; base < n; base += PT) {
    const int i = base + t;
    bool lt = false, eq = false;
    if (i < n) {
      const unsigned long long key = keyfn(i);
      lt = key < cut.key || (key >> 32) != 0ull;            // (a far row's key lies above the cut: the cut is a near row's)
      eq = key == cut.key;
    }
    int tot;
    const int ex = block_excl_scan<PW>((lt ? 1 : 0) | (eq ? 1 << 16 : 0), s_w, tot);
    const int eq_rank = run_eq + (ex >> 16);
    if (lt || (eq && eq_rank <= cut.rank)) {
      const int pos = run_lt + (ex & 0xFFFF) + min(eq_rank, cut.rank + 1);
      if ((unsigned)pos < (unsigned)m) L[head + pos] = i;   // (never beyond it)
    }
    run_lt += tot & 0xFFFF;
    run_eq += tot >> 16;
  }
}

__global__ __launch_bounds__(GT) void k_smp_gather(const uint32_t *__restrict__ points, int C, int K, int out_cols,
                                                   const int *__restrict__ order, const int *__restrict__ list,
                                                   const int *__restrict__ first, const int *__restrict__ rows,
                                                   uint32_t *__restrict__ out, long long total) {
  const long long e = (long long)blockIdx.x * GT + threadIdx.x;
  if (e >= total) return;
  const int W = 1 + out_cols;
  const long long r = e / W;
  const int c = (int)(e - r * W), b = (int)(r / K);
  uint32_t v = 0u;
  if (c == 0) {
    v = __float_as_uint((float)b);
  } else {
    const int n = rows[b];
    const int slot = min(max(order[r], 0), K - 1);
    const int l = min(list[(size_t)b * K + slot], n - 1);
    if (l >= 0) v = points[(size_t)(first[b] + l) * (1 + C) + c];
  }
  out[e] = v;
}

bool smp_sizes_ok(int B, int R, int K) {
  return B >= 0 && R >= 0 && K >= 1 && K <= DFU3D_SMP_MAX_OUT && B <= DFU3D_SMP_MAX_BATCH;
}

}  // namespace

static_assert(DFU3D_SMP_LAUNCHES == 3, "k_smp_order, k_smp_list, k_smp_gather");

extern "C" int32_t dfu3d_smp_version(void) { return DFU3D_SMP_VERSION; }

extern "C" size_t dfu3d_smp_scratch_bytes(int32_t B, int32_t R, int32_t K) {
  if (!smp_sizes_ok(B, R, K) || B == 0) return 0;
  return smp_scratch(B, R, K).bytes;
}

extern "C" int dfu3d_sample_points(const float *points, const int32_t *point_cnt, int32_t B, int32_t R, int32_t C,
                                   int32_t K, int32_t out_cols, const int32_t *sel, const int32_t *ord,
                                   const int32_t *rep, void *scratch, size_t scratch_bytes, float *out, int32_t *status,
                                   void *stream) {
  DFU3D_CLEAR_STALE_ERROR();
  if (!point_cnt || !ord || !rep || !scratch || !out || !status) return DFU3D_EINVAL;
  if (B < 0 || R < 0 || K < 1 || C < 3 || out_cols < 3 || out_cols > C) return DFU3D_EINVAL;
  if (R > 0 && (!points || !sel)) return DFU3D_EINVAL;
  if (K > DFU3D_SMP_MAX_OUT || B > DFU3D_SMP_MAX_BATCH) return DFU3D_ERANGE;
  if ((int64_t)R * (1 + (int64_t)C) > (int64_t)DFU3D_SMP_MAX_ELEMS) return DFU3D_ERANGE;
  if ((int64_t)B * K * (1 + (int64_t)out_cols) > (int64_t)DFU3D_SMP_MAX_ELEMS) return DFU3D_ERANGE;
  if (B == 0) return DFU3D_OK;
  const SmpScratch S = smp_scratch(B, R, K);
  if (((uintptr_t)scratch & 15u) || scratch_bytes < S.bytes) return DFU3D_EINVAL;
  char *base = (char *)scratch;
  hipStream_t st = (hipStream_t)stream;
  int *order = (int *)(base + S.order), *list = (int *)(base + S.list);
  int *first = (int *)(base + S.first), *rows = (int *)(base + S.rows);
  hipLaunchKernelGGL(k_smp_order, dim3((unsigned)B), dim3(PT), 0, st, K, (const uint32_t *)ord,
                     (uint32_t *)(base + S.key0), (int *)(base + S.idx0), (uint32_t *)(base + S.key1),
                     (int *)(base + S.idx1), order);
  DFU3D_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_smp_list, dim3((unsigned)B), dim3(PT), 0, st, points, (const int *)point_cnt, R, C, K,
                     (const uint32_t *)sel, (const uint32_t *)rep, (uint8_t *)(base + S.far), list, first, rows,
                     (int *)status);
  DFU3D_LAUNCH_CHECK();
  const long long total = (long long)B * K * (1 + out_cols);
  hipLaunchKernelGGL(k_smp_gather, dim3((unsigned)((total + GT - 1) / GT)), dim3(GT), 0, st, (const uint32_t *)points, C,
                     K, out_cols, (const int *)order, (const int *)list, (const int *)first, (const int *)rows,
                     (uint32_t *)out, total);
  DFU3D_LAUNCH_CHECK();
  return DFU3D_OK;
}
