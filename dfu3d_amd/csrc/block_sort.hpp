// block_sort.hpp -- the workgroup radix sort of 32-bit keys: k_pr_order (proposal_stage.hip) sorts a sample's scores
// with it, k_sp_plan (pointsample_stage.hip) a scene's shuffle words.
//
// A stable least-significant-digit radix sort, four passes of eight bits, of (key, index) by ONE workgroup of NT
// threads.  Every wave owns a contiguous run of the array; a pass counts the digits per wave (lanes of equal digit found
// by eight ballots, the first of them adds their number: no atomics), scans the 256 x NT/64 counts digit-major with
// block_scan_range -- the start of every (digit, wave) --, and after a barrier (a wave's starts were stored by threads of
// all waves) every wave scatters its run in order, moving on its own column of starts without a further barrier.  Pass 0
// takes its keys from the caller, the passes between alternate between two buffers in global memory (128 KiB of keys
// and indices for 16 384 entries would fit the LDS only once, not twice), pass 3 writes the first K indices.  Equal keys
// never change places: ascending index among them.
#pragma once
#include "common.hpp"

// The lanes among `active` whose 8-bit digit equals this lane's (unspecified in a lane that is not active).
// PRECONDITION: wave-uniform control flow (ballots).
__device__ __forceinline__ unsigned long long wave_match8(bool active, int digit) {
  unsigned long long m = __ballot(active);
#pragma unroll
  for (int b = 0; b < 8; b++) {
    const bool bit = (digit >> b) & 1;
    const unsigned long long v = __ballot(bit);
    m &= bit ? v : ~v;
  }
  return m;
}

// One pass of the sort over the digit at `shift`.  first: the keys come from keyfn and the index is the position;
// last: only the first K indices are written, to `order`.  cnt: 256 * NT / 64 ints of LDS, s_w: NT / 64 ints.
// PRECONDITION: all threads of the workgroup, uniform control flow.
template <int NT, class KeyFn>
__device__ __forceinline__ void block_sort_pass(bool first, bool last, KeyFn keyfn, const uint32_t *src_key,
                                                const int *src_idx, uint32_t *dst_key, int *dst_idx, int *order, int N,
                                                int K, int shift, int i0, int i1, volatile int *cnt, int *s_w) {
  constexpr int NW = NT / 64;
  const int t = threadIdx.x, w = t >> 6, lane = t & 63;
  for (int i = t; i < 256 * NW; i += NT) cnt[i] = 0;
  __syncthreads();
  for (int base = i0; base < i1; base += 64) {              // uniform per wave
    const int i = base + lane;
    const bool act = i < i1;
    const uint32_t key = act ? (first ? keyfn(i) : src_key[i]) : 0u;
    const int d = (int)((key >> shift) & 255u);
    const unsigned long long m = wave_match8(act, d);
    if (act && lane == __ffsll((long long)m) - 1) cnt[d * NW + w] += __popcll(m);   // one lane per digit: no atomics
  }
  __syncthreads();
  // digit-major: the start of (digit, wave) = every smaller digit, and the same digit in the waves (= runs) before
  block_scan_range<NT, 4, int, int>(256 * NW, [&](int i) { return cnt[i]; }, [&](int i, int v) { cnt[i] = v; }, s_w);
  __syncthreads();                                          // cnt[] is read below by other threads than its writers
  for (int base = i0; base < i1; base += 64) {
    const int i = base + lane;
    const bool act = i < i1;
    const uint32_t key = act ? (first ? keyfn(i) : src_key[i]) : 0u;
    const int idx = act ? (first ? i : src_idx[i]) : 0;
    const int d = (int)((key >> shift) & 255u);
    const unsigned long long m = wave_match8(act, d);
    if (act) {
      // the wave's lanes read the start in one instruction, then the last lane of every digit moves it on: a wave's
      // LDS operations are carried out in program order
      const int start = cnt[d * NW + w];
      const int pos = start + __popcll(m & ((1ull << lane) - 1ull));
      if (last) {
        if (pos < K) order[pos] = idx;
      } else if ((unsigned)pos < (unsigned)N) {
        dst_key[pos] = key;
        dst_idx[pos] = idx;
      }
      if (lane == 63 - __clzll((long long)m)) cnt[d * NW + w] = start + __popcll(m);
    }
  }
  __syncthreads();                                          // the scattered rows are the next pass's input
}

// order[0 .. K-1] <- the indices of the K smallest of keyfn(0), ..., keyfn(N - 1), ascending by (key, index).
// key0, idx0, key1, idx1: N entries each, the buffers the passes alternate between; their content on entry does not
// matter.  cnt: 256 * NT / 64 ints of LDS, s_w: NT / 64 ints.
// PRECONDITION: all threads of the workgroup, uniform control flow, the same arguments in every thread; K <= N.
template <int NT, class KeyFn>
__device__ __forceinline__ void block_radix_sort(int N, int K, KeyFn keyfn, uint32_t *key0, int *idx0, uint32_t *key1,
                                                 int *idx1, int *order, volatile int *cnt, int *s_w) {
  const int w = threadIdx.x >> 6;
  uint32_t *ka = key0, *kb = key1;
  int *ia = idx0, *ib = idx1;
  const int run = (N + NT - 1) / NT * 64;                   // rows of a wave: a multiple of 64
  const int i0 = min(w * run, N), i1 = min(i0 + run, N);
  for (int pass = 0; pass < 4; pass++) {                    // ka -> kb -> ka -> order; pass 0 takes the caller's keys
    block_sort_pass<NT>(pass == 0, pass == 3, keyfn, kb, ib, ka, ia, order, N, K, 8 * pass, i0, i1, cnt, s_w);
    uint32_t *tk = ka; ka = kb; kb = tk;
    int *ti = ia; ia = ib; ib = ti;
  }
}
