// pn2_device.hpp -- device functions shared by the batched PointNet++ ops (pointnet2_stage.hip, k_pn_*) and the
// stacked ones (pointstack_stage.hip, k_stk_*): the squared distance of dfu3d_pn2.h, the two forms of one farthest
// point sampling step, and the hits of one 64-point tile of a ball query.  ONE statement of each, so both stages give
// the same picks and the same indices.  Everything here wants wave-uniform control flow (ballots, DPP reductions).
#pragma once
#include "common.hpp"

namespace pn2 {

__device__ __forceinline__ float sqdist(float ax, float ay, float az, float bx, float by, float bz) {
  return (ax - bx) * (ax - bx) + (ay - by) * (ay - by) + (az - bz) * (az - bz);
}
__device__ __forceinline__ int wave_max_i(int v) { return ~wave_min_i_dpp(~v); }
__device__ __forceinline__ void status_or(uint32_t st, uint32_t *__restrict__ status) {   // all lanes of the wave call it
  st = wave_or_u32_dpp(st);
  if (lane_id() == 0 && st) atomicOr(status, st);
}
__device__ __forceinline__ bool finite3(float x, float y, float z) { return isfinite(x) && isfinite(y) && isfinite(z); }

// ---- farthest point sampling ------------------------------------------------------------------------------------------
// The workgroup's pick of a step from the waves' picks (wave-uniform wkey, widx, wx, wy, wz; waves own ascending runs of
// points, so among equal keys the lowest wave holds the lowest index).  One barrier; the slot alternates with `par`, so
// a wave that is a step ahead writes the other slot.
template <int NW>
__device__ __forceinline__ void fps_exchange(int4 (*s_a)[NW], float (*s_z)[NW], int par, int wkey, int widx, float wx,
                                             float wy, float wz, int &old, float &x1, float &y1, float &z1) {
  const int lane = lane_id(), w = threadIdx.x >> 6;
  if (lane == 0) {
    s_a[par][w] = make_int4(wkey, widx, __float_as_int(wx), __float_as_int(wy));
    s_z[par][w] = wz;
  }
  __syncthreads();
  const int4 e = s_a[par][lane & (NW - 1)];
  const float ez = s_z[par][lane & (NW - 1)];
  const int bkey = wave_max_i(e.x);
  const int wsel = __ffsll((unsigned long long)__ballot(e.x == bkey)) - 1;   // < NW: lane l < NW holds wave l's
  old = __builtin_amdgcn_readlane(e.y, wsel);
  x1 = __int_as_float(__builtin_amdgcn_readlane(e.z, wsel));
  y1 = __int_as_float(__builtin_amdgcn_readlane(e.w, wsel));
  z1 = readlane_f(ez, wsel);
}

// The register form: thread t keeps the PT consecutive points t * PT .. of p (rows of `stride` floats, n of them) and
// their running minima.  fps_load fills them and says whether a coordinate of the thread's is not finite.
template <int PT>
__device__ __forceinline__ bool fps_load(const float *__restrict__ p, int stride, int n, float (&px)[PT], float (&py)[PT],
                                         float (&pz)[PT], float (&pm)[PT]) {
  bool bad = false;
#pragma unroll
  for (int j = 0; j < PT; j++) {
    const int k = threadIdx.x * PT + j;
    if (k < n) {
      px[j] = p[k * stride + 0];
      py[j] = p[k * stride + 1];
      pz[j] = p[k * stride + 2];
      pm[j] = 1e10f;
      if (!finite3(px[j], py[j], pz[j])) bad = true;
    } else {                                         // no point: a negative minimum never becomes a maximum
      px[j] = py[j] = pz[j] = 0.0f;
      pm[j] = -1.0f;
    }
  }
  return bad;
}

// One step: the minima against the last pick (x1, y1, z1), the thread's best (key = the bits of the running minimum, a
// non-negative float, so integer order = float order), the wave's, the workgroup's -> old, x1, y1, z1.
template <int NW, int PT>
__device__ __forceinline__ void fps_step_reg(const float (&px)[PT], const float (&py)[PT], const float (&pz)[PT],
                                             float (&pm)[PT], int4 (*s_a)[NW], float (*s_z)[NW], int par, int &old,
                                             float &x1, float &y1, float &z1) {
  int key = -1, bj = 0;
#pragma unroll
  for (int j = 0; j < PT; j++) {
    const float d = sqdist(px[j], py[j], pz[j], x1, y1, z1);
    float m = pm[j];
    m = d < m ? d : m;                               // a NaN distance leaves the minimum
    pm[j] = m;
    const int kj = __float_as_int(m);
    if (kj > key) {                                  // strict: the lowest index of the thread among equals
      key = kj;
      bj = j;
    }
  }
  const int wkey = wave_max_i(key);
  const int src = __ffsll((unsigned long long)__ballot(key == wkey)) - 1;
  const int jsel = __builtin_amdgcn_readlane(bj, src);
  float wx = 0.0f, wy = 0.0f, wz = 0.0f;
#pragma unroll
  for (int j = 0; j < PT; j++) {
    if (j == jsel) {                                 // wave-uniform
      wx = readlane_f(px[j], src);
      wy = readlane_f(py[j], src);
      wz = readlane_f(pz[j], src);
    }
  }
  const int widx = (((int)threadIdx.x & ~63) + src) * PT + jsel;   // >= n only with wkey < 0, which no workgroup picks
  fps_exchange<NW>(s_a, s_z, par, wkey, widx, wx, wy, wz, old, x1, y1, z1);
}

// The memory form: the running minima live in pm (one float per point), the coordinates are read every step; the wave
// owns the points lo .. hi, its lanes stride them.  `first`: the minima start at 1e10f and pm is not read; the
// coordinates are looked at and `bad` is set for one that is not finite.
template <int NW>
__device__ __forceinline__ void fps_step_mem(const float *__restrict__ p, int stride, float *__restrict__ pm, int lo, int hi,
                                             bool first, bool &bad, int4 (*s_a)[NW], float (*s_z)[NW], int par, int &old,
                                             float &x1, float &y1, float &z1) {
  const int lane = lane_id();
  int key = -1, bi = 0;
  float bx = 0.0f, by = 0.0f, bz = 0.0f;
  for (int k = lo + lane; k < hi; k += 64) {
    const float x = p[k * stride + 0], y = p[k * stride + 1], z = p[k * stride + 2];
    float m = 1e10f;
    if (first) {
      if (!finite3(x, y, z)) bad = true;
    } else {
      m = pm[k];
    }
    const float d = sqdist(x, y, z, x1, y1, z1);
    m = d < m ? d : m;
    pm[k] = m;
    const int kj = m >= 0.0f ? __float_as_int(m) : 0;      // (a scratch the caller overwrote cannot leave the range)
    if (kj > key) {
      key = kj;
      bi = k;
      bx = x;
      by = y;
      bz = z;
    }
  }
  const int wkey = wave_max_i(key);
  const int widx = wave_min_i_dpp(key == wkey ? bi : 0x7FFFFFFF);
  const int src = __ffsll((unsigned long long)__ballot(key == wkey && bi == widx)) - 1;
  fps_exchange<NW>(s_a, s_z, par, wkey, widx, readlane_f(bx, src), readlane_f(by, src), readlane_f(bz, src), old, x1, y1,
                   z1);
}

// ---- ball query -------------------------------------------------------------------------------------------------------
// the hits of one 64-point tile for one scale; wave-uniform control flow
__device__ __forceinline__ void ball_take(bool hit, int k, int tile0, int nsample, int *__restrict__ o, int &cnt, int &first,
                                          bool &full) {
  const unsigned long long m = __ballot(hit);
  if (!m) return;
  if (cnt == 0) first = tile0 + __ffsll(m) - 1;
  const int rank = cnt + __popcll(m & ((1ull << lane_id()) - 1ull));
  if (hit && rank < nsample) o[rank] = k;
  cnt += __popcll(m);
  full = cnt >= nsample;
}

}  // namespace pn2
