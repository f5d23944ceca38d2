// pointnet2_stage.hip -- SURVEY.md §8 row f-14: the native ops of the PointNet++ set-abstraction / feature-propagation
// backbone (include/dfu3d_pn2.h).
//
// What it stands in for in the reference: pcdet/ops/pointnet2/pointnet2_batch (CUDA only) -- farthest point sampling,
// ball query, grouping, three nearest neighbours, three-point interpolation, and the two float-atomicAdd backward
// scatters, which are ONE ordered gather here.
//
//   k_pn_fps<NT, PT>  one workgroup per sample, PT consecutive points per thread: coordinates and running minima stay in
//                     registers for all npoint steps.  A step: the thread's best (key = the bits of the running minimum,
//                     a non-negative float, so integer order = float order), the wave's maximum by the shared DPP
//                     reduction, a ballot for its lowest lane (points are dealt out in index order, so the lowest lane
//                     holds the lowest index), the winner's coordinates by readlane, ONE LDS exchange of
//                     (key, index, x, y, z) per wave in a slot that alternates with the step's parity -- one barrier.
//   k_pn_fps_big      more points than registers hold: the running minima live in the scratch, the coordinates are read
//                     from memory every step; every wave owns a contiguous run of points, lanes stride it.  Same picks.
//   k_pn_ball         one wave per centre, all scales of the module in one walk: 256 points per trip (four coalesced
//                     loads in flight), per scale a ballot and a prefix count keep the ascending order; the walk ends
//                     when every scale is full.
//   k_pn_group        one thread per (centre, slot): the index once, then the channels; xyz - centre is the only float
//                     operation, features move as bits.
//   k_pn_three_nn     one thread per unknown point, the known points through an LDS tile (broadcast reads).
//   k_pn_interp       one thread per unknown point and chunk of channels.
//   k_pn_count / k_pn_offsets / k_pn_place / k_pn_order   the inverse of a gather as a CSR: integer atomics count and
//                     place, then a wave per source sorts its run by entry number, so the list does not depend on them.
//   k_pn_gather_bwd   one thread per source point and chunk of channels: its entries in ascending order, one float
//                     addition each, starting from +0.0f.
//   k_pn_check_batch  column 0 of the stacked points against row / points-per-sample.
#include "common.hpp"
#include "dfu3d_pn2.h"
#include "pn2_device.hpp"

#include <math.h>

namespace {

constexpr int BT = 256;                              // threads per workgroup of every kernel but k_pn_fps<1024, .>
constexpr int CCH = 16;                              // channels per workgroup of the channel-looping kernels
constexpr int FPS_BIG_NT = 1024;

using pn2::ball_take;
using pn2::sqdist;
using pn2::status_or;

// ---- farthest point sampling (the step itself: pn2_device.hpp) -------------------------------------------------------
__device__ __forceinline__ void fps_emit(int *__restrict__ idx, float *__restrict__ new_xyz, size_t slot, int old, float x,
                                         float y, float z) {
  if (threadIdx.x == 0) {
    idx[slot] = old;
    new_xyz[slot * 3 + 0] = x;
    new_xyz[slot * 3 + 1] = y;
    new_xyz[slot * 3 + 2] = z;
  }
}

template <int NT, int PT>
__global__ __launch_bounds__(NT) void k_pn_fps(const float *__restrict__ xyz, int N, int npoint, int *__restrict__ idx,
                                               float *__restrict__ new_xyz, uint32_t *__restrict__ status) {
  constexpr int NW = NT / 64;
  static_assert(NW >= 1 && NW <= 16 && (NW & (NW - 1)) == 0, "the waves' slots are read by lane & (NW - 1)");
  __shared__ int4 s_a[2][NW];
  __shared__ float s_z[2][NW];
  const int b = blockIdx.x;
  const float *p = xyz + (size_t)b * N * 3;
  float px[PT], py[PT], pz[PT], pm[PT];
  status_or(pn2::fps_load<PT>(p, 3, N, px, py, pz, pm) ? DFU3D_PN2_ST_BAD_POINT : 0u, status);
  int old = 0;
  float x1 = p[0], y1 = p[1], z1 = p[2];
  const size_t out0 = (size_t)b * npoint;
  fps_emit(idx, new_xyz, out0, old, x1, y1, z1);
  for (int s = 1; s < npoint; s++) {
    pn2::fps_step_reg<NW, PT>(px, py, pz, pm, s_a, s_z, s & 1, old, x1, y1, z1);
    fps_emit(idx, new_xyz, out0 + s, old, x1, y1, z1);
  }
}

__global__ __launch_bounds__(FPS_BIG_NT) void k_pn_fps_big(const float *__restrict__ xyz, int N, int npoint,
                                                           int *__restrict__ idx, float *__restrict__ new_xyz,
                                                           float *__restrict__ tmp, uint32_t *__restrict__ status) {
  constexpr int NW = FPS_BIG_NT / 64;
  __shared__ int4 s_a[2][NW];
  __shared__ float s_z[2][NW];
  const int b = blockIdx.x, t = threadIdx.x, lane = t & 63, w = t >> 6;
  const float *p = xyz + (size_t)b * N * 3;
  float *pm = tmp + (size_t)b * N;
  const int chunk = ((N + NW - 1) / NW + 63) & ~63;  // points of a wave
  const int lo = w * chunk < N ? w * chunk : N, hi = lo + chunk < N ? lo + chunk : N;
  int old = 0;
  float x1 = p[0], y1 = p[1], z1 = p[2];
  const size_t out0 = (size_t)b * npoint;
  fps_emit(idx, new_xyz, out0, old, x1, y1, z1);
  bool bad = false;
  for (int s = 1; s < npoint; s++) {
    pn2::fps_step_mem<NW>(p, 3, pm, lo, hi, s == 1, bad, s_a, s_z, s & 1, old, x1, y1, z1);
    fps_emit(idx, new_xyz, out0 + s, old, x1, y1, z1);
  }
  if (npoint == 1)                                   // the walk that looks at the coordinates did not run
    for (int k = lo + lane; k < hi; k += 64)
      if (!pn2::finite3(p[k * 3 + 0], p[k * 3 + 1], p[k * 3 + 2])) bad = true;
  status_or(bad ? DFU3D_PN2_ST_BAD_POINT : 0u, status);
}

// ---- ball query -------------------------------------------------------------------------------------------------------
struct BallScale {
  float r2;
  int nsample;
  int *idx;
};

__global__ __launch_bounds__(BT) void k_pn_ball(const float *__restrict__ xyz, const float *__restrict__ centres, int N, int M,
                                                int S, BallScale s0, BallScale s1) {
  const int lane = lane_id(), b = blockIdx.y, m = blockIdx.x * (BT / 64) + (threadIdx.x >> 6);
  if (m >= M) return;                                // a whole wave; the kernel has no barrier
  const float *p = xyz + (size_t)b * N * 3, *c = centres + ((size_t)b * M + m) * 3;
  const float cx = c[0], cy = c[1], cz = c[2];
  int *o0 = s0.idx + ((size_t)b * M + m) * s0.nsample;
  int *o1 = S > 1 ? s1.idx + ((size_t)b * M + m) * s1.nsample : nullptr;
  int cnt0 = 0, cnt1 = 0, first0 = 0, first1 = 0;
  bool full0 = false, full1 = S < 2;
  for (int base = 0; base < N && !(full0 && full1); base += 256) {
    float d2[4];
#pragma unroll
    for (int u = 0; u < 4; u++) {
      const int k = base + u * 64 + lane;
      d2[u] = INFINITY;                              // no point: below no radius
      if (k < N) d2[u] = sqdist(cx, cy, cz, p[k * 3 + 0], p[k * 3 + 1], p[k * 3 + 2]);
    }
#pragma unroll
    for (int u = 0; u < 4; u++) {
      const int k = base + u * 64 + lane;
      if (!full0) ball_take(d2[u] < s0.r2, k, base + u * 64, s0.nsample, o0, cnt0, first0, full0);
      if (!full1) ball_take(d2[u] < s1.r2, k, base + u * 64, s1.nsample, o1, cnt1, first1, full1);
    }
  }
  for (int i = cnt0 + lane; i < s0.nsample; i += 64) o0[i] = first0;    // the first hit, or 0 without one
  if (S > 1)
    for (int i = cnt1 + lane; i < s1.nsample; i += 64) o1[i] = first1;
}

// ---- grouping ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(BT) void k_pn_group(const float *__restrict__ xyz, const float *__restrict__ centres,
                                                 const uint32_t *__restrict__ feat, const int *__restrict__ idx, int N, int M,
                                                 int ns, int C, int use_xyz, uint32_t *__restrict__ out,
                                                 uint32_t *__restrict__ status) {
  const int b = blockIdx.z, e = blockIdx.x * BT + threadIdx.x, E = M * ns;
  uint32_t st = 0u;
  if (e < E) {
    int i = idx[(size_t)b * E + e];
    if ((unsigned)i >= (unsigned)N) {
      st = DFU3D_PN2_ST_BAD_INDEX;
      i = 0;
    }
    const int xo = use_xyz ? 3 : 0;
    uint32_t *o = out + (size_t)b * (xo + C) * E + e;
    if (use_xyz && blockIdx.y == 0) {
      const float *q = xyz + ((size_t)b * N + i) * 3, *c = centres + ((size_t)b * M + e / ns) * 3;
      float *of = reinterpret_cast<float *>(o);
      of[0] = q[0] - c[0];
      of[(size_t)E] = q[1] - c[1];
      of[(size_t)2 * E] = q[2] - c[2];
    }
    const int c0 = blockIdx.y * CCH, c1 = c0 + CCH < C ? c0 + CCH : C;
    const uint32_t *f = feat + (size_t)b * C * N + i;
    for (int ch = c0; ch < c1; ch++) o[(size_t)(xo + ch) * E] = f[(size_t)ch * N];
  }
  status_or(st, status);
}

// ---- three nearest neighbours, interpolation --------------------------------------------------------------------------
__global__ __launch_bounds__(BT) void k_pn_three_nn(const float *__restrict__ unknown, const float *__restrict__ known, int n,
                                                    int m, float *__restrict__ dist, int *__restrict__ idx) {
  __shared__ float s_k[BT * 3];
  const int b = blockIdx.y, t = threadIdx.x, j = blockIdx.x * BT + t;
  const float *kp = known + (size_t)b * m * 3;
  float ux = 0.0f, uy = 0.0f, uz = 0.0f;
  if (j < n) {
    const float *u = unknown + ((size_t)b * n + j) * 3;
    ux = u[0];
    uy = u[1];
    uz = u[2];
  }
  float b1 = INFINITY, b2 = INFINITY, b3 = INFINITY;
  int i1 = 0, i2 = 0, i3 = 0;
  for (int k0 = 0; k0 < m; k0 += BT) {
    const int nk = m - k0 < BT ? m - k0 : BT;
    if (k0) __syncthreads();                         // the tile before has been read
    for (int i = t; i < nk * 3; i += BT) s_k[i] = kp[(size_t)k0 * 3 + i];
    __syncthreads();
    for (int i = 0; i < nk; i++) {
      const float d = sqdist(ux, uy, uz, s_k[i * 3 + 0], s_k[i * 3 + 1], s_k[i * 3 + 2]);
      const int k = k0 + i;
      if (d < b1) {
        b3 = b2; i3 = i2;
        b2 = b1; i2 = i1;
        b1 = d; i1 = k;
      } else if (d < b2) {
        b3 = b2; i3 = i2;
        b2 = d; i2 = k;
      } else if (d < b3) {
        b3 = d; i3 = k;
      }
    }
  }
  if (j < n) {
    float *od = dist + ((size_t)b * n + j) * 3;
    int *oi = idx + ((size_t)b * n + j) * 3;
    od[0] = sqrtf(b1); od[1] = sqrtf(b2); od[2] = sqrtf(b3);
    oi[0] = i1; oi[1] = i2; oi[2] = i3;
  }
}

__global__ __launch_bounds__(BT) void k_pn_interp(const float *__restrict__ feat, const int *__restrict__ idx,
                                                  const float *__restrict__ weight, int C, int m, int n,
                                                  float *__restrict__ out, uint32_t *__restrict__ status) {
  const int b = blockIdx.z, j = blockIdx.x * BT + threadIdx.x;
  uint32_t st = 0u;
  if (j < n) {
    const int *ip = idx + ((size_t)b * n + j) * 3;
    const float *wp = weight + ((size_t)b * n + j) * 3;
    int i0 = ip[0], i1 = ip[1], i2 = ip[2];
    if ((unsigned)i0 >= (unsigned)m || (unsigned)i1 >= (unsigned)m || (unsigned)i2 >= (unsigned)m) {
      st = DFU3D_PN2_ST_BAD_INDEX;
      i0 = (unsigned)i0 >= (unsigned)m ? 0 : i0;
      i1 = (unsigned)i1 >= (unsigned)m ? 0 : i1;
      i2 = (unsigned)i2 >= (unsigned)m ? 0 : i2;
    }
    const float w0 = wp[0], w1 = wp[1], w2 = wp[2];
    const int c0 = blockIdx.y * CCH, c1 = c0 + CCH < C ? c0 + CCH : C;
    for (int ch = c0; ch < c1; ch++) {
      const float *f = feat + ((size_t)b * C + ch) * m;
      out[((size_t)b * C + ch) * n + j] = w0 * f[i0] + w1 * f[i1] + w2 * f[i2];
    }
  }
  status_or(st, status);
}

// ---- the inverse of a gather and the ordered backward ---------------------------------------------------------------
__global__ __launch_bounds__(BT) void k_pn_count(const int *__restrict__ idx, int N, int E, int *__restrict__ csr,
                                                 uint32_t *__restrict__ status) {
  const int b = blockIdx.y, e = blockIdx.x * BT + threadIdx.x;
  uint32_t st = 0u;
  if (e < E) {
    const int s = idx[(size_t)b * E + e];
    if ((unsigned)s < (unsigned)N)
      atomicAdd(&csr[(size_t)b * (N + 1) + s], 1);
    else
      st = DFU3D_PN2_ST_BAD_INDEX;
  }
  status_or(st, status);
}

// counts -> exclusive offsets, in place; csr[N] <- the number of entries kept; cursor <- the offsets
__global__ __launch_bounds__(BT) void k_pn_offsets(int *__restrict__ csr, int *__restrict__ cursor, int N) {
  __shared__ int s_w[BT / 64];
  int *c = csr + (size_t)blockIdx.x * (N + 1), *cur = cursor + (size_t)blockIdx.x * N;
  const int total = block_scan_range<BT, 4, int, int>(
      N, [&](int i) { return c[i]; }, [&](int i, int ex) { c[i] = ex; cur[i] = ex; }, s_w);
  if (threadIdx.x == 0) c[N] = total;
}

__global__ __launch_bounds__(BT) void k_pn_place(const int *__restrict__ idx, int N, int E, int *__restrict__ cursor,
                                                 int *__restrict__ tmp) {
  const int b = blockIdx.y, e = blockIdx.x * BT + threadIdx.x;
  if (e >= E) return;
  const int s = idx[(size_t)b * E + e];
  if ((unsigned)s >= (unsigned)N) return;
  const int pos = atomicAdd(&cursor[(size_t)b * N + s], 1);
  if ((unsigned)pos < (unsigned)E) tmp[(size_t)b * E + pos] = e;   // (always, for the idx k_pn_count saw)
}

// one wave per source: its run of entry numbers (distinct, in the order the atomics left) into ascending order, every
// element to the place its rank gives it
__global__ __launch_bounds__(BT) void k_pn_order(const int *__restrict__ csr, const int *__restrict__ tmp,
                                                 int *__restrict__ list, int N, int E) {
  const int lane = lane_id(), b = blockIdx.y, s = blockIdx.x * (BT / 64) + (threadIdx.x >> 6);
  if (s >= N) return;                                // a whole wave; the kernel has no barrier
  const int beg = csr[(size_t)b * (N + 1) + s], L = csr[(size_t)b * (N + 1) + s + 1] - beg;
  if (L <= 0 || beg < 0 || beg > E - L) return;
  const int *seg = tmp + (size_t)b * E + beg;
  int *dst = list + (size_t)b * E + beg;
  for (int a0 = 0; a0 < L; a0 += 64) {
    const int a = a0 + lane < L ? seg[a0 + lane] : 0x7FFFFFFF;
    int rank = 0;
    for (int b0 = 0; b0 < L; b0 += 64) {
      const int bv = b0 + lane < L ? seg[b0 + lane] : 0x7FFFFFFF;
      const int nb = L - b0 < 64 ? L - b0 : 64;
      for (int i = 0; i < nb; i++) rank += __builtin_amdgcn_readlane(bv, i) < a ? 1 : 0;
    }
    if (a0 + lane < L && rank < L) dst[rank] = a;
  }
}

__global__ __launch_bounds__(BT) void k_pn_gather_bwd(const float *__restrict__ go, const float *__restrict__ w,
                                                      const int *__restrict__ csr, const int *__restrict__ list, int C, int N,
                                                      int E, int k, float *__restrict__ gf) {
  const int b = blockIdx.z, s = blockIdx.x * BT + threadIdx.x;
  if (s >= N) return;
  int beg = csr[(size_t)b * (N + 1) + s], end = csr[(size_t)b * (N + 1) + s + 1];
  beg = beg < 0 ? 0 : (beg > E ? E : beg);
  end = end < beg ? beg : (end > E ? E : end);
  const int *l = list + (size_t)b * E;
  const float *wb = w ? w + (size_t)b * E : nullptr;
  const int Ek = E / k, c0 = blockIdx.y * CCH, c1 = c0 + CCH < C ? c0 + CCH : C;
  for (int ch = c0; ch < c1; ch++) {
    const float *g = go + ((size_t)b * C + ch) * Ek;
    float acc = 0.0f;
    for (int q = beg; q < end; q++) {
      const int e = l[q];
      if ((unsigned)e >= (unsigned)E) continue;
      float v = g[k == 1 ? e : e / k];
      if (wb) v = wb[e] * v;
      acc = acc + v;
    }
    gf[((size_t)b * C + ch) * N + s] = acc;
  }
}

__global__ __launch_bounds__(BT) void k_pn_check_batch(const float *__restrict__ points, long long rows, int cols, int per,
                                                       uint32_t *__restrict__ status) {
  uint32_t st = 0u;
  for (long long r = (long long)blockIdx.x * BT + threadIdx.x; r < rows; r += (long long)gridDim.x * BT)
    if (!(points[r * cols] == (float)(r / per))) st = DFU3D_PN2_ST_BAD_BATCH;
  status_or(st, status);
}

// ---- host side --------------------------------------------------------------------------------------------------------
bool dims_ok(int32_t B, int32_t a, int32_t b) { return B >= 1 && a >= 1 && b >= 1; }
// DFU3D_OK, or DFU3D_ERANGE when a batch, a point count or a tensor of `elems` elements is beyond its limit
int range_of(int32_t B, int32_t a, int32_t b, double elems) {
  if (B > DFU3D_PN2_MAX_BATCH || a > DFU3D_PN2_MAX_POINTS || b > DFU3D_PN2_MAX_POINTS) return DFU3D_ERANGE;
  return elems > (double)DFU3D_PN2_MAX_ELEMS ? DFU3D_ERANGE : DFU3D_OK;
}
unsigned blocks(int64_t n, int per) { return (unsigned)((n + per - 1) / per < 1 ? 1 : (n + per - 1) / per); }

template <int NT, int PT>
void launch_fps(const float *xyz, int B, int N, int npoint, int *idx, float *new_xyz, uint32_t *status, hipStream_t st) {
  hipLaunchKernelGGL((k_pn_fps<NT, PT>), dim3(B), dim3(NT), 0, st, xyz, N, npoint, idx, new_xyz, status);
}

}  // namespace

extern "C" int32_t dfu3d_pn2_version(void) { return DFU3D_PN2_VERSION; }

extern "C" int64_t dfu3d_pn2_scratch_bytes(int32_t B, int32_t N, int64_t E) {
  if (B < 1 || N < 1 || E < 0 || B > DFU3D_PN2_MAX_BATCH || N > DFU3D_PN2_MAX_POINTS) return -1;
  if (E == 0) return N <= DFU3D_PN2_FPS_ONCHIP ? 0 : (int64_t)B * N * (int64_t)sizeof(float);
  if ((double)B * (double)E > (double)DFU3D_PN2_MAX_ELEMS) return -1;
  return ((int64_t)B * N + (int64_t)B * E) * (int64_t)sizeof(int32_t);      // cursor (B, N), then the unsorted list (B, E)
}

extern "C" int dfu3d_pn2_fps(const float *xyz, int32_t B, int32_t N, int32_t npoint, int32_t *idx, float *new_xyz,
                             void *scratch, uint32_t *status, void *stream) {
  DFU3D_CLEAR_STALE_ERROR();
  if (!xyz || !idx || !new_xyz || !status || !dims_ok(B, N, npoint) || npoint > N) return DFU3D_EINVAL;
  const int rc = range_of(B, N, npoint, (double)B * N * 3.0);
  if (rc != DFU3D_OK) return rc;
  if (N > DFU3D_PN2_FPS_ONCHIP && !scratch) return DFU3D_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  if (N <= 256) launch_fps<256, 1>(xyz, B, N, npoint, idx, new_xyz, status, st);
  else if (N <= 1024) launch_fps<256, 4>(xyz, B, N, npoint, idx, new_xyz, status, st);
  else if (N <= 2048) launch_fps<1024, 2>(xyz, B, N, npoint, idx, new_xyz, status, st);
  else if (N <= 4096) launch_fps<1024, 4>(xyz, B, N, npoint, idx, new_xyz, status, st);
  else if (N <= 8192) launch_fps<1024, 8>(xyz, B, N, npoint, idx, new_xyz, status, st);
  else if (N <= DFU3D_PN2_FPS_ONCHIP) launch_fps<1024, 16>(xyz, B, N, npoint, idx, new_xyz, status, st);
  else
    hipLaunchKernelGGL(k_pn_fps_big, dim3(B), dim3(FPS_BIG_NT), 0, st, xyz, N, npoint, idx, new_xyz, (float *)scratch,
                       status);
  DFU3D_LAUNCH_CHECK();
  return DFU3D_OK;
}
static_assert(DFU3D_PN2_FPS_ONCHIP == 1024 * 16, "the largest register form");

extern "C" int dfu3d_pn2_ball_query(const float *xyz, const float *centres, int32_t B, int32_t N, int32_t M,
                                    int32_t n_scales, float radius0, int32_t nsample0, int32_t *idx0, float radius1,
                                    int32_t nsample1, int32_t *idx1, void *stream) {
  DFU3D_CLEAR_STALE_ERROR();
  if (!xyz || !centres || !dims_ok(B, N, M) || n_scales < 1 || n_scales > DFU3D_PN2_MAX_SCALES) return DFU3D_EINVAL;
  if (!idx0 || nsample0 < 1 || radius0 != radius0) return DFU3D_EINVAL;
  if (n_scales > 1 && (!idx1 || nsample1 < 1 || radius1 != radius1 || idx1 == idx0)) return DFU3D_EINVAL;
  const int32_t ns_max = n_scales > 1 && nsample1 > nsample0 ? nsample1 : nsample0;
  const int rc = range_of(B, N, M, (double)B * M * (double)ns_max);
  if (rc != DFU3D_OK) return rc;
  BallScale s0{radius0 * radius0, nsample0, idx0}, s1{0.0f, 1, nullptr};
  if (n_scales > 1) s1 = BallScale{radius1 * radius1, nsample1, idx1};
  hipLaunchKernelGGL(k_pn_ball, dim3(blocks(M, BT / 64), B), dim3(BT), 0, (hipStream_t)stream, xyz, centres, N, M, n_scales,
                     s0, s1);
  DFU3D_LAUNCH_CHECK();
  return DFU3D_OK;
}

extern "C" int dfu3d_pn2_group(const float *xyz, const float *centres, const float *features, const int32_t *idx,
                               int32_t B, int32_t N, int32_t M, int32_t nsample, int32_t C, int32_t use_xyz, float *out,
                               uint32_t *status, void *stream) {
  DFU3D_CLEAR_STALE_ERROR();
  if (!idx || !out || !status || !dims_ok(B, N, M) || nsample < 1 || C < 0) return DFU3D_EINVAL;
  if (!features) C = 0;
  if (use_xyz ? (!xyz || !centres) : C == 0) return DFU3D_EINVAL;
  const int cout = (use_xyz ? 3 : 0) + C;
  int rc = range_of(B, N, M, (double)B * cout * (double)M * nsample);
  if (rc == DFU3D_OK) rc = range_of(B, N, M, (double)B * (C > 3 ? C : 3) * (double)N);
  if (rc != DFU3D_OK) return rc;
  hipLaunchKernelGGL(k_pn_group, dim3(blocks((int64_t)M * nsample, BT), blocks(C, CCH), B), dim3(BT), 0, (hipStream_t)stream,
                     xyz, centres, (const uint32_t *)features, idx, N, M, nsample, C, use_xyz ? 1 : 0, (uint32_t *)out, status);
  DFU3D_LAUNCH_CHECK();
  return DFU3D_OK;
}

extern "C" int dfu3d_pn2_three_nn(const float *unknown, const float *known, int32_t B, int32_t n, int32_t m, float *dist,
                                  int32_t *idx, void *stream) {
  DFU3D_CLEAR_STALE_ERROR();
  if (!unknown || !known || !dist || !idx || !dims_ok(B, n, m)) return DFU3D_EINVAL;
  const int rc = range_of(B, n, m, (double)B * 3.0 * (n > m ? n : m));
  if (rc != DFU3D_OK) return rc;
  hipLaunchKernelGGL(k_pn_three_nn, dim3(blocks(n, BT), B), dim3(BT), 0, (hipStream_t)stream, unknown, known, n, m, dist, idx);
  DFU3D_LAUNCH_CHECK();
  return DFU3D_OK;
}

extern "C" int dfu3d_pn2_three_interpolate(const float *features, const int32_t *idx, const float *weight, int32_t B,
                                           int32_t C, int32_t m, int32_t n, float *out, uint32_t *status, void *stream) {
  DFU3D_CLEAR_STALE_ERROR();
  if (!features || !idx || !weight || !out || !status || !dims_ok(B, m, n) || C < 1) return DFU3D_EINVAL;
  const int rc = range_of(B, m, n, (double)B * C * (double)(n > m ? n : m));
  if (rc != DFU3D_OK) return rc;
  if ((const void *)features == (const void *)out) return DFU3D_EINVAL;
  hipLaunchKernelGGL(k_pn_interp, dim3(blocks(n, BT), blocks(C, CCH), B), dim3(BT), 0, (hipStream_t)stream, features, idx,
                     weight, C, m, n, out, status);
  DFU3D_LAUNCH_CHECK();
  return DFU3D_OK;
}

extern "C" int dfu3d_pn2_invert(const int32_t *idx, int32_t B, int32_t N, int64_t E, int32_t *csr, int32_t *list,
                                void *scratch, uint32_t *status, void *stream) {
  DFU3D_CLEAR_STALE_ERROR();
  if (!idx || !csr || !list || !scratch || !status || B < 1 || N < 1 || E < 1) return DFU3D_EINVAL;
  if (E > DFU3D_PN2_MAX_ELEMS) return DFU3D_ERANGE;
  int rc = range_of(B, N, 1, (double)B * (double)E);
  if (rc == DFU3D_OK) rc = range_of(B, N, 1, (double)B * ((double)N + 1.0));
  if (rc != DFU3D_OK) return rc;
  hipStream_t st = (hipStream_t)stream;
  int *cursor = (int *)scratch, *tmp = cursor + (size_t)B * N;
  if (dfu3d_fill_async(csr, 0, (size_t)B * (N + 1) * sizeof(int32_t), st) != hipSuccess) return DFU3D_ELAUNCH;
  const dim3 ge(blocks(E, BT), B);
  hipLaunchKernelGGL(k_pn_count, ge, dim3(BT), 0, st, idx, N, (int)E, csr, status);
  DFU3D_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_pn_offsets, dim3(B), dim3(BT), 0, st, csr, cursor, N);
  DFU3D_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_pn_place, ge, dim3(BT), 0, st, idx, N, (int)E, cursor, tmp);
  DFU3D_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_pn_order, dim3(blocks(N, BT / 64), B), dim3(BT), 0, st, (const int *)csr, (const int *)tmp, list, N,
                     (int)E);
  DFU3D_LAUNCH_CHECK();
  return DFU3D_OK;
}

extern "C" int dfu3d_pn2_gather_backward(const float *grad_out, const float *w, const int32_t *csr, const int32_t *list,
                                         int32_t B, int32_t C, int32_t N, int64_t E, int32_t k, float *grad_features,
                                         void *stream) {
  DFU3D_CLEAR_STALE_ERROR();
  if (!grad_out || !csr || !list || !grad_features || B < 1 || C < 1 || N < 1 || E < 1 || k < 1 || E % k != 0)
    return DFU3D_EINVAL;
  if (E > DFU3D_PN2_MAX_ELEMS) return DFU3D_ERANGE;
  int rc = range_of(B, N, 1, (double)B * C * (double)(E / k));
  if (rc == DFU3D_OK) rc = range_of(B, N, 1, (double)B * C * (double)N);
  if (rc == DFU3D_OK) rc = range_of(B, N, 1, (double)B * (double)E);
  if (rc != DFU3D_OK) return rc;
  if ((const void *)grad_out == (const void *)grad_features) return DFU3D_EINVAL;
  hipLaunchKernelGGL(k_pn_gather_bwd, dim3(blocks(N, BT), blocks(C, CCH), B), dim3(BT), 0, (hipStream_t)stream, grad_out, w,
                     csr, list, C, N, (int)E, k, grad_features);
  DFU3D_LAUNCH_CHECK();
  return DFU3D_OK;
}

extern "C" int dfu3d_pn2_check_batch(const float *points, int64_t rows, int32_t cols, int32_t per_sample, uint32_t *status,
                                     void *stream) {
  DFU3D_CLEAR_STALE_ERROR();
  if (!points || !status || rows < 1 || cols < 4 || per_sample < 1 || rows % per_sample != 0) return DFU3D_EINVAL;
  if ((double)rows * cols > (double)DFU3D_PN2_MAX_ELEMS) return DFU3D_ERANGE;
  const int64_t g = (rows + BT - 1) / BT;
  hipLaunchKernelGGL(k_pn_check_batch, dim3((unsigned)(g > 4096 ? 4096 : g)), dim3(BT), 0, (hipStream_t)stream, points,
                     (long long)rows, cols, per_sample, status);
  DFU3D_LAUNCH_CHECK();
  return DFU3D_OK;
}
