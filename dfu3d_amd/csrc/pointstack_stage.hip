// pointstack_stage.hip -- SURVEY.md §8 row f-22: the native ops of PV-RCNN's stacked set abstraction (csrc/dfu3d_stk.h).
//
// What it stands in for in the reference: pcdet/ops/pointnet2/pointnet2_stack (CUDA only) and the torch code around it
// in VoxelSetAbstraction -- B masked sums per source for the counts, one FPS launch per sample, a one-thread-per-centre
// linear scan for the centre's sample, two grouping launches, a subtraction, two masked fills and a permute per scale,
// a permuted copy of the BEV map and four fancy-index gathers per sample.
//
//   k_stk_count       one thread per row: the sample index of column 0, checked; a wave whose rows share one sample (all
//                     but B - 1 waves of a sorted tensor) adds once, the others per lane.  Integer atomics.
//   k_stk_starts      counts -> starts, one workgroup scan.
//   k_stk_fps<NT, PT> one workgroup per sample over start: the register form of k_pn_fps (the step is pn2_device.hpp's,
//                     so the picks are its picks), keypoints [b, x, y, z] written as they are picked, short samples
//                     cycled after the last pick.
//   k_stk_fps_big     the memory form, for a bound beyond DFU3D_STK_FPS_ONCHIP.
//   k_stk_ball        one wave per centre, its sample by a binary search in cstart, all scales in one walk over the
//                     sample's rows only: 256 rows per trip, the tile hits of pn2_device.hpp; the walk ends when every
//                     scale is full.  Writes the empty flags.
//   k_stk_group       one thread per (centre, slot) and chunk of channels: xyz - centre, then the feature row's channels
//                     as bits; out is (3 + C, M, nsample), so stores are coalesced and nothing is permuted afterwards.
//   k_stk_gidx        global rows for the backward, -1 for what is left out.
//   k_stk_bev         one thread per (keypoint, channel), channel fastest.
#include "common.hpp"
#include "dfu3d_stk.h"
#include "dfu3d_pn2.h"
#include "pn2_device.hpp"

#include <math.h>

namespace {

constexpr int BT = 256;
constexpr int CCH = 16;                              // channels per workgroup of k_stk_group
constexpr int FPS_BIG_NT = 1024;

using pn2::ball_take;
using pn2::sqdist;
using pn2::status_or;

static_assert(DFU3D_STK_FPS_ONCHIP == DFU3D_PN2_FPS_ONCHIP && DFU3D_STK_MAX_SCALES == DFU3D_PN2_MAX_SCALES,
              "the stacked ops share the limits of the batched ones");

// rows of sample b inside [0, rows]: lo .. lo + n
__device__ __forceinline__ void sample_rows(const int *__restrict__ start, int b, int rows, int &lo, int &n, uint32_t &st) {
  const int a = start[b], e = start[b + 1];
  lo = a < 0 ? 0 : (a > rows ? rows : a);
  const int hi = e < lo ? lo : (e > rows ? rows : e);
  n = hi - lo;
  if (lo != a || hi != e) st |= DFU3D_STK_ST_BAD_COUNT;
}

// the sample whose rows hold row m: the first b with start[b + 1] > m; B when there is none
__device__ __forceinline__ int sample_of(const int *__restrict__ start, int B, int m) {
  int lo = 0, hi = B;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (start[mid + 1] <= m) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// ---- counts and starts ------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool batch_of(const void *__restrict__ col, int is_int, size_t at, int B, int &b, float &raw) {
  if (is_int) {
    b = static_cast<const int *>(col)[at];
    raw = (float)b;                                  // only compared with its neighbour's: monotone in b
    return (unsigned)b < (unsigned)B;
  }
  raw = static_cast<const float *>(col)[at];
  if (!(raw >= 0.0f && raw < (float)B)) return false;
  b = (int)raw;
  return (float)b == raw;
}

__global__ __launch_bounds__(BT) void k_stk_count(const void *__restrict__ col, int is_int, long long rows, int stride, int B,
                                                  int *__restrict__ cnt, uint32_t *__restrict__ status) {
  const long long r = (long long)blockIdx.x * BT + threadIdx.x;
  uint32_t st = 0u;
  int b = -1;
  if (r < rows) {
    float raw = 0.0f;
    int bb = 0;
    if (batch_of(col, is_int, (size_t)r * stride, B, bb, raw)) b = bb; else st |= DFU3D_STK_ST_BAD_BATCH;
    if (r + 1 < rows) {
      float next = 0.0f;
      if (is_int) {
        if (static_cast<const int *>(col)[(size_t)(r + 1) * stride] < static_cast<const int *>(col)[(size_t)r * stride])
          st |= DFU3D_STK_ST_UNSORTED;
      } else {
        next = static_cast<const float *>(col)[(size_t)(r + 1) * stride];
        if (next < raw) st |= DFU3D_STK_ST_UNSORTED;
      }
    }
  }
  const int b0 = readlane_i(b, 0);
  if (__ballot(b == b0) == ~0ull) {                  // one sample for the whole wave
    if (lane_id() == 0 && b0 >= 0) atomicAdd(&cnt[b0], 64);
  } else if (b >= 0) {
    atomicAdd(&cnt[b], 1);
  }
  status_or(st, status);
}

__global__ __launch_bounds__(BT) void k_stk_starts(const int *__restrict__ cnt, int B, int *__restrict__ start,
                                                   uint32_t *__restrict__ status) {
  __shared__ int s_w[BT / 64];
  uint32_t st = 0u;
  const int total = block_scan_range<BT, 4, int, int>(
      B, [&](int i) { const int c = cnt[i]; if (c < 0) st = DFU3D_STK_ST_BAD_COUNT; return c < 0 ? 0 : c; },
      [&](int i, int ex) { start[i] = ex; }, s_w);
  if (threadIdx.x == 0) start[B] = total;
  status_or(st, status);
}

// ---- farthest point sampling ------------------------------------------------------------------------------------------
__device__ __forceinline__ void stk_emit(int *__restrict__ idx, float *__restrict__ kp, size_t slot, int b, int old, float x,
                                         float y, float z) {
  if (threadIdx.x == 0) {
    idx[slot] = old;
    kp[slot * 4 + 0] = (float)b;
    kp[slot * 4 + 1] = x;
    kp[slot * 4 + 2] = y;
    kp[slot * 4 + 3] = z;
  }
}

// after the last pick: a sample without rows -> index 0 and [b, 0, 0, 0]; a short one -> its picks again, in order
__device__ __forceinline__ void stk_fill(int *__restrict__ idx, float *__restrict__ kp, size_t out0, int b, int npick, int K) {
  __syncthreads();                                   // thread 0's picks are visible to the workgroup
  for (int j = npick + (int)threadIdx.x; j < K; j += (int)blockDim.x) {
    int v = 0;
    float x = 0.0f, y = 0.0f, z = 0.0f;
    if (npick > 0) {
      const size_t s = out0 + (size_t)(j % npick);
      v = idx[s];
      x = kp[s * 4 + 1];
      y = kp[s * 4 + 2];
      z = kp[s * 4 + 3];
    }
    idx[out0 + j] = v;
    kp[(out0 + j) * 4 + 0] = (float)b;
    kp[(out0 + j) * 4 + 1] = x;
    kp[(out0 + j) * 4 + 2] = y;
    kp[(out0 + j) * 4 + 3] = z;
  }
}

template <int NT, int PT>
__global__ __launch_bounds__(NT) void k_stk_fps(const float *__restrict__ xyz, int stride, int rows,
                                                const int *__restrict__ start, int K, int bound, int *idx, float *kp,
                                                uint32_t *__restrict__ status) {
  constexpr int NW = NT / 64;
  static_assert(NW >= 1 && NW <= 16 && (NW & (NW - 1)) == 0, "the waves' slots are read by lane & (NW - 1)");
  __shared__ int4 s_a[2][NW];
  __shared__ float s_z[2][NW];
  const int b = blockIdx.x;
  uint32_t st = 0u;
  int lo, n;
  sample_rows(start, b, rows, lo, n, st);
  if (n > bound) {                                   // bound <= NT * PT: the registers hold what is sampled
    st |= DFU3D_STK_ST_BAD_COUNT;
    n = bound;
  }
  if (n == 0) st |= DFU3D_STK_ST_EMPTY;
  const size_t out0 = (size_t)b * K;
  const int npick = n < K ? n : K;
  if (n > 0) {                                       // uniform over the workgroup
    const float *p = xyz + (size_t)lo * stride;
    float px[PT], py[PT], pz[PT], pm[PT];
    if (pn2::fps_load<PT>(p, stride, n, px, py, pz, pm)) st |= DFU3D_STK_ST_BAD_POINT;
    int old = 0;
    float x1 = p[0], y1 = p[1], z1 = p[2];
    stk_emit(idx, kp, out0, b, old, x1, y1, z1);
    for (int s = 1; s < npick; s++) {
      pn2::fps_step_reg<NW, PT>(px, py, pz, pm, s_a, s_z, s & 1, old, x1, y1, z1);
      stk_emit(idx, kp, out0 + s, b, old, x1, y1, z1);
    }
  }
  stk_fill(idx, kp, out0, b, npick, K);
  status_or(st, status);
}

__global__ __launch_bounds__(FPS_BIG_NT) void k_stk_fps_big(const float *__restrict__ xyz, int stride, int rows,
                                                            const int *__restrict__ start, int K, int bound, int *idx,
                                                            float *kp, float *__restrict__ tmp,
                                                            uint32_t *__restrict__ status) {
  constexpr int NW = FPS_BIG_NT / 64;
  __shared__ int4 s_a[2][NW];
  __shared__ float s_z[2][NW];
  const int b = blockIdx.x, lane = lane_id(), w = threadIdx.x >> 6;
  uint32_t st = 0u;
  int lo0, n;
  sample_rows(start, b, rows, lo0, n, st);
  if (n > bound) {                                   // as the register form: the rows beyond the bound are not looked at
    st |= DFU3D_STK_ST_BAD_COUNT;
    n = bound;
  }
  if (n == 0) st |= DFU3D_STK_ST_EMPTY;
  const size_t out0 = (size_t)b * K;
  const int npick = n < K ? n : K;
  if (n > 0) {
    const float *p = xyz + (size_t)lo0 * stride;
    float *pm = tmp + lo0;
    const int chunk = ((n + NW - 1) / NW + 63) & ~63;  // rows of a wave
    const int lo = w * chunk < n ? w * chunk : n, hi = lo + chunk < n ? lo + chunk : n;
    int old = 0;
    float x1 = p[0], y1 = p[1], z1 = p[2];
    stk_emit(idx, kp, out0, b, old, x1, y1, z1);
    bool bad = false;
    for (int s = 1; s < npick; s++) {
      pn2::fps_step_mem<NW>(p, stride, pm, lo, hi, s == 1, bad, s_a, s_z, s & 1, old, x1, y1, z1);
      stk_emit(idx, kp, out0 + s, b, old, x1, y1, z1);
    }
    if (npick == 1)                                  // the walk that looks at the coordinates did not run
      for (int k = lo + lane; k < hi; k += 64)
        if (!pn2::finite3(p[k * stride + 0], p[k * stride + 1], p[k * stride + 2])) bad = true;
    if (bad) st |= DFU3D_STK_ST_BAD_POINT;
  }
  stk_fill(idx, kp, out0, b, npick, K);
  status_or(st, status);
}

// ---- ball query -------------------------------------------------------------------------------------------------------
struct StkScale {
  float r2;
  int nsample;
  int *idx;
  uint8_t *empty;
};

__global__ __launch_bounds__(BT) void k_stk_ball(const float *__restrict__ xyz, int stride, int N, const int *__restrict__ start,
                                                 const float *__restrict__ centres, int cstride, int M,
                                                 const int *__restrict__ cstart, int B, int S, StkScale s0, StkScale s1,
                                                 uint32_t *__restrict__ status) {
  const int lane = lane_id();
  const long long mm = (long long)blockIdx.x * (BT / 64) + (threadIdx.x >> 6);
  if (mm >= M) return;                               // a whole wave; the kernel has no barrier
  const int m = (int)mm;
  uint32_t st = 0u;
  const int b = sample_of(cstart, B, m);
  int lo = 0, n = 0;
  if (b < B && cstart[b] <= m) sample_rows(start, b, N, lo, n, st); else st |= DFU3D_STK_ST_BAD_COUNT;
  const float *p = xyz + (size_t)lo * stride, *c = centres + (size_t)m * cstride;
  const float cx = c[0], cy = c[1], cz = c[2];
  int *o0 = s0.idx + (size_t)m * s0.nsample;
  int *o1 = S > 1 ? s1.idx + (size_t)m * s1.nsample : nullptr;
  int cnt0 = 0, cnt1 = 0, first0 = 0, first1 = 0;
  bool full0 = false, full1 = S < 2;
  for (int base = 0; base < n && !(full0 && full1); base += 256) {
    float d2[4];
#pragma unroll
    for (int u = 0; u < 4; u++) {
      const int k = base + u * 64 + lane;
      d2[u] = INFINITY;                              // no row: below no radius
      if (k < n) d2[u] = sqdist(cx, cy, cz, p[k * stride + 0], p[k * stride + 1], p[k * stride + 2]);
    }
#pragma unroll
    for (int u = 0; u < 4; u++) {
      const int k = base + u * 64 + lane;
      if (!full0) ball_take(d2[u] < s0.r2, k, base + u * 64, s0.nsample, o0, cnt0, first0, full0);
      if (!full1) ball_take(d2[u] < s1.r2, k, base + u * 64, s1.nsample, o1, cnt1, first1, full1);
    }
  }
  for (int i = cnt0 + lane; i < s0.nsample; i += 64) o0[i] = first0;    // the first hit, or 0 without one
  if (lane == 0) s0.empty[m] = cnt0 == 0 ? 1 : 0;
  if (S > 1) {
    for (int i = cnt1 + lane; i < s1.nsample; i += 64) o1[i] = first1;
    if (lane == 0) s1.empty[m] = cnt1 == 0 ? 1 : 0;
  }
  status_or(st, status);
}

// ---- grouping ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(BT) void k_stk_group(const float *__restrict__ xyz, int stride, int N, const int *__restrict__ start,
                                                  const float *__restrict__ centres, int cstride, int M,
                                                  const int *__restrict__ cstart, int B, const uint32_t *__restrict__ feat,
                                                  int C, const int *__restrict__ idx, const uint8_t *__restrict__ empty,
                                                  int ns, uint32_t *__restrict__ out, uint32_t *__restrict__ status) {
  const long long E = (long long)M * ns, e = (long long)blockIdx.x * BT + threadIdx.x;
  uint32_t st = 0u;
  if (e < E) {
    const int m = (int)(e / ns);
    const int b = sample_of(cstart, B, m);
    int lo = 0, n = 0;
    if (b < B && cstart[b] <= m) sample_rows(start, b, N, lo, n, st); else st |= DFU3D_STK_ST_BAD_COUNT;
    bool zero = empty[m] != 0;
    int i = idx[e];
    if (!zero && (unsigned)i >= (unsigned)n) {
      st |= DFU3D_STK_ST_BAD_INDEX;
      i = 0;
      zero = n == 0;
    }
    const size_t g = (size_t)lo + (zero ? 0 : i);
    const int xo = xyz ? 3 : 0;                        // without xyz: the plain grouping_operation
    uint32_t *o = out + e;
    if (xyz && blockIdx.y == 0) {
      float dx = 0.0f, dy = 0.0f, dz = 0.0f;
      if (!zero) {
        const float *q = xyz + g * stride, *c = centres + (size_t)m * cstride;
        dx = q[0] - c[0];
        dy = q[1] - c[1];
        dz = q[2] - c[2];
      }
      float *of = reinterpret_cast<float *>(o);
      of[0] = dx;
      of[(size_t)E] = dy;
      of[(size_t)2 * E] = dz;
    }
    const int c0 = blockIdx.y * CCH, c1 = c0 + CCH < C ? c0 + CCH : C;
    if (zero) {
      for (int ch = c0; ch < c1; ch++) o[(size_t)(xo + ch) * E] = 0u;
    } else {
      const uint32_t *f = feat + g * C;
      for (int ch = c0; ch < c1; ch++) o[(size_t)(xo + ch) * E] = f[ch];
    }
  }
  status_or(st, status);
}

__global__ __launch_bounds__(BT) void k_stk_gidx(const int *__restrict__ idx, const uint8_t *__restrict__ empty, int M, int ns,
                                                 int N, const int *__restrict__ start, const int *__restrict__ cstart, int B,
                                                 int *__restrict__ gidx, uint32_t *__restrict__ status) {
  const long long E = (long long)M * ns, e = (long long)blockIdx.x * BT + threadIdx.x;
  uint32_t st = 0u;
  if (e < E) {
    const int m = (int)(e / ns);
    int g = -1;
    const int b = sample_of(cstart, B, m);           // as k_stk_group: the starts are checked for an empty ball too
    int lo = 0, n = 0;
    if (b < B && cstart[b] <= m) sample_rows(start, b, N, lo, n, st); else st |= DFU3D_STK_ST_BAD_COUNT;
    if (!empty[m]) {
      const int i = idx[e];
      if ((unsigned)i < (unsigned)n) g = lo + i; else st |= DFU3D_STK_ST_BAD_INDEX;
    }
    gidx[e] = g;
  }
  status_or(st, status);
}

// ---- bilinear BEV sampling --------------------------------------------------------------------------------------------
// floor(f) as the reference's .long() then clamp(0, hi) does it, and the same for floor(f) + 1; NaN and both
// infinities -> 0 (.long() of a non-finite float is the most negative integer on the host): both compares are false
__device__ __forceinline__ int clamp_floor(float fl, int hi) {
  return fl >= 0.0f && fl <= 3.402823466e38f ? (fl >= (float)hi ? hi : (int)fl) : 0;
}

__global__ __launch_bounds__(BT) void k_stk_bev(const float *__restrict__ kp, int kstride, long long total,
                                                const float *__restrict__ spatial, int B, int C, int H, int W, float rx,
                                                float ry, float vx, float vy, float bs, float *__restrict__ out,
                                                uint32_t *__restrict__ status) {
  const long long t = (long long)blockIdx.x * BT + threadIdx.x;
  uint32_t st = 0u;
  if (t < total) {
    const long long m = t / C;
    const int c = (int)(t - m * C);
    const float *k = kp + (size_t)m * kstride;
    const float fb = k[0];
    float v = 0.0f;
    if (fb >= 0.0f && fb < (float)B && (float)(int)fb == fb) {
      const float fx = ((k[1] - rx) / vx) / bs, fy = ((k[2] - ry) / vy) / bs;
      const float flx = floorf(fx), fly = floorf(fy);
      const int x0 = clamp_floor(flx, W - 1), x1 = clamp_floor(flx + 1.0f, W - 1);
      const int y0 = clamp_floor(fly, H - 1), y1 = clamp_floor(fly + 1.0f, H - 1);
      const float *im = spatial + ((size_t)(int)fb * C + c) * ((size_t)H * W);
      const float Ia = im[(size_t)y0 * W + x0], Ib = im[(size_t)y1 * W + x0], Ic = im[(size_t)y0 * W + x1],
                  Id = im[(size_t)y1 * W + x1];
      const float wa = ((float)x1 - fx) * ((float)y1 - fy), wb = ((float)x1 - fx) * (fy - (float)y0),
                  wc = (fx - (float)x0) * ((float)y1 - fy), wd = (fx - (float)x0) * (fy - (float)y0);
      v = Ia * wa + Ib * wb + Ic * wc + Id * wd;
    } else {
      st = DFU3D_STK_ST_BAD_BATCH;
    }
    out[t] = v;
  }
  status_or(st, status);
}

// ---- host side --------------------------------------------------------------------------------------------------------
unsigned blocks(int64_t n, int per) { return (unsigned)((n + per - 1) / per < 1 ? 1 : (n + per - 1) / per); }
bool fits(double elems) { return elems <= (double)DFU3D_STK_MAX_ELEMS; }

template <int NT, int PT>
void launch_fps(const float *xyz, int stride, int rows, const int *start, int B, int K, int bound, int *idx, float *kp,
                uint32_t *status, hipStream_t st) {
  hipLaunchKernelGGL((k_stk_fps<NT, PT>), dim3(B), dim3(NT), 0, st, xyz, stride, rows, start, K, bound, idx, kp, status);
}

int64_t fps_bound(int64_t rows, int32_t cap) { return cap >= 1 && cap < rows ? cap : rows; }

// what every call over a stacked set checks: DFU3D_OK, DFU3D_EINVAL or DFU3D_ERANGE
int set_ok(const void *p, int32_t stride, int64_t rows, const int32_t *start, int min_stride) {
  if (rows < 0 || stride < min_stride || !start || (rows > 0 && !p)) return DFU3D_EINVAL;
  return fits((double)rows * stride) ? DFU3D_OK : DFU3D_ERANGE;
}

}  // namespace

extern "C" int32_t dfu3d_stk_version(void) { return DFU3D_STK_VERSION; }

extern "C" int dfu3d_stk_starts(const int32_t *cnt, int32_t B, int32_t *start, uint32_t *status, void *stream) {
  DFU3D_CLEAR_STALE_ERROR();
  if (!cnt || !start || !status || B < 1) return DFU3D_EINVAL;
  if (B > DFU3D_STK_MAX_BATCH) return DFU3D_ERANGE;
  hipLaunchKernelGGL(k_stk_starts, dim3(1), dim3(BT), 0, (hipStream_t)stream, cnt, B, start, status);
  DFU3D_LAUNCH_CHECK();
  return DFU3D_OK;
}

extern "C" int dfu3d_stk_counts(const void *col, int32_t is_int, int64_t rows, int32_t stride, int32_t B, int32_t *cnt,
                                int32_t *start, uint32_t *status, void *stream) {
  DFU3D_CLEAR_STALE_ERROR();
  if (!cnt || !start || !status || B < 1 || stride < 1 || rows < 0 || (rows > 0 && !col)) return DFU3D_EINVAL;
  if (B > DFU3D_STK_MAX_BATCH || !fits((double)rows * stride)) return DFU3D_ERANGE;
  hipStream_t st = (hipStream_t)stream;
  if (dfu3d_fill_async(cnt, 0, (size_t)B * sizeof(int32_t), st) != hipSuccess) return DFU3D_ELAUNCH;
  if (rows > 0) {
    hipLaunchKernelGGL(k_stk_count, dim3(blocks(rows, BT)), dim3(BT), 0, st, col, is_int ? 1 : 0, (long long)rows, stride, B,
                       cnt, status);
    DFU3D_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(k_stk_starts, dim3(1), dim3(BT), 0, st, (const int *)cnt, B, start, status);
  DFU3D_LAUNCH_CHECK();
  return DFU3D_OK;
}

extern "C" int64_t dfu3d_stk_fps_scratch_bytes(int64_t rows, int32_t cap) {
  if (rows < 0 || cap < 0 || rows > DFU3D_STK_MAX_ELEMS / 3) return -1;
  return fps_bound(rows, cap) <= DFU3D_STK_FPS_ONCHIP ? 0 : rows * (int64_t)sizeof(float);
}

extern "C" int dfu3d_stk_fps(const float *xyz, int32_t stride, int64_t rows, const int32_t *start, int32_t B, int32_t K,
                             int32_t cap, int32_t *idx, float *keypoints, void *scratch, uint32_t *status, void *stream) {
  DFU3D_CLEAR_STALE_ERROR();
  if (!idx || !keypoints || !status || B < 1 || K < 1 || cap < 0) return DFU3D_EINVAL;
  const int rc = set_ok(xyz, stride, rows, start, 3);
  if (rc != DFU3D_OK) return rc;
  if (B > DFU3D_STK_MAX_BATCH || !fits((double)B * K * 4.0)) return DFU3D_ERANGE;
  const int64_t bound64 = fps_bound(rows, cap);
  if (bound64 > DFU3D_STK_FPS_ONCHIP && !scratch) return DFU3D_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  const int N = (int)rows, bound = (int)bound64;
  if (bound <= 256) launch_fps<256, 1>(xyz, stride, N, start, B, K, bound, idx, keypoints, status, st);
  else if (bound <= 1024) launch_fps<256, 4>(xyz, stride, N, start, B, K, bound, idx, keypoints, status, st);
  else if (bound <= 2048) launch_fps<1024, 2>(xyz, stride, N, start, B, K, bound, idx, keypoints, status, st);
  else if (bound <= 4096) launch_fps<1024, 4>(xyz, stride, N, start, B, K, bound, idx, keypoints, status, st);
  else if (bound <= 8192) launch_fps<1024, 8>(xyz, stride, N, start, B, K, bound, idx, keypoints, status, st);
  else if (bound <= DFU3D_STK_FPS_ONCHIP) launch_fps<1024, 16>(xyz, stride, N, start, B, K, bound, idx, keypoints, status, st);
  else
    hipLaunchKernelGGL(k_stk_fps_big, dim3(B), dim3(FPS_BIG_NT), 0, st, xyz, stride, N, start, K, bound, idx, keypoints,
                       (float *)scratch, status);
  DFU3D_LAUNCH_CHECK();
  return DFU3D_OK;
}
static_assert(DFU3D_STK_FPS_ONCHIP == 1024 * 16, "the largest register form");

extern "C" int dfu3d_stk_ball_query(const float *xyz, int32_t stride, int64_t N, const int32_t *start, const float *centres,
                                    int32_t cstride, int64_t M, const int32_t *cstart, int32_t B, int32_t n_scales,
                                    float radius0, int32_t nsample0, int32_t *idx0, uint8_t *empty0, float radius1,
                                    int32_t nsample1, int32_t *idx1, uint8_t *empty1, uint32_t *status, void *stream) {
  DFU3D_CLEAR_STALE_ERROR();
  if (!status || B < 1 || n_scales < 1 || n_scales > DFU3D_STK_MAX_SCALES) return DFU3D_EINVAL;
  if (nsample0 < 1 || radius0 != radius0 || (n_scales > 1 && (nsample1 < 1 || radius1 != radius1))) return DFU3D_EINVAL;
  if (M > 0) {                                       // without centres the outputs have no element: any pointer, NULL too
    if (!idx0 || !empty0) return DFU3D_EINVAL;
    if (n_scales > 1 && (!idx1 || !empty1 || idx1 == idx0 || empty1 == empty0)) return DFU3D_EINVAL;
  }
  int rc = set_ok(xyz, stride, N, start, 3);
  if (rc == DFU3D_OK) rc = set_ok(centres, cstride, M, cstart, 3);
  if (rc != DFU3D_OK) return rc;
  const int32_t ns_max = n_scales > 1 && nsample1 > nsample0 ? nsample1 : nsample0;
  if (B > DFU3D_STK_MAX_BATCH || !fits((double)M * ns_max)) return DFU3D_ERANGE;
  if (M == 0) return DFU3D_OK;
  StkScale s0{radius0 * radius0, nsample0, idx0, empty0}, s1{0.0f, 1, nullptr, nullptr};
  if (n_scales > 1) s1 = StkScale{radius1 * radius1, nsample1, idx1, empty1};
  hipLaunchKernelGGL(k_stk_ball, dim3(blocks(M, BT / 64)), dim3(BT), 0, (hipStream_t)stream, xyz, stride, (int)N, start,
                     centres, cstride, (int)M, cstart, B, n_scales, s0, s1, status);
  DFU3D_LAUNCH_CHECK();
  return DFU3D_OK;
}

extern "C" int dfu3d_stk_group(const float *xyz, int32_t stride, int64_t N, const int32_t *start, const float *centres,
                               int32_t cstride, int64_t M, const int32_t *cstart, int32_t B, const float *features,
                               int32_t C, const int32_t *idx, const uint8_t *empty, int32_t nsample, float *out,
                               uint32_t *status, void *stream) {
  DFU3D_CLEAR_STALE_ERROR();
  if (!status || B < 1 || nsample < 1 || C < 0) return DFU3D_EINVAL;
  if (!features) C = 0;
  const bool plain = !xyz && !centres && C > 0;      // the plain grouping_operation: features only
  int rc = plain ? (N < 0 || !start ? DFU3D_EINVAL : DFU3D_OK) : set_ok(xyz, stride, N, start, 3);
  if (rc == DFU3D_OK) rc = plain ? (M < 0 || !cstart ? DFU3D_EINVAL : DFU3D_OK) : set_ok(centres, cstride, M, cstart, 3);
  if (rc != DFU3D_OK) return rc;
  if (B > DFU3D_STK_MAX_BATCH || !fits(((plain ? 0.0 : 3.0) + C) * (double)M * nsample) ||
      !fits((double)N * (C > 3 ? C : 3)) || !fits((double)M * 3.0))
    return DFU3D_ERANGE;
  if (M == 0) return DFU3D_OK;
  if (!idx || !empty || !out) return DFU3D_EINVAL;
  hipLaunchKernelGGL(k_stk_group, dim3(blocks(M * nsample, BT), blocks(C, CCH)), dim3(BT), 0, (hipStream_t)stream, xyz, stride,
                     (int)N, start, centres, cstride, (int)M, cstart, B, (const uint32_t *)features, C, idx, empty, nsample,
                     (uint32_t *)out, status);
  DFU3D_LAUNCH_CHECK();
  return DFU3D_OK;
}

extern "C" int dfu3d_stk_global_index(const int32_t *idx, const uint8_t *empty, int64_t M, int32_t nsample, int64_t N,
                                      const int32_t *start, const int32_t *cstart, int32_t B, int32_t *gidx,
                                      uint32_t *status, void *stream) {
  DFU3D_CLEAR_STALE_ERROR();
  if (!idx || !empty || !start || !cstart || !gidx || !status || B < 1 || M < 1 || nsample < 1 || N < 0) return DFU3D_EINVAL;
  if (B > DFU3D_STK_MAX_BATCH || !fits((double)M * nsample) || !fits((double)N)) return DFU3D_ERANGE;
  hipLaunchKernelGGL(k_stk_gidx, dim3(blocks(M * nsample, BT)), dim3(BT), 0, (hipStream_t)stream, idx, empty, (int)M, nsample,
                     (int)N, start, cstart, B, gidx, status);
  DFU3D_LAUNCH_CHECK();
  return DFU3D_OK;
}

extern "C" int dfu3d_stk_bev_sample(const float *keypoints, int32_t kstride, int64_t M, const float *spatial, int32_t B,
                                    int32_t C, int32_t H, int32_t W, float range_x, float range_y, float voxel_x,
                                    float voxel_y, float bev_stride, float *out, uint32_t *status, void *stream) {
  DFU3D_CLEAR_STALE_ERROR();
  if (!keypoints || !spatial || !out || !status || kstride < 3 || M < 1 || B < 1 || C < 1 || H < 1 || W < 1)
    return DFU3D_EINVAL;
  if ((const void *)spatial == (const void *)out || (const void *)keypoints == (const void *)out) return DFU3D_EINVAL;
  if (B > DFU3D_STK_MAX_BATCH || !fits((double)M * kstride) || !fits((double)M * C) ||
      !fits((double)B * C * (double)H * W))
    return DFU3D_ERANGE;
  hipLaunchKernelGGL(k_stk_bev, dim3(blocks(M * C, BT)), dim3(BT), 0, (hipStream_t)stream, keypoints, kstride,
                     (long long)M * C, spatial, B, C, H, W, range_x, range_y, voxel_x, voxel_y, bev_stride, out, status);
  DFU3D_LAUNCH_CHECK();
  return DFU3D_OK;
}
