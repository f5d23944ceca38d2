// centerloss_stage.hip -- the CenterHead loss (include/dfu3d_head.h): focal loss of the heat maps and L1 loss of the
// regression maps at the target cells, all heads and samples in one launch chain per direction.
//
// Forward, 3 launches: k_cl_focal (fp64 partial sums of a head's heat map per workgroup), k_cl_reg (one workgroup per
// (head, sample): fp64 |pred - target| per channel, summed in slot order), k_cl_final (one workgroup: partials summed in index
// order, the losses rounded once).  Backward, 2 launches: k_cl_hm_bwd (elementwise, recomputed from x and g) and
// k_cl_reg_bwd (a workgroup per (head, sample, span of cells) zeroes its span of every channel, then the lowest slot
// of each target cell in the span sums the cell's slots in ascending slot order and stores once).
//
// The per-head tensors are separate allocations; their addresses travel in the kernel arguments (ClMaps / ClGrads).
// Every reduction has a fixed shape (xor butterfly over the wave, the four waves in order, partials in index order; the
// regression sums in slot order) that depends on the tensors' shapes alone, not on their alignment, and
// there is no float atomic, so every result is the same bits on every run.
#include <math.h>

#include "common.hpp"
#include "dfu3d.h"
#include "dfu3d_head.h"

namespace {

constexpr int CT = 256;                     // threads of every kernel but k_cl_final
constexpr int CW = CT / 64;                 // its waves
constexpr int FOCAL_PER_PART = 4096;        // heat-map elements per workgroup partial before the cap of PARTS is met
constexpr int SPAN = 2048;                  // cells of a workgroup of k_cl_reg_bwd
constexpr int NH = DFU3D_HEAD_MAX_HEADS, NM = DFU3D_HEAD_MAX_REG_MAPS, NC = DFU3D_HEAD_MAX_CODE;
constexpr int PARTS = DFU3D_HEAD_PARTS;
constexpr float P_MIN = 1e-4f, P_MAX = (float)(1 - 1e-4);

struct ClMaps {
  const float *hm[NH], *heat[NH], *tgt[NH];
  const long long *ind[NH], *mask[NH];
  const float *reg[NH][NM];
  int n_cls[NH], parts[NH];
  int ch_map[NC], ch_idx[NC], reg_ch[NM];   // channel d of the code: its map, its channel in the map; channels of a map
  double w[2 + NC];                         // cls_weight, loc_weight, code_weights
  int n_heads, B, hw, n_reg, n_max, code;
};
struct ClGrads {
  float *hm[NH];
  float *reg[NH][NM];
};

// ---- scratch: ONE definition of the carve-up; dfu3d_center_loss_scratch_bytes is its last field ---------------------
struct ClScratch {
  size_t focal, reg, bytes;
};
ClScratch cl_scratch(int n_heads, int batch) {
  ClScratch s;
  size_t o = 0;
  s.focal = o; o += (size_t)n_heads * PARTS * 3 * sizeof(double);          // {S_pos, S_neg, num_pos} per partial
  s.reg = o;   o += (size_t)n_heads * batch * (NC + 1) * sizeof(double);   // {S_d .. , valid slots} per (head, sample)
  s.bytes = o + 16;
  return s;
}

__device__ __forceinline__ float clamped_sigmoid(float x, double &s) {
  s = 1.0 / (1.0 + exp(-(double)x));
  return fminf(fmaxf((float)s, P_MIN), P_MAX);
}

// (noinline: the fp64 exp / log bodies once per kernel, not once per unrolled vector component)
__device__ __noinline__ double focal_value(float x, float g) {
  double s;
  const double p = (double)clamped_sigmoid(x, s);
  const bool is_pos = g == 1.0f;
  const double l = log(is_pos ? p : 1.0 - p);
  double w = 1.0 - (double)g;
  w = w * w;
  return is_pos ? l * ((1.0 - p) * (1.0 - p)) : l * (p * p) * (w * w);
}
// the element's term into the positive (g == 1) or the negative (g < 1) sum.  For g > 1 or NaN the value is computed and
// dropped: heat maps hold no such element, and a branch around the call would only split the wave
__device__ __forceinline__ void focal_term(float x, float g, double &pos, double &neg, double &cnt) {
  const double v = focal_value(x, g);
  if (g == 1.0f) {
    pos += v;
    cnt += 1.0;
  } else if (g < 1.0f) {
    neg += v;
  }
}

__device__ __noinline__ float focal_grad(float x, float g, double scale) {
  double s;
  const float pf = clamped_sigmoid(x, s);
  const float sf = (float)s;
  if (!(sf >= P_MIN && sf <= P_MAX)) return 0.0f;          // torch's clamp passes the gradient iff min <= v <= max
  const double p = (double)pf;
  const bool is_pos = g == 1.0f;
  if (!is_pos && !(g < 1.0f)) return 0.0f;
  const double q = 1.0 - p;
  const double l = log(is_pos ? p : q);
  double dt;
  if (is_pos) {
    dt = q * q / p - 2.0 * q * l;
  } else {
    double w = 1.0 - (double)g;
    w = w * w;
    dt = (w * w) * (2.0 * p * l - p * p / q);
  }
  return (float)(scale * dt * (s * (1.0 - s)));
}

__device__ __forceinline__ bool aligned16(const void *a, const void *b) {
  return ((((uintptr_t)a) | ((uintptr_t)b)) & 15u) == 0;
}

// grid (max parts, n_heads)
__global__ __launch_bounds__(CT) void k_cl_focal(ClMaps a, double *__restrict__ partials) {
  const int h = blockIdx.y, part = blockIdx.x, parts = a.parts[h];
  if (part >= parts) return;
  const float *__restrict__ x = a.hm[h];
  const float *__restrict__ g = a.heat[h];
  const int64_t n = (int64_t)a.B * a.n_cls[h] * a.hw;
  // The partition does not depend on alignment: a thread takes the quads q = t, t + stride, ... of four consecutive
  // elements and, of the n % 4 elements behind the last quad, the one of its index.  Only the way a quad is loaded does.
  const bool vec = aligned16(x, g);
  const int64_t nq = n / 4;
  const int64_t t = (int64_t)part * CT + threadIdx.x, stride = (int64_t)parts * CT;
  double pos = 0.0, neg = 0.0, cnt = 0.0;
  for (int64_t q = t; q < nq; q += stride) {
    float4 xv, gv;
    if (vec) {
      xv = ((const float4 *)x)[q];
      gv = ((const float4 *)g)[q];
    } else {
      xv = make_float4(x[4 * q], x[4 * q + 1], x[4 * q + 2], x[4 * q + 3]);
      gv = make_float4(g[4 * q], g[4 * q + 1], g[4 * q + 2], g[4 * q + 3]);
    }
    focal_term(xv.x, gv.x, pos, neg, cnt);
    focal_term(xv.y, gv.y, pos, neg, cnt);
    focal_term(xv.z, gv.z, pos, neg, cnt);
    focal_term(xv.w, gv.w, pos, neg, cnt);
  }
  for (int64_t i = nq * 4 + t; i < n; i += stride) focal_term(x[i], g[i], pos, neg, cnt);
  __shared__ double s_w[CW][3];
  pos = wave_sum_d(pos);
  neg = wave_sum_d(neg);
  cnt = wave_sum_d(cnt);
  if (lane_id() == 0) {
    s_w[threadIdx.x >> 6][0] = pos;
    s_w[threadIdx.x >> 6][1] = neg;
    s_w[threadIdx.x >> 6][2] = cnt;
  }
  __syncthreads();
  if (threadIdx.x < 3) {
    double v = s_w[0][threadIdx.x];
    for (int w = 1; w < CW; ++w) v += s_w[w][threadIdx.x];
    partials[((size_t)h * PARTS + part) * 3 + threadIdx.x] = v;
  }
}

// cell of slot k of (head h, sample b), -1 unless the slot counts
__device__ __forceinline__ int slot_cell(const ClMaps &a, int h, int b, int k) {
  const size_t i = (size_t)b * a.n_max + k;
  if (a.mask[h][i] == 0) return -1;
  const long long c = a.ind[h][i];
  return c >= 0 && c < a.hw ? (int)c : -1;
}

__device__ __forceinline__ size_t reg_at(const ClMaps &a, int b, int d, int cell) {
  return ((size_t)b * a.reg_ch[a.ch_map[d]] + a.ch_idx[d]) * a.hw + cell;
}

// grid (n_heads * B).  |pred - target| of a tile of CT slots goes to LDS, one thread per slot; thread d then adds the tile's
// column d to its running fp64 sum in ascending slot order (a slot that does not count holds +0.0, which changes no sum).
__global__ __launch_bounds__(CT) void k_cl_reg(ClMaps a, double *__restrict__ regpart) {
  const int h = blockIdx.x / a.B, b = blockIdx.x % a.B;
  __shared__ double s_v[CT][NC + 1];                 // (+1: the column walk of thread d meets no bank twice in a row)
  double sum = 0.0;                                  // thread d < code: S_d; thread NC: the slots that count
  for (int k0 = 0; k0 < a.n_max; k0 += CT) {
    const int k = k0 + threadIdx.x;
    const int cell = k < a.n_max ? slot_cell(a, h, b, k) : -1;
#pragma unroll 1
    for (int d = 0; d < a.code; ++d) {               // (not unrolled: sixteen channels' addresses at once spill SGPRs)
      double v = 0.0;
      if (cell >= 0) {
        const float tv = a.tgt[h][((size_t)b * a.n_max + k) * a.code + d];
        if (tv == tv) v = fabs((double)a.reg[h][a.ch_map[d]][reg_at(a, b, d, cell)] - (double)tv);
      }
      s_v[threadIdx.x][d] = v;
    }
    s_v[threadIdx.x][NC] = cell >= 0 ? 1.0 : 0.0;
    __syncthreads();
    if ((int)threadIdx.x < a.code || threadIdx.x == NC) {
      const int n = a.n_max - k0 < CT ? a.n_max - k0 : CT;
      for (int i = 0; i < n; ++i) sum += s_v[i][threadIdx.x];
    }
    __syncthreads();
  }
  if ((int)threadIdx.x < a.code || threadIdx.x == NC) regpart[(size_t)blockIdx.x * (NC + 1) + threadIdx.x] = sum;
}

// one workgroup of 64: thread h finishes head h, thread 0 the total
__global__ __launch_bounds__(64) void k_cl_final(ClMaps a, const double *__restrict__ partials,
                                                 const double *__restrict__ regpart, float *__restrict__ losses,
                                                 float *__restrict__ chan, double *__restrict__ stats) {
  __shared__ float s_hm[NH], s_loc[NH];
  const int h = threadIdx.x;
  if (h < a.n_heads) {
    double pos = 0.0, neg = 0.0, npos = 0.0;
    if (a.hm[h]) {
      for (int i = 0; i < a.parts[h]; ++i) {
        const double *p = partials + ((size_t)h * PARTS + i) * 3;
        pos += p[0];
        neg += p[1];
        npos += p[2];
      }
    }
    const double hm = npos > 0.0 ? -(pos + neg) / npos : -neg;
    s_hm[h] = (float)(hm * a.w[0]);
    double num = 0.0, loc = 0.0;
    if (a.n_reg > 0) {
      for (int b = 0; b < a.B; ++b) num += regpart[((size_t)h * a.B + b) * (NC + 1) + NC];
      const double den = num > 1.0 ? num : 1.0;
      for (int d = 0; d < a.code; ++d) {
        double s = 0.0;
        for (int b = 0; b < a.B; ++b) s += regpart[((size_t)h * a.B + b) * (NC + 1) + d];
        const double l = s / den;
        chan[h * a.code + d] = (float)l;
        loc += a.w[2 + d] * l;
      }
    }
    s_loc[h] = (float)(a.w[1] * loc);
    stats[2 * h] = npos;
    stats[2 * h + 1] = num;
    losses[2 * h] = s_hm[h];
    losses[2 * h + 1] = s_loc[h];
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    float total = 0.0f;
    for (int i = 0; i < a.n_heads; ++i) total = total + (s_hm[i] + s_loc[i]);
    losses[2 * a.n_heads] = total;
  }
}

// grid (blocks, n_heads), grid-stride over a head's heat map
__global__ __launch_bounds__(CT) void k_cl_hm_bwd(ClMaps a, ClGrads o, const float *__restrict__ grad_losses,
                                                  const double *__restrict__ stats) {
  const int h = blockIdx.y;
  float *__restrict__ out = o.hm[h];
  if (!out) return;
  const float *__restrict__ x = a.hm[h];
  const float *__restrict__ g = a.heat[h];
  const double up = grad_losses ? (double)grad_losses[2 * h] + (double)grad_losses[2 * a.n_heads] : 0.0;
  const double npos = stats[2 * h];
  const double scale = npos > 0.0 ? -(up * a.w[0]) / npos : -(up * a.w[0]);
  const int64_t n = (int64_t)a.B * a.n_cls[h] * a.hw;
  const bool vec = aligned16(x, g) && aligned16(out, out);
  const int64_t nq = n / 4;
  const int64_t t = (int64_t)blockIdx.x * CT + threadIdx.x, stride = (int64_t)gridDim.x * CT;
  for (int64_t q = t; q < nq; q += stride) {
    float4 xv, gv, r;
    if (vec) {
      xv = ((const float4 *)x)[q];
      gv = ((const float4 *)g)[q];
    } else {
      xv = make_float4(x[4 * q], x[4 * q + 1], x[4 * q + 2], x[4 * q + 3]);
      gv = make_float4(g[4 * q], g[4 * q + 1], g[4 * q + 2], g[4 * q + 3]);
    }
    r.x = focal_grad(xv.x, gv.x, scale);
    r.y = focal_grad(xv.y, gv.y, scale);
    r.z = focal_grad(xv.z, gv.z, scale);
    r.w = focal_grad(xv.w, gv.w, scale);
    if (vec) {
      ((float4 *)out)[q] = r;
    } else {
      out[4 * q] = r.x, out[4 * q + 1] = r.y, out[4 * q + 2] = r.z, out[4 * q + 3] = r.w;
    }
  }
  for (int64_t i = nq * 4 + t; i < n; i += stride) out[i] = focal_grad(x[i], g[i], scale);
}

// zero p[0, n): scalar stores up to the first 16-byte boundary, 16-byte stores, a scalar tail
__device__ __forceinline__ void zero_span(float *__restrict__ p, int n) {
  int head = (int)(((16u - (unsigned)((uintptr_t)p & 15u)) & 15u) / 4u);
  head = head < n ? head : n;
  const int nq = (n - head) / 4;
  float4 *q = (float4 *)(p + head);
  for (int i = threadIdx.x; i < nq; i += CT) q[i] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  const int done = head + nq * 4;
  if ((int)threadIdx.x < head) p[threadIdx.x] = 0.0f;
  if ((int)threadIdx.x < n - done) p[done + threadIdx.x] = 0.0f;
}

// grid (spans of SPAN cells, n_heads * B)
__global__ __launch_bounds__(CT) void k_cl_reg_bwd(ClMaps a, ClGrads o, const float *__restrict__ grad_losses,
                                                   const float *__restrict__ grad_chan,
                                                   const double *__restrict__ stats) {
  const int h = blockIdx.y / a.B, b = blockIdx.y % a.B;
  const int c0 = blockIdx.x * SPAN, c1 = c0 + SPAN < a.hw ? c0 + SPAN : a.hw;
  __shared__ int s_cell[DFU3D_HEAD_MAX_OBJS];
  __shared__ float s_scale[NC];
  for (int d = 0; d < a.code; ++d) {
    float *m = o.reg[h][a.ch_map[d]];
    if (m) zero_span(m + reg_at(a, b, d, c0), c1 - c0);
  }
  for (int k = threadIdx.x; k < a.n_max; k += CT) s_cell[k] = slot_cell(a, h, b, k);
  if ((int)threadIdx.x < a.code) {
    const int d = threadIdx.x;
    const double up = grad_losses ? (double)grad_losses[2 * h + 1] + (double)grad_losses[2 * a.n_heads] : 0.0;
    const double gc = grad_chan ? (double)grad_chan[h * a.code + d] : 0.0;
    const double num = stats[2 * h + 1];
    s_scale[d] = (float)((up * a.w[1] * a.w[2 + d] + gc) / (num > 1.0 ? num : 1.0));
  }
  __syncthreads();                                   // the zeroes of this span are written before any of its targets
  for (int k = threadIdx.x; k < a.n_max; k += CT) {
    const int cell = s_cell[k];
    if (cell < c0 || cell >= c1) continue;
    bool lowest = true;
    for (int j = 0; j < k; ++j) lowest = lowest && s_cell[j] != cell;
    if (!lowest) continue;
#pragma unroll 1
    for (int d = 0; d < a.code; ++d) {               // (not unrolled, as in k_cl_reg)
      float *m = o.reg[h][a.ch_map[d]];
      if (!m) continue;
      const size_t at = reg_at(a, b, d, cell);
      const float pred = a.reg[h][a.ch_map[d]][at], sc = s_scale[d];
      float acc = 0.0f;
      for (int j = k; j < a.n_max; ++j) {
        if (s_cell[j] != cell) continue;
        const float tv = a.tgt[h][((size_t)b * a.n_max + j) * a.code + d];
        if (tv == tv) {
          const float diff = pred - tv;
          acc = acc + (float)((diff > 0.0f) - (diff < 0.0f)) * sc;
        }
      }
      m[at] = acc;
    }
  }
}

// host: arguments -> ClMaps; DFU3D_OK or the error
int cl_fill(ClMaps &a, const uint64_t *maps, const int32_t *n_cls, int32_t n_heads, int32_t batch, int32_t hw,
            const int32_t *reg_ch, int32_t n_reg, int32_t n_max, const double *weights) {
  if (!maps || !n_cls || !weights || n_heads < 1 || batch < 1 || hw < 1 || n_reg < 0 || n_max < 0) return DFU3D_EINVAL;
  if (n_reg > 0 && (!reg_ch || n_max < 1)) return DFU3D_EINVAL;
  if (n_heads > NH || n_reg > NM || n_max > DFU3D_HEAD_MAX_OBJS) return DFU3D_ERANGE;
  a = ClMaps{};
  int code = 0;
  for (int m = 0; m < n_reg; ++m) {
    if (reg_ch[m] < 1) return DFU3D_EINVAL;
    if (code + reg_ch[m] > NC) return DFU3D_ERANGE;
    a.reg_ch[m] = reg_ch[m];
    for (int c = 0; c < reg_ch[m]; ++c) {
      a.ch_map[code] = m;
      a.ch_idx[code++] = c;
    }
  }
  if ((int64_t)batch * (code > 1 ? code : 1) * hw > 0x7FFFFFFF) return DFU3D_ERANGE;
  a.n_heads = n_heads, a.B = batch, a.hw = hw, a.n_reg = n_reg, a.n_max = n_max, a.code = code;
  for (int i = 0; i < 2 + code; ++i) a.w[i] = weights[i];
  for (int h = 0; h < n_heads; ++h) {
    const uint64_t *row = maps + (size_t)h * DFU3D_HEAD_FWD_PTRS;
    a.hm[h] = (const float *)(uintptr_t)row[0];
    a.heat[h] = (const float *)(uintptr_t)row[1];
    if (!a.hm[h] != !a.heat[h]) return DFU3D_EINVAL;
    if (!a.hm[h] && n_reg == 0) return DFU3D_EINVAL;
    if (a.hm[h]) {
      if (n_cls[h] < 1) return DFU3D_EINVAL;
      const int64_t n = (int64_t)batch * n_cls[h] * hw;
      if (n > 0x7FFFFFFF) return DFU3D_ERANGE;
      const int64_t parts = (n + FOCAL_PER_PART - 1) / FOCAL_PER_PART;
      a.n_cls[h] = n_cls[h];
      a.parts[h] = (int)(parts < PARTS ? parts : PARTS);
    }
    if (n_reg > 0) {
      a.tgt[h] = (const float *)(uintptr_t)row[2];
      a.ind[h] = (const long long *)(uintptr_t)row[3];
      a.mask[h] = (const long long *)(uintptr_t)row[4];
      if (!a.tgt[h] || !a.ind[h] || !a.mask[h]) return DFU3D_EINVAL;
      for (int m = 0; m < n_reg; ++m) {
        a.reg[h][m] = (const float *)(uintptr_t)row[5 + m];
        if (!a.reg[h][m]) return DFU3D_EINVAL;
      }
    }
  }
  return DFU3D_OK;
}

}  // namespace

extern "C" int32_t dfu3d_head_version(void) { return DFU3D_HEAD_VERSION; }

// (`code` is validated only: the layout reserves DFU3D_HEAD_MAX_CODE + 1 doubles per (head, sample) whatever the code
// length, so that a row's place does not depend on it)
extern "C" int64_t dfu3d_center_loss_scratch_bytes(int32_t n_heads, int32_t batch, int32_t code) {
  if (n_heads < 1 || n_heads > NH || batch < 1 || code < 0 || code > NC) return -1;
  return (int64_t)cl_scratch(n_heads, batch).bytes;
}

extern "C" int dfu3d_center_loss_fwd(const uint64_t *maps, const int32_t *n_cls, int32_t n_heads, int32_t batch,
                                     int32_t hw, const int32_t *reg_ch, int32_t n_reg, int32_t n_max,
                                     const double *weights, float *losses, float *chan, double *stats, void *scratch,
                                     int64_t scratch_bytes, void *stream) {
  DFU3D_CLEAR_STALE_ERROR();
  if (!losses || !chan || !stats || !scratch) return DFU3D_EINVAL;
  ClMaps a;
  const int rc = cl_fill(a, maps, n_cls, n_heads, batch, hw, reg_ch, n_reg, n_max, weights);
  if (rc != DFU3D_OK) return rc;
  const ClScratch L = cl_scratch(n_heads, batch);
  if (((uintptr_t)scratch & 15u) || scratch_bytes < (int64_t)L.bytes) return DFU3D_EINVAL;
  double *partials = (double *)((char *)scratch + L.focal), *regpart = (double *)((char *)scratch + L.reg);
  hipStream_t st = (hipStream_t)stream;
  int max_parts = 0;
  for (int h = 0; h < n_heads; ++h) max_parts = a.parts[h] > max_parts ? a.parts[h] : max_parts;
  if (max_parts > 0) {
    hipLaunchKernelGGL(k_cl_focal, dim3(max_parts, n_heads), dim3(CT), 0, st, a, partials);
    DFU3D_LAUNCH_CHECK();
  }
  if (n_reg > 0) {
    hipLaunchKernelGGL(k_cl_reg, dim3(n_heads * batch), dim3(CT), 0, st, a, regpart);
    DFU3D_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(k_cl_final, dim3(1), dim3(64), 0, st, a, partials, regpart, losses, chan, stats);
  DFU3D_LAUNCH_CHECK();
  return DFU3D_OK;
}

extern "C" int dfu3d_center_loss_bwd(const uint64_t *maps, const uint64_t *grads, const int32_t *n_cls,
                                     int32_t n_heads, int32_t batch, int32_t hw, const int32_t *reg_ch, int32_t n_reg,
                                     int32_t n_max, const double *weights, const float *grad_losses,
                                     const float *grad_chan, const double *stats, void *stream) {
  DFU3D_CLEAR_STALE_ERROR();
  if (!grads || !stats) return DFU3D_EINVAL;
  ClMaps a;
  const int rc = cl_fill(a, maps, n_cls, n_heads, batch, hw, reg_ch, n_reg, n_max, weights);
  if (rc != DFU3D_OK) return rc;
  ClGrads o = ClGrads{};
  int64_t max_n = 0;
  bool any_hm = false, any_reg = false;
  for (int h = 0; h < n_heads; ++h) {
    const uint64_t *row = grads + (size_t)h * DFU3D_HEAD_BWD_PTRS;
    o.hm[h] = a.hm[h] ? (float *)(uintptr_t)row[0] : nullptr;
    if (o.hm[h]) {
      const int64_t n = (int64_t)batch * a.n_cls[h] * hw;
      max_n = n > max_n ? n : max_n;
      any_hm = true;
    }
    for (int m = 0; m < n_reg; ++m) {
      o.reg[h][m] = (float *)(uintptr_t)row[1 + m];
      any_reg = any_reg || o.reg[h][m];
    }
  }
  hipStream_t st = (hipStream_t)stream;
  if (any_hm) {
    const int64_t blocks = (max_n + 4 * CT - 1) / (4 * CT);
    hipLaunchKernelGGL(k_cl_hm_bwd, dim3((unsigned)(blocks < 1024 ? blocks : 1024), n_heads), dim3(CT), 0, st, a, o,
                       grad_losses, stats);
    DFU3D_LAUNCH_CHECK();
  }
  if (any_reg) {
    hipLaunchKernelGGL(k_cl_reg_bwd, dim3((hw + SPAN - 1) / SPAN, n_heads * batch), dim3(CT), 0, st, a, o, grad_losses,
                       grad_chan, stats);
    DFU3D_LAUNCH_CHECK();
  }
  return DFU3D_OK;
}
