// optim_stage.hip -- SURVEY.md §8 row f-12: the optimiser step of the `adam_onecycle` recipe (include/dfu3d_opt.h).
//
// What it stands in for in the reference: tools/train_utils/train_utils.py's clip_grad_norm_ (a norm per tensor, a norm
// of norms, a multiply per tensor), OptimWrapper.step's true weight decay (a multiply per parameter in a Python loop)
// and torch.optim.Adam over two parameter groups.  Here one tensor table and one chunk map describe every parameter,
// and the whole step is three launches:
//
//   k_opt_sumsq  one workgroup per chunk: the fp64 sum of the squares of the chunk's gradient elements in the fixed shape
//                of the header's contract -> partial[chunk] (0 for a tensor without a gradient).
//   k_opt_total  one wave: the partials added one after the other in chunk order (a coalesced load of 64, then 64
//                dependent adds fed by lane reads), total_norm, coef, the status bit.
//   k_opt_step   one workgroup per chunk: clip, decay and the Adam update of the header's contract; 16-byte loads and
//                stores of four consecutive floats per lane where every address of the tensor is 16-byte aligned, single
//                words for a tensor that is only 4-byte aligned and for the tail of a tensor.  grad is read only.
// Both chunk kernels give thread t the elements 4 * (t + 256 * k) .. + 3 on either path, so the sum does not depend on
// the path.
#include <math.h>

#include "common.hpp"
#include "dfu3d_opt.h"

namespace {

constexpr int OT = DFU3D_OPT_THREADS;
constexpr int CHUNK = DFU3D_OPT_CHUNK;
constexpr int QUADS = CHUNK / (4 * OT);            // float4 per thread and chunk
static_assert(CHUNK == 4 * OT * QUADS && OT % 64 == 0, "a chunk is whole float4 rounds of the workgroup");
static_assert(sizeof(dfu3d_opt_tensor) == 40 && sizeof(dfu3d_opt_chunk) == 8, "records of dfu3d_opt.h");

struct StepConst { float decay, b1, omb1, b2, omb2, step_size, sqrt_bc2, eps; };

// elements of the chunk (0 when the record is not one of this table's), and its tensor in T
__device__ __forceinline__ int chunk_of(const dfu3d_opt_tensor *__restrict__ table, int n_tensors,
                                        const dfu3d_opt_chunk *__restrict__ chunks, dfu3d_opt_tensor &T, int &start) {
  const dfu3d_opt_chunk ck = chunks[blockIdx.x];
  if ((unsigned)ck.tensor >= (unsigned)n_tensors || ck.start < 0) return 0;
  T = table[ck.tensor];
  start = ck.start;
  const int64_t rest = T.n - (int64_t)ck.start;
  return rest <= 0 ? 0 : (rest < CHUNK ? (int)rest : CHUNK);
}

__global__ __launch_bounds__(OT) void k_opt_sumsq(const dfu3d_opt_tensor *__restrict__ table, int n_tensors,
                                                  const dfu3d_opt_chunk *__restrict__ chunks,
                                                  double *__restrict__ partial) {
  __shared__ double s_w[OT / 64];
  dfu3d_opt_tensor T = {};
  int start = 0;
  const int len = chunk_of(table, n_tensors, chunks, T, start);
  double acc = 0.0;
  if (len > 0 && T.grad) {
    const float *g = (const float *)T.grad + start;
    const bool vec = (T.grad & 15u) == 0;
#pragma unroll
    for (int k = 0; k < QUADS; k++) {
      const int i = 4 * ((int)threadIdx.x + OT * k);
      float x0 = 0.f, x1 = 0.f, x2 = 0.f, x3 = 0.f;
      if (vec && i + 3 < len) {
        const float4 q = *reinterpret_cast<const float4 *>(g + i);
        x0 = q.x; x1 = q.y; x2 = q.z; x3 = q.w;
      } else {
        if (i < len) x0 = g[i];
        if (i + 1 < len) x1 = g[i + 1];
        if (i + 2 < len) x2 = g[i + 2];
        if (i + 3 < len) x3 = g[i + 3];
      }
      acc += (double)x0 * (double)x0;
      acc += (double)x1 * (double)x1;
      acc += (double)x2 * (double)x2;
      acc += (double)x3 * (double)x3;
    }
  }
  acc = block_sum_d<OT / 64>(acc, s_w);
  if (threadIdx.x == 0) partial[blockIdx.x] = acc;
}

__global__ __launch_bounds__(64) void k_opt_total(const double *__restrict__ partial, int n_chunks, double max_norm,
                                                  double *__restrict__ out_norm, uint32_t *__restrict__ status) {
  const int lane = threadIdx.x;
  double s = 0.0;
  for (int base = 0; base < n_chunks; base += 64) {
    const double x = base + lane < n_chunks ? partial[base + lane] : 0.0;     // s >= +0 or NaN: adding +0.0 keeps its bits
#pragma unroll
    for (int k = 0; k < 64; k++) s += readlane_d(x, k);
  }
  if (lane == 0) {
    const double total_norm = sqrt(s);
    const double c = max_norm / (total_norm + 1e-6);
    out_norm[0] = total_norm;
    out_norm[1] = (double)(float)(c > 1.0 ? 1.0 : c);            // a NaN stays one, as under the reference's clamp
    if (!(fabs(s) <= 1.7976931348623157e308)) atomicOr(status, (uint32_t)DFU3D_OPT_ST_NONFINITE);
  }
}

__device__ __forceinline__ void adam_element(float g, float coef, const StepConst &c, float &p, float &m, float &v) {
  const float g1 = g * coef;
  const float p1 = p * c.decay;
  const float m1 = c.b1 * m + c.omb1 * g1;
  const float v1 = c.b2 * v + c.omb2 * (g1 * g1);
  const float d = sqrtf(v1) / c.sqrt_bc2 + c.eps;
  p = p1 - c.step_size * (m1 / d);
  m = m1;
  v = v1;
}

__global__ __launch_bounds__(OT) void k_opt_step(const dfu3d_opt_tensor *__restrict__ table, int n_tensors,
                                                 const dfu3d_opt_chunk *__restrict__ chunks,
                                                 const double *__restrict__ out_norm, StepConst c) {
  dfu3d_opt_tensor T = {};
  int start = 0;
  const int len = chunk_of(table, n_tensors, chunks, T, start);
  if (len <= 0) return;
  float *p = (float *)T.param + start;
  if (!T.grad) {                                      // true weight decay only
    const bool vec = (T.param & 15u) == 0;
#pragma unroll
    for (int k = 0; k < QUADS; k++) {
      const int i = 4 * ((int)threadIdx.x + OT * k);
      if (vec && i + 3 < len) {
        float4 q = *reinterpret_cast<float4 *>(p + i);
        q.x *= c.decay; q.y *= c.decay; q.z *= c.decay; q.w *= c.decay;
        *reinterpret_cast<float4 *>(p + i) = q;
      } else {
        for (int j = i; j < i + 4 && j < len; j++) p[j] = p[j] * c.decay;
      }
    }
    return;
  }
  const float coef = (float)out_norm[1];
  const float *g = (const float *)T.grad + start;
  float *m = (float *)T.exp_avg + start, *v = (float *)T.exp_avg_sq + start;
  const bool vec = ((T.param | T.grad | T.exp_avg | T.exp_avg_sq) & 15u) == 0;
#pragma unroll
  for (int k = 0; k < QUADS; k++) {
    const int i = 4 * ((int)threadIdx.x + OT * k);
    if (vec && i + 3 < len) {
      const float4 gq = *reinterpret_cast<const float4 *>(g + i);
      float4 pq = *reinterpret_cast<float4 *>(p + i);
      float4 mq = *reinterpret_cast<float4 *>(m + i);
      float4 vq = *reinterpret_cast<float4 *>(v + i);
      adam_element(gq.x, coef, c, pq.x, mq.x, vq.x);
      adam_element(gq.y, coef, c, pq.y, mq.y, vq.y);
      adam_element(gq.z, coef, c, pq.z, mq.z, vq.z);
      adam_element(gq.w, coef, c, pq.w, mq.w, vq.w);
      *reinterpret_cast<float4 *>(p + i) = pq;
      *reinterpret_cast<float4 *>(m + i) = mq;
      *reinterpret_cast<float4 *>(v + i) = vq;
    } else {
      for (int j = i; j < i + 4 && j < len; j++) {
        float pj = p[j], mj = m[j], vj = v[j];
        adam_element(g[j], coef, c, pj, mj, vj);
        p[j] = pj;
        m[j] = mj;
        v[j] = vj;
      }
    }
  }
}

bool finite_d(double x) { return x - x == 0.0; }

}  // namespace

extern "C" int32_t dfu3d_opt_version(void) { return DFU3D_OPT_VERSION; }

extern "C" int64_t dfu3d_opt_scratch_bytes(int64_t n_chunks) {
  if (n_chunks < 1 || n_chunks > DFU3D_OPT_MAX_CHUNKS) return -1;
  return n_chunks * (int64_t)sizeof(double);
}

extern "C" int dfu3d_adam_step(const void *table, int32_t n_tensors, const void *chunks, int32_t n_chunks, double lr,
                               double beta1, double beta2, double eps, double weight_decay, double max_norm,
                               double bias_correction1, double bias_correction2, void *scratch, double *out_norm,
                               uint32_t *status, void *stream) {
  DFU3D_CLEAR_STALE_ERROR();
  if (!table || !chunks || !scratch || !out_norm || !status) return DFU3D_EINVAL;
  if ((((uintptr_t)table | (uintptr_t)chunks | (uintptr_t)scratch | (uintptr_t)out_norm) & 7u) || ((uintptr_t)status & 3u))
    return DFU3D_EINVAL;
  if (n_tensors < 1 || n_tensors > DFU3D_OPT_MAX_TENSORS || n_chunks < 1 || n_chunks > DFU3D_OPT_MAX_CHUNKS)
    return DFU3D_EINVAL;
  if (!finite_d(lr) || !finite_d(eps) || !finite_d(weight_decay) || !finite_d(max_norm)) return DFU3D_EINVAL;
  if (!(max_norm > 0.0) || !(lr >= 0.0) || !(eps >= 0.0)) return DFU3D_EINVAL;
  if (!(beta1 >= 0.0 && beta1 < 1.0) || !(beta2 >= 0.0 && beta2 < 1.0)) return DFU3D_EINVAL;
  if (!(bias_correction1 > 0.0 && bias_correction1 <= 1.0) || !(bias_correction2 > 0.0 && bias_correction2 <= 1.0))
    return DFU3D_EINVAL;
  StepConst c;
  c.decay = (float)(1.0 - weight_decay * lr);
  c.b1 = (float)beta1;
  c.omb1 = (float)(1.0 - beta1);
  c.b2 = (float)beta2;
  c.omb2 = (float)(1.0 - beta2);
  c.step_size = (float)(lr / bias_correction1);
  c.sqrt_bc2 = (float)sqrt(bias_correction2);
  c.eps = (float)eps;
  hipStream_t st = (hipStream_t)stream;
  const dfu3d_opt_tensor *tb = (const dfu3d_opt_tensor *)table;
  const dfu3d_opt_chunk *ck = (const dfu3d_opt_chunk *)chunks;
  double *partial = (double *)scratch;
  hipLaunchKernelGGL(k_opt_sumsq, dim3((unsigned)n_chunks), dim3(OT), 0, st, tb, (int)n_tensors, ck, partial);
  DFU3D_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_opt_total, dim3(1), dim3(64), 0, st, (const double *)partial, (int)n_chunks, max_norm, out_norm, status);
  DFU3D_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_opt_step, dim3((unsigned)n_chunks), dim3(OT), 0, st, tb, (int)n_tensors, ck, (const double *)out_norm, c);
  DFU3D_LAUNCH_CHECK();
  return DFU3D_OK;
}
