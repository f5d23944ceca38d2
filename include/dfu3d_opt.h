/* dfu3d_opt.h -- C ABI of the fused optimiser step of libdfu3d_hip.so (csrc/optim_stage.hip): gradient clipping by the
 * global norm, true weight decay and the Adam update of OpenPCDet's `adam_onecycle` recipe (clip_grad_norm_, the decay
 * loop of OptimWrapper.step, torch.optim.Adam) for every parameter tensor of a model in DFU3D_OPT_LAUNCHES launches.
 *
 * The entry points live in the same library as include/dfu3d.h's and follow its rules: device pointers, results in
 * device memory, the library never allocates and never synchronises, every call returns DFU3D_OK / DFU3D_EINVAL /
 * DFU3D_ELAUNCH / DFU3D_ERANGE (dfu3d.h) and validates its arguments on the host before any launch.  The header keeps
 * to the C subset dfu3d_amd/_header.py reads.
 *
 * NUMERICS CONTRACT
 *   S = sum of g * g over all elements of all tensors that have a gradient.  Every square is formed in fp64 (exact for
 *   float32 g) and summed in fp64 in a fixed shape: inside a chunk, thread t of 256 adds the elements
 *   4 * (t + 256 * k) + j (k = 0 .. 3 outer, j = 0 .. 3 inner, in this order; elements beyond the chunk count as +0.0),
 *   the 64 threads of a wave are added by the xor butterfly (distances 32, 16, .. 1), the four waves in wave order;
 *   then the chunk partials one after the other in chunk order.  The bits of S depend on the lengths and the values
 *   only -- not on the grid, on timing, on addresses or on the alignment path taken.  No float atomics.
 *   total_norm = sqrt(S) in fp64;  coef = (float) min(1.0, max_norm / (total_norm + 1e-6)).
 *   S not finite: DFU3D_OPT_ST_NONFINITE is ORed into the status word and the arithmetic goes on as defined (NaN
 *   spreads as in the reference); raising is the caller's business.
 *   On the host, in fp64, each rounded ONCE to float32:  decay = 1 - weight_decay * lr,  b1 = beta1,  omb1 = 1 - beta1,
 *   b2 = beta2,  omb2 = 1 - beta2,  step_size = lr / bias_correction1,  sqrt_bc2 = sqrt(bias_correction2),  eps.
 *   Per element of a tensor with a gradient, every operation ONE float32 operation rounded on its own (no contraction,
 *   correctly rounded division and square root):
 *       g1 = g * coef
 *       p1 = p * decay
 *       m1 = b1 * m + omb1 * g1
 *       v1 = b2 * v + omb2 * (g1 * g1)
 *       d  = sqrt(v1) / sqrt_bc2 + eps
 *       p2 = p1 - step_size * (m1 / d)
 *   p2, m1 and v1 are stored; grad is never written.  A tensor without a gradient (grad = 0 in its record) gets
 *   p = p * decay only: its moments are untouched and it adds nothing to S.
 */
#ifndef DFU3D_OPT_H
#define DFU3D_OPT_H

#include <stddef.h>
#include <stdint.h>

#define DFU3D_OPT_VERSION 1

/* elements of a chunk: the work of one workgroup of DFU3D_OPT_THREADS threads; a chunk never crosses a tensor */
#define DFU3D_OPT_CHUNK 4096
#define DFU3D_OPT_THREADS 256
/* kernel launches of one dfu3d_adam_step: the chunk sums, the total (one wave), the step */
#define DFU3D_OPT_LAUNCHES 3
/* tensors of a table: 1 .. DFU3D_OPT_MAX_TENSORS, else DFU3D_EINVAL */
#define DFU3D_OPT_MAX_TENSORS 65536
/* chunks of a call: 1 .. DFU3D_OPT_MAX_CHUNKS (2^32 elements), else DFU3D_EINVAL */
#define DFU3D_OPT_MAX_CHUNKS 1048576
/* elements of one tensor: 1 .. DFU3D_OPT_MAX_LEN (the caller's duty: the table is device memory) */
#define DFU3D_OPT_MAX_LEN 1073741824

/* bits of the status word */
#define DFU3D_OPT_ST_NONFINITE 1

/* One record of the tensor table, 40 bytes: device addresses of float32, contiguous arrays of n elements, each at least
 * 4-byte aligned; grad = 0: no gradient in this call. */
typedef struct dfu3d_opt_tensor {
  uint64_t param, grad, exp_avg, exp_avg_sq;
  int64_t n;
} dfu3d_opt_tensor;

/* One record of the chunk map, 8 bytes: the elements start .. min(start + DFU3D_OPT_CHUNK, n) - 1 of tensor `tensor`;
 * start is a multiple of DFU3D_OPT_CHUNK.  Tensor after tensor, starts ascending: n_chunks = sum of ceil(n_i / CHUNK). */
typedef struct dfu3d_opt_chunk {
  int32_t tensor, start;
} dfu3d_opt_chunk;

#ifdef __cplusplus
extern "C" {
#endif

int32_t dfu3d_opt_version(void);

/* bytes of the scratch of a call over n_chunks chunks (one double each); -1 for n_chunks < 1 or beyond DFU3D_OPT_MAX_CHUNKS */
int64_t dfu3d_opt_scratch_bytes(int64_t n_chunks);

/* table: n_tensors dfu3d_opt_tensor records, chunks: n_chunks dfu3d_opt_chunk records, both in device memory and
 * 8-byte aligned, built by the caller and trusted by the library (a wrong address in them is a GPU fault).
 * scratch: dfu3d_opt_scratch_bytes(n_chunks) bytes, 8-byte aligned; every double is written before it is read.
 * out_norm: two doubles, [total_norm, coef]; status: ORed into, never cleared.
 * DFU3D_EINVAL before any launch: max_norm <= 0 (or NaN), lr < 0, a beta outside [0, 1), a bias correction outside
 * (0, 1], eps < 0, a value that is not finite, n_tensors or n_chunks out of range, a null or misaligned table, chunks,
 * scratch, out_norm, a null status. */
int dfu3d_adam_step(const void *table, int32_t n_tensors, const void *chunks, int32_t n_chunks, double lr,
                    double beta1, double beta2, double eps, double weight_decay, double max_norm,
                    double bias_correction1, double bias_correction2, void *scratch, double *out_norm,
                    uint32_t *status, void *stream);

#ifdef __cplusplus
}
#endif

#endif
