/* dfu3d_head.h -- C ABI of the CenterHead loss stage of libdfu3d_hip.so (csrc/centerloss_stage.hip): the focal loss of
 * the heat maps and the L1 loss of the regression maps at the target cells, forward and backward, for all heads and
 * samples in one launch chain per direction.
 *
 * The entry points live in the same library as include/dfu3d.h's and follow its rules: device pointers, results in
 * device memory, the library never allocates and never synchronises, every call returns DFU3D_OK / DFU3D_EINVAL /
 * DFU3D_ELAUNCH / DFU3D_ERANGE (dfu3d.h) and validates its arguments on the host before any launch.  The header keeps
 * to the C subset dfu3d_amd/_header.py reads.
 *
 * Per-head tensors are separate allocations.  Their device addresses arrive in HOST arrays of uint64 (`maps`, `grads`);
 * the library copies them into the kernel arguments, so no table is copied to the device.
 *   maps : n_heads rows of DFU3D_HEAD_FWD_PTRS = [hm, heat, target, ind, mask, reg_0 .. reg_4]
 *          hm (B, n_cls, H, W) float32 logits, heat the same shape (targets in [0, 1]); target (B, n_max, code) float32;
 *          ind, mask (B, n_max) int64; reg_m (B, reg_ch[m], H, W) float32, the code's channels in map order.
 *          hm = heat = 0: the head has no focal part.  n_reg = 0: no regression part (target, ind, mask unused).
 *   grads: n_heads rows of DFU3D_HEAD_BWD_PTRS = [grad_hm, grad_reg_0 .. grad_reg_4]; a null entry is not written.
 * weights (host doubles): [cls_weight, loc_weight, code_weights[code]].
 *
 * Numerics: p = clamp(float32(sigmoid(x)), 1e-4f, float32(1 - 1e-4)), the sigmoid and both focal terms in fp64; all sums
 * in fp64 with a fixed shape that depends on the tensors' shapes alone, not on their alignment (heat maps: workgroup
 * partials, then one workgroup in index order; |pred - target|: in slot order, then the samples in order); every result
 * rounded to float32 once.  No float atomics: results are the same bits on every run.
 */
#ifndef DFU3D_HEAD_H
#define DFU3D_HEAD_H

#include <stdint.h>

#define DFU3D_HEAD_VERSION 100

#define DFU3D_HEAD_MAX_HEADS 8
#define DFU3D_HEAD_MAX_REG_MAPS 5
/* channels of all regression maps of a head together (= columns of target) at most */
#define DFU3D_HEAD_MAX_CODE 16
/* NUM_MAX_OBJS at most */
#define DFU3D_HEAD_MAX_OBJS 1024
/* workgroup partials of a head's focal sums at most */
#define DFU3D_HEAD_PARTS 64
#define DFU3D_HEAD_FWD_PTRS (5 + 5)
#define DFU3D_HEAD_BWD_PTRS (1 + 5)

#ifdef __cplusplus
extern "C" {
#endif

int32_t dfu3d_head_version(void);

/* bytes of scratch dfu3d_center_loss_fwd needs (16-byte aligned); -1 for an argument out of range */
int64_t dfu3d_center_loss_scratch_bytes(int32_t n_heads, int32_t batch, int32_t code);

/* Forward.  losses (2 n_heads + 1) = [hm_loss_0, loc_loss_0, ..., total]:
 *   hm_loss_h  = float32(cls_weight * (num_pos > 0 ? -(S_pos + S_neg) / num_pos : -S_neg))
 *   loc_loss_h = float32(loc_weight * sum_d code_weights[d] * (S_d / max(num, 1)))
 *   total      = the float32 sum of (hm_loss_h + loc_loss_h) in head order
 * chan (n_heads, code) = float32(S_d / max(num, 1)); stats (n_heads, 2) double = {num_pos, num}.
 * A slot counts iff mask != 0 and 0 <= ind < H * W; a channel of a slot whose target is NaN is skipped. */
int dfu3d_center_loss_fwd(const uint64_t *maps, const int32_t *n_cls, int32_t n_heads, int32_t batch, int32_t hw,
                          const int32_t *reg_ch, int32_t n_reg, int32_t n_max, const double *weights, float *losses,
                          float *chan, double *stats, void *scratch, int64_t scratch_bytes, void *stream);

/* Backward, recomputed from the inputs and `stats`.  grad_losses (2 n_heads + 1) and grad_chan (n_heads, code) are the
 * upstream gradients of the two outputs in DEVICE memory; either may be null (zero).  Every cell of every gradient map
 * is written: grad_hm = float32 of the fp64 element gradient, zero where the clamp is active; grad_reg zero except at
 * the target cells, where the lowest slot of a cell sums sign(pred - target) * s_d over the valid slots of that cell
 * in ascending slot order, s_d = float32(((g_loc_h + g_total) * loc_weight * code_weights[d] + grad_chan[h][d]) /
 * max(num, 1)). */
int dfu3d_center_loss_bwd(const uint64_t *maps, const uint64_t *grads, const int32_t *n_cls, int32_t n_heads,
                          int32_t batch, int32_t hw, const int32_t *reg_ch, int32_t n_reg, int32_t n_max,
                          const double *weights, const float *grad_losses, const float *grad_chan,
                          const double *stats, void *stream);

#ifdef __cplusplus
}
#endif

#endif
