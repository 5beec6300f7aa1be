/* merl_hip_diff.h — the differentiation extension of the C ABI of libmerl_hip.so: the gradient of eval in the directions.
 * It includes merl_hip.h (contexts, materials, status codes, mrl_eval_batch, mrl_eval_queue) and adds to it; the library exports
 * both sets.  The gradients in the material live in merl_hip_fit.h (mrl_ggx_grad_batch) and merl_hip.h (mrl_table_grad_batch); the
 * direction gradient on table materials lives in merl_hip_diff_table.h.
 * Calls added here are listed in host.DIFF_ABI_SYMBOLS and checked against this header by tests/test_ggx_dir_grad_cpu.py. */
#ifndef MERL_HIP_DIFF_H
#define MERL_HIP_DIFF_H

#include "merl_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- the direction gradient of eval on GGX conductors ----
 * Let E_c(wi, wo) be the real-valued function mrl_eval_batch computes for a GGX id — F_c D G1(i) G1(o) / (4 cos(theta_i)), the
 * cosine of wo folded in, at the material's stored Float parameters, evaluated in f64 from the Float inputs, the normalisation of
 * wi and wo INCLUDED.  Per unit u the calls compute the vector-Jacobian products
 *     grad_wi[u] = sum_c grad_rgb[u][c] dE_c / d wi          grad_wo[u] = sum_c grad_rgb[u][c] dE_c / d wo
 * — what the backward pass of a differentiable renderer hands on to its normal-map, shading-frame, pose and geometry gradients.
 * wi, wo, grad_rgb, grad_wi, grad_wo: [n][3] f32.  The outputs are OVERWRITTEN per unit, like eval's, not accumulated into.
 * E is homogeneous of degree 0 in each direction, so
 *   - each gradient is orthogonal to its own direction: grad_wi[u] . wi[u] = 0, grad_wo[u] . wo[u] = 0 (to rounding);
 *   - for unnormalised inputs it scales with 1 / |w|: scaling wi by s divides grad_wi by s and leaves grad_wo as it is.
 * Dead units: a unit that eval masks (cos(theta_i) <= 0, cos(theta_o) <= 0, a NaN / inf / zero-length direction), or for which one
 * of eval's own D / G1 selects returns 0, gets exactly +0.0f in both outputs, whatever its grad_rgb holds (NaN and inf included).
 * Materials: mat == NULL: every unit uses single_id, which must be a live GGX material (MRL_ERR_MATERIAL otherwise).  mat != NULL:
 * one id per unit; a unit whose id names no live GGX material (out of range, negative, released, a table, n-channel, RGL or spectral
 * material) gets zeros, as the RGB batch calls treat unknown ids.
 * One of grad_wi / grad_wo may be NULL: that gradient is then neither computed nor written; both NULL: MRL_ERR_INVALID.  NULL wi,
 * wo or grad_rgb: MRL_ERR_INVALID.  Pointers all host or all device (MRL_ERR_POINTER_MIX).  Device pointers: asynchronous on the
 * context's stream; no workspace, no reduction, no atomics.  n == 0 / capacity == 0: MRL_OK, nothing is touched.
 * mrl_ggx_grad_dir_batch takes host arrays as well, through the staged chunk loop (MRL_OPT_HOST_CHUNK), mat included.
 * mrl_ggx_grad_dir_queue follows mrl_eval_queue: device pointers only; it processes the slots queue[0 .. min(*queue_count,
 * capacity)), reads a slot's inputs from and writes its outputs to the slot named, leaves every other slot untouched;
 * capacity <= 2^32; capturable in a HIP graph (the count is read on the device at run time).
 * DETERMINISM (a contract of these calls): a unit's output bits depend on its own inputs and its material's parameters alone —
 * the whole-array, material-id, queue and host-array forms return identical bits for the same unit, whatever n, the grid or the
 * unit's position, and grad_wi has the same bits with and without grad_wo.
 * Not offered here: RGB table materials have the same pair of calls in merl_hip_diff_table.h (mrl_table_grad_dir_batch / _queue),
 * n-channel tables in merl_hip_diff_nch.h (mrl_table_grad_dir_batch_nch / _queue_nch).
 * RGB RGL materials in merl_hip_diff_rgl.h (mrl_rgl_grad_dir_batch / _queue).
 * Not offered: spectral RGL materials, device groups (mrl_group_*), the one-unit paths, second derivatives.
 * The gradients of pdf and sample on GGX conductors live in merl_hip_diff_sample.h (mrl_ggx_pdf_grad_batch, mrl_ggx_sample_grad_batch). */
int mrl_ggx_grad_dir_batch(mrl_ctx *ctx, const float *wi, const float *wo, const float *grad_rgb,
                           const int32_t *mat, int32_t single_id, size_t n,
                           float *grad_wi, float *grad_wo);
int mrl_ggx_grad_dir_queue(mrl_ctx *ctx, const float *wi, const float *wo, const float *grad_rgb,
                           const int32_t *mat, int32_t single_id,
                           const uint32_t *queue, const uint32_t *queue_count, size_t capacity,
                           float *grad_wi, float *grad_wo);

#ifdef __cplusplus
}
#endif
#endif
