/* merl_hip_diff_sample.h — the gradients of pdf and of sample on GGX conductors: what an MIS weight and an attached sampler hand back
 * to the shading frame, the pose and the roughness of a differentiable path tracer.  The sibling of merl_hip_diff.h (the gradient
 * of eval in the directions) and merl_hip_fit.h (the gradient of eval in the parameters).  It includes merl_hip.h (contexts,
 * materials, status codes, mrl_pdf_batch, mrl_sample_batch, mrl_eval_queue); the same library exports these calls.
 * Calls added here are listed in host.DIFF_SAMPLE_ABI_SYMBOLS and checked against this header by tests/test_ggx_sample_grad_cpu.py. */
#ifndef MERL_HIP_DIFF_SAMPLE_H
#define MERL_HIP_DIFF_SAMPLE_H

#include "merl_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- the gradient of pdf ----
 * Let P(wi, wo) be the real-valued function mrl_pdf_batch computes for a GGX id — D(m) G1(wi, m) / (4 cos(theta_i)), m the unit
 * half vector — at the material's stored Float alpha, evaluated in f64 from the Float inputs, the normalisation of wi and wo
 * INCLUDED.  Per unit u
 *     grad_wi[u] = grad_pdf[u] dP / d wi     grad_wo[u] = grad_pdf[u] dP / d wo     grad_alpha[u] = grad_pdf[u] dP / d alpha
 * wi, wo, grad_wi, grad_wo: [n][3] f32; grad_pdf, grad_alpha: [n] f32.  grad_alpha is PER UNIT on purpose: no reduction, no
 * workspace, no ordering — the caller sums it (in f64, over the units of each material).
 * Any output may be NULL: it is then neither computed into memory nor written; all three NULL: MRL_ERR_INVALID.
 * Dead units: a unit that pdf masks (cos(theta_i) <= 0, cos(theta_o) <= 0, a NaN / inf / zero-length direction), or for which one
 * of pdf's own D / G1 selects returns 0, gets exactly +0.0f in every output, whatever its grad_pdf holds (NaN and inf included).
 *
 * ---- the gradient of sample ----
 * Let (wo', p', w') be the real-valued function mrl_sample_batch computes for a GGX id BEFORE its results are rounded to Float:
 * wo' the direction reflected about the sampled visible normal, p' its pdf, w'[3] the weight F G1(wo').  It is differentiated on
 * the branch the forward call takes — all its selects are held fixed: the normal-incidence branch (stretched s_z >= 0.99999), the
 * s1 / s2 slope select, the sign select at u1 = 0.5, the |A| = 1 nudge — and u is held fixed.
 * grad_out: [n][7] f32 = (g_wo xyz, g_pdf, g_weight rgb), one packed array.  Per unit u, with y = (wo', p', w'):
 *     grad_wi[u]        = sum_j grad_out[u][j] d y_j / d wi                       [n][3] f32
 *     grad_params[u][p] = sum_j grad_out[u][j] d y_j / d p                        [n][7] f32
 * p in the order of merl_hip_fit.h: (alpha, eta rgb, k rgb), at the material's stored Float parameters; eta and k enter through
 * the weight only.  grad_params is PER UNIT, like grad_alpha above.  Either output may be NULL, not both (MRL_ERR_INVALID).
 * Dead units: a unit is dead exactly when the forward call rejects it, that is returns pdf = 0 — wi.z <= 0, a NaN / inf /
 * zero-length wi, a reflection below the horizon, wi . m <= 0, p' <= 0, a Float wo'.z that rounds to 0; it gets +0.0f everywhere,
 * whatever its grad_out holds.
 *
 * ---- all four calls ----
 * The functions are homogeneous of degree 0 in each direction, so
 *   - each direction gradient is orthogonal to its own direction: grad_wi[u] . wi[u] = 0, grad_wo[u] . wo[u] = 0 (to rounding);
 *   - for unnormalised inputs it scales with 1 / |w|: scaling wi by s divides grad_wi by s and leaves the other outputs as they are.
 * The outputs are OVERWRITTEN per unit, not accumulated into.
 * Materials: mat == NULL: every unit uses single_id, which must be a live GGX material (MRL_ERR_MATERIAL otherwise).  mat != NULL:
 * one id per unit; a unit whose id names no live GGX material (out of range, negative, released, a table, n-channel, RGL or spectral
 * material) gets zeros.
 * A NULL input: MRL_ERR_INVALID.  Pointers all host or all device (MRL_ERR_POINTER_MIX).  Device pointers: asynchronous on the
 * context's stream; no workspace, no reduction, no atomics.  n == 0 / capacity == 0: MRL_OK, nothing is touched.
 * The *_batch calls take host arrays as well, through the staged chunk loop (MRL_OPT_HOST_CHUNK), mat included.
 * The *_queue calls follow mrl_eval_queue: device pointers only; they process the slots queue[0 .. min(*queue_count, capacity)),
 * read a slot's inputs from and write its outputs to the slot named, leave every other slot untouched; capacity <= 2^32;
 * capturable in a HIP graph as one launch on one stream (the count is read on the device at run time).
 * DETERMINISM (a contract of these calls): a unit's output bits depend on its own inputs and its material's parameters alone —
 * the whole-array, material-id, queue and host-array forms return identical bits for the same unit, whatever n, the grid or the
 * unit's position, and each output has the same bits whichever other outputs are NULL.
 * Not offered: gradients in u; tables and RGL materials (a table's pdf is cos / pi or piecewise constant; RGL's pdf and sampler
 * gradients need a design of their own); device groups (mrl_group_*); the one-unit paths; second derivatives. */
int mrl_ggx_pdf_grad_batch(mrl_ctx *ctx, const float *wi, const float *wo, const float *grad_pdf,
                           const int32_t *mat, int32_t single_id, size_t n,
                           float *grad_wi, float *grad_wo, float *grad_alpha);
int mrl_ggx_pdf_grad_queue(mrl_ctx *ctx, const float *wi, const float *wo, const float *grad_pdf,
                           const int32_t *mat, int32_t single_id,
                           const uint32_t *queue, const uint32_t *queue_count, size_t capacity,
                           float *grad_wi, float *grad_wo, float *grad_alpha);
int mrl_ggx_sample_grad_batch(mrl_ctx *ctx, const float *wi, const float *u, const float *grad_out,
                              const int32_t *mat, int32_t single_id, size_t n,
                              float *grad_wi, float *grad_params);
int mrl_ggx_sample_grad_queue(mrl_ctx *ctx, const float *wi, const float *u, const float *grad_out,
                              const int32_t *mat, int32_t single_id,
                              const uint32_t *queue, const uint32_t *queue_count, size_t capacity,
                              float *grad_wi, float *grad_params);

#ifdef __cplusplus
}
#endif
#endif
