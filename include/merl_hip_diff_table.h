/* merl_hip_diff_table.h — the direction gradient of eval on RGB TABLE materials (MERL / customized_measurement): the table twin of
 * merl_hip_diff.h, which it includes (and with it merl_hip.h: contexts, materials, status codes, options); the library exports all
 * three sets.  Calls added here are listed in host.DIFF_TABLE_ABI_SYMBOLS and checked against this header by
 * tests/test_table_dir_grad_cpu.py.  DESIGN.md §5j. */
#ifndef MERL_HIP_DIFF_TABLE_H
#define MERL_HIP_DIFF_TABLE_H

#include "merl_hip_diff.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- the operator ----
 * Let a = wi / |wi|, b = wo / |wo| and x(a, b) = (x0, x1, x2) the continuous table coordinates of the material's parameterisation,
 * exactly as eval forms them: MRL_PARAM_HALF_DIFF with its sqrt-warped theta_h, MRL_PARAM_STANDARD, MRL_PARAM_STANDARD_FULL.
 * Let T_c(x) be the trilinear interpolant of the material's STORED Float texels (scaled; clamped at 0 under MRL_OPT_NEGATIVE = 0),
 * with eval's cell selection, its clamped and periodic axes and the half-texel shift of MRL_OPT_NODE = 1.  Let kappa be the Float
 * wo.z — raw, not normalised, as eval multiplies by it — or 1 under MRL_OPT_COSINE_FACTOR = 1.  E_c(wi, wo) = T_c(x(a, b)) kappa is
 * the real-valued function mrl_eval_batch rounds.  Per unit u the calls write the vector-Jacobian products
 *     grad_wi[u] = sum_c grad_rgb[u][c] dE_c / d wi          grad_wo[u] = sum_c grad_rgb[u][c] dE_c / d wo
 * wi, wo, grad_rgb, grad_wi, grad_wo: [n][3] f32.  The outputs are OVERWRITTEN per unit, not accumulated into.
 * What is differentiated is the exact interpolant, not eval's rounded arithmetic: nothing of eval's Float corner weights or its
 * packed Float blend enters.  dT / df_axis is a weighted sum of differences of corner texels; the differences and the sums are
 * formed in f64 from the Float texels, per channel and before the channels are summed (the difference of two Floats is exact in f64;
 * on a smooth table, where neighbouring texels agree to 1e-3 relative and better, a Float difference would lose everything): the
 * rounding error scales with the variation of each channel inside the cell, never with a channel's magnitude.
 * T is piecewise trilinear: the gradient is the one of the cell eval selects.  A clamped fraction has derivative 0 while its clamp
 * is active (x - shift < 0 on a clamped axis); the padded upper end has derivative 0 through its equal texels.
 * Where a coordinate map has no derivative — half / diff: h == n (rho == 0), retro-reflection (e == 0), px == py == 0; the standard
 * forms: a direction exactly at the normal — that coordinate's term is dropped (taken as 0).  Every output is finite for every
 * finite input: a component beyond the Float range is written as +-FLT_MAX, and one that a grad_rgb near FLT_MAX turns into inf - inf
 * inside is written as 0.
 * MRL_OPT_LOOKUP = 0 (nearest): T is piecewise constant, the table term is 0: grad_wi = 0, grad_wo = (d kappa / d wo.z) sum_c g_c T_c
 * e_z.  MRL_OPT_NEGATIVE = 1 (keep) differentiates the raw texels; MRL_OPT_NEGATIVE = 2 (renormalise): MRL_ERR_INVALID, as the
 * adjoint mrl_table_grad_batch refuses it.
 * Identities: E is homogeneous of degree 0 in wi and, with the cosine factor, of degree 1 in wo (the raw wo.z), so
 *   - grad_wi[u] . wi[u] = 0 (orthogonal to its own direction, to rounding);
 *   - grad_wo[u] . wo[u] = sum_c grad_rgb[u][c] E_c (Euler's identity) with the cosine factor, 0 without it;
 *   - for unnormalised inputs grad_wi scales with 1 / |w|: scaling wi by s divides grad_wi by s.
 * Dead units — eval's: wi.z <= 0, wo.z <= 0, a NaN / inf component — get exactly +0.0f in both outputs, whatever their grad_rgb holds
 * (NaN and inf included).
 * Materials: mat == NULL: every unit uses single_id, which must be a live MERL / customized_measurement RGB table (MRL_ERR_MATERIAL
 * otherwise).  mat != NULL: one id per unit; a unit whose id names no live RGB table (out of range, negative, released, a GGX,
 * n-channel, RGL or spectral material) gets zeros.  Tables of different dims and parameterisations may meet in one launch.
 * One of grad_wi / grad_wo may be NULL: that gradient is then not written; both NULL: MRL_ERR_INVALID.  NULL wi, wo or grad_rgb:
 * MRL_ERR_INVALID.  Pointers all host or all device (MRL_ERR_POINTER_MIX).  Device pointers: asynchronous on the context's stream;
 * no workspace, no reduction, no atomics.  n == 0 / capacity == 0: MRL_OK, nothing is touched.
 * mrl_table_grad_dir_batch takes host arrays as well, through the staged chunk loop (MRL_OPT_HOST_CHUNK), mat included.
 * mrl_table_grad_dir_queue follows mrl_eval_queue: device pointers only; it processes the slots queue[0 .. min(*queue_count,
 * capacity)), reads a slot's inputs from and writes its outputs to the slot named, leaves every other slot untouched;
 * capacity <= 2^32; capturable in a HIP graph (the count is read on the device at run time).
 * DETERMINISM (a contract of these calls): a unit's output bits depend on its own inputs, its material and the context's options
 * alone — the whole-array, material-id, queue and host-array forms return identical bits for the same unit, whatever n, the grid
 * or the unit's position; grad_wi has the same bits with and without grad_wo; MRL_OPT_TABLE_LAYOUT rows and bricks return identical
 * bits.
 * Not offered here: n-channel tables have the same pair of calls in merl_hip_diff_nch.h (mrl_table_grad_dir_batch_nch / _queue_nch).
 * RGB RGL materials have theirs in merl_hip_diff_rgl.h (mrl_rgl_grad_dir_batch / _queue).
 * Not offered: spectral RGL materials, device groups (mrl_group_*), the one-unit paths, second derivatives, gradients of pdf and sample, the
 * renormalising blend (MRL_OPT_NEGATIVE = 2). */
int mrl_table_grad_dir_batch(mrl_ctx *ctx, const float *wi, const float *wo, const float *grad_rgb,
                             const int32_t *mat, int32_t single_id, size_t n,
                             float *grad_wi, float *grad_wo);
int mrl_table_grad_dir_queue(mrl_ctx *ctx, const float *wi, const float *wo, const float *grad_rgb,
                             const int32_t *mat, int32_t single_id,
                             const uint32_t *queue, const uint32_t *queue_count, size_t capacity,
                             float *grad_wi, float *grad_wo);

#ifdef __cplusplus
}
#endif
#endif
