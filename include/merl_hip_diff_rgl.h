/* merl_hip_diff_rgl.h — the direction gradient of eval on RGB RGL materials (the adaptive parameterisation of the RGL material
 * database's *.bsdf files, upstream Mitsuba 3's `measured`): the RGL twin of merl_hip_diff_table.h.  It includes merl_hip_diff.h
 * (and with it merl_hip.h: contexts, materials, status codes, options); the library exports all the sets.  Calls added here are
 * listed in host.DIFF_RGL_ABI_SYMBOLS and checked against this header by tests/test_rgl_dir_grad_cpu.py.  DESIGN.md §5p. */
#ifndef MERL_HIP_DIFF_RGL_H
#define MERL_HIP_DIFF_RGL_H

#include "merl_hip_diff.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- the operator ----
 * Let a = wi / |wi| and b = wo / |wo|, after the sign reduction of a symmetry-reduced file (both directions' x and y multiplied by
 * the +-1 factors the signs of wi choose).  E_c(wi, wo) is the real-valued function mrl_eval_batch rounds for an RGB RGL material:
 *     m = (a + b) normalised;   u_m = (sqrt(2 theta_m / pi), frac((phi_m - [phi_i if isotropic]) / 2 pi + 1/2));
 *     (tp, tt) the clamped positions of (phi_i, theta_i) in their parameter brackets;   s = vndf.invert(u_m; tp, tt);
 *     V_c = max(0, bilinear of the rgb cell at s, blended over the bracket's slices);
 *     E_c = V_c ndf(u_m) / (4 sigma(u_wi)) if the file's jacobian flag is set, else V_c.
 * Every table is the STORED Float image: the normalised corner values, the integrals left of the cell, the row totals and the
 * marginal, rounded once when the material is built.  Per unit u the calls write the vector-Jacobian products
 *     grad_wi[u] = sum_c grad_rgb[u][c] dE_c / d wi          grad_wo[u] = sum_c grad_rgb[u][c] dE_c / d wo
 * wi, wo, grad_rgb, grad_wi, grad_wo: [n][3] f32.  The outputs are OVERWRITTEN per unit, not accumulated into.
 * Exact derivative of the piecewise function, in the cells eval selects.  The inverse warp is a direct cell lookup, so the gradient
 * has a closed form.  Differences of stored Floats inside a cell — left(row + 1) - left(row), r1 - r0 of the row totals, the corner
 * differences along x and y — are formed per slice in f64 (exact) before any weight meets them; the differences between the
 * slices of a bracket are the same blends with the derivative weights below, whose f64 products are summed by FMAs.  Nothing of
 * lower accuracy than the library's 1e-15 reciprocals and square roots enters.
 * Inside the inverse warp, with x, y the cell fractions: d uy / dy = lerp(y, r0, r1); d sx / dx = lerp(x, c0, c1) / tot; d sx / dy
 * carries the y-derivatives of c0, c1, `left` and `tot`.  tot == 0 (a cell row without mass) gives zero terms, as it gives a zero
 * value.
 * Parameter derivatives d / d tp and d / d tt of every blended quantity (corner values, left, totals, marginal, rgb) are the same
 * blends with the weights (-(1 - tt), (1 - tt), -tt, tt) and (-(1 - tp), -tp, (1 - tp), tp).  d tp / d phi_i = 1 / (p1 - p0), or 0
 * while the bracket's clamp is active or the grid has one node; the same holds for tt.
 * Channel clamp: a clamped channel (bilinear value < 0) contributes 0.
 * Where a map has no derivative that term is dropped (taken as 0) and every output stays finite: m at the normal (theta_m's square
 * root, phi_m undefined), wi at the normal (phi_i undefined, the square root of theta_i); a + b = 0 cannot happen on a live unit.
 * A component beyond the Float range is written as +-FLT_MAX, and one that a grad_rgb near FLT_MAX turns into inf - inf inside is
 * written as 0, as the table family does.
 * Identities: E is homogeneous of degree 0 in wi and in wo — wo is normalised, the cosine lives in the measured values — so
 *   - grad_wi[u] . wi[u] = 0 and grad_wo[u] . wo[u] = 0 (to rounding);
 *   - for unnormalised inputs the gradients scale with 1 / |w|: scaling wi by s divides grad_wi by s.
 * MRL_OPT_COSINE_FACTOR, MRL_OPT_NEGATIVE, MRL_OPT_LOOKUP and MRL_OPT_NODE do not apply, as they do not apply to RGL eval.
 * Symmetry-reduced files: the gradient components are multiplied back by the +-1 factors of the reduction; a pair and its
 * mirrored pair return mirrored gradients with identical bits.
 * Dead units — eval's: wi.z <= 0, wo.z <= 0, a NaN / inf component, a failed normalisation — get exactly +0.0f in both outputs,
 * whatever their grad_rgb holds (NaN and inf included).
 * Materials: mat == NULL: every unit uses single_id, which must be a live RGB RGL material (MRL_KIND_RGL; MRL_ERR_MATERIAL
 * otherwise).  mat != NULL: one id per unit; a unit whose id names anything else (out of range, negative, released, a table, GGX,
 * n-channel or spectral RGL material) gets zeros.  Files of different shapes may meet in one launch.
 * One of grad_wi / grad_wo may be NULL: that gradient is then not written; both NULL: MRL_ERR_INVALID.  NULL wi, wo or grad_rgb:
 * MRL_ERR_INVALID.  Pointers all host or all device (MRL_ERR_POINTER_MIX).  Device pointers: asynchronous on the context's stream;
 * no workspace, no reduction, no atomics.  n == 0 / capacity == 0: MRL_OK, nothing is touched.
 * mrl_rgl_grad_dir_batch takes host arrays as well, through the staged chunk loop (MRL_OPT_HOST_CHUNK), mat included.
 * mrl_rgl_grad_dir_queue follows mrl_eval_queue: device pointers only; it processes the slots queue[0 .. min(*queue_count,
 * capacity)), reads a slot's inputs from and writes its outputs to the slot named, leaves every other slot untouched;
 * capacity <= 2^32; capturable in a HIP graph (the count is read on the device at run time).
 * DETERMINISM (a contract of these calls): a unit's output bits depend on its own inputs and its material alone — the whole-array,
 * material-id, queue and host-array forms return identical bits for the same unit, whatever n, the grid or the unit's position;
 * grad_wi has the same bits with and without grad_wo.  Contraction is off and the FMAs are explicit in the per-unit function; no
 * kernel is compiled for one bracket shape.
 * Not offered: device groups (mrl_group_*), the one-unit paths, second derivatives, gradients of pdf and sample.  The gradient in an
 * RGB file's measured values (fitting a file) is mrl_rgl_values_grad_batch / _queue of merl_hip_fit_rgl.h.  Spectral RGL files:
 * merl_hip_diff_rgl_spectral.h. */
int mrl_rgl_grad_dir_batch(mrl_ctx *ctx, const float *wi, const float *wo, const float *grad_rgb,
                           const int32_t *mat, int32_t single_id, size_t n,
                           float *grad_wi, float *grad_wo);
int mrl_rgl_grad_dir_queue(mrl_ctx *ctx, const float *wi, const float *wo, const float *grad_rgb,
                           const int32_t *mat, int32_t single_id,
                           const uint32_t *queue, const uint32_t *queue_count, size_t capacity,
                           float *grad_wi, float *grad_wo);

#ifdef __cplusplus
}
#endif
#endif
