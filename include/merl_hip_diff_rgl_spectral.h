/* merl_hip_diff_rgl_spectral.h — the gradient of eval in the directions and in the wavelengths on SPECTRAL RGL materials (the
 * "spectra" + "wavelengths" files of the RGL material database, what upstream Mitsuba 3's `measured` evaluates in its spectral
 * variants): the spectral twin of merl_hip_diff_rgl.h, which it includes (and with it merl_hip_diff.h and merl_hip.h: contexts,
 * materials, status codes, options); the library exports all the sets.  Calls added here are listed in
 * host.DIFF_RGL_SPECTRAL_ABI_SYMBOLS and checked against this header by tests/test_rgl_spectral_dir_grad_cpu.py.  DESIGN.md §5q. */
#ifndef MERL_HIP_DIFF_RGL_SPECTRAL_H
#define MERL_HIP_DIFF_RGL_SPECTRAL_H

#include "merl_hip_diff_rgl.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The contract is merl_hip_diff_rgl.h's — the half vector, the parameter brackets, the inverse warp with its tot == 0 rule, the
 * factor ndf / (4 sigma), the dropped terms at the normal, +-FLT_MAX, the sign reduction — with the changes below.
 * ---- the operator ----
 * E_k(wi, wo, lambda_k) is the real-valued function mrl_eval_spectral_batch rounds for a spectral RGL material, k = 0 .. W - 1:
 *     s = vndf.invert(u_m; tp, tt) as for an RGB file;   [c0, c0 + 1] the bracket of lambda_k in the file's wavelength nodes (the
 *     largest c0 in [0, nodes - 2] with node(c0) <= lambda_k) and t_k its position there, clamped to [0, 1];
 *     v(node) = the bilinear value of the spectra cell at s, blended over the parameter bracket's slices;
 *     V_k = max(0, lerp(t_k, v(c0), v(c0 + 1)))   (a file with one node: V_k = max(0, v(0)));
 *     E_k = V_k ndf(u_m) / (4 sigma(u_wi)) if the file's jacobian flag is set, else V_k.   Below, scale is that factor, or 1.
 * Per unit u the calls write
 *     grad_wi[u] = sum_k grad_values[u][k] dE_k / d wi        grad_wo[u] = sum_k grad_values[u][k] dE_k / d wo            [n][3]
 *     grad_wavelengths[u][k] = grad_values[u][k] dE_k / d lambda_k
 *                            = grad_values[u][k] scale (v(c0 + 1) - v(c0)) / (node(c0 + 1) - node(c0))                  [n][W]
 * wi, wo: [n][3] f32; wavelengths, grad_values: [n][W] f32, rows 4-byte aligned (any W).  The outputs are OVERWRITTEN per unit.
 * dE_k / d lambda_k is piecewise constant in lambda_k; E_k does not depend on the other wavelengths of the unit.
 * Derivative rules, beyond the RGB contract's:
 *   - the value clamp is decided on the INTERPOLATED value, as eval decides it: a wavelength whose lerp is < 0 contributes 0 to
 *     every output, whatever its two nodes' values are;
 *   - d t_k / d lambda_k = 1 / (node(c0 + 1) - node(c0)), or 0 while the wavelength clamp is active (lambda_k outside the file's
 *     nodes) or the file has one node; grad_wavelengths[u][k] is exactly 0 in those two cases and where the value clamp is active;
 *   - the two-node difference v(c0 + 1) - v(c0) counts among the differences of stored Floats: it is formed corner by corner per
 *     slice in f64 before any weight meets it.
 * wavelengths == NULL: the file's own nodes — n_wavelengths must equal the node count (MRL_ERR_INVALID otherwise) and channel k is
 * node k, with no interpolation.  Allowed only with mat == NULL (MRL_ERR_INVALID with ids: the files of one call may have
 * different grids, as in mrl_eval_spectral_*), and grad_wavelengths must then be NULL too (MRL_ERR_INVALID: the nodes are no input).
 * mat != NULL requires wavelengths.  n_wavelengths is 1 .. 4096 (MRL_ERR_INVALID).
 * Any one or two of grad_wi, grad_wo, grad_wavelengths may be NULL: those are not written.  All three NULL: MRL_ERR_INVALID.  NULL
 * wi, wo or grad_values: MRL_ERR_INVALID.
 * Dead units — eval's: wi.z <= 0, wo.z <= 0, a NaN / inf component of a direction, a failed normalisation — get exactly +0.0f in all
 * outputs, their whole grad_wavelengths row included, whatever grad_values and wavelengths hold (NaN and inf included).
 * A non-finite lambda_k on a LIVE unit takes the bracket eval takes (+inf: the last, clamped; -inf and NaN: the first); every output
 * stays finite: +-inf is a clamped wavelength like any other; with a NaN, E_k is no number: grad_wavelengths[u][k] and the unit's
 * grad_wi and grad_wo are written as 0, the unit's other grad_wavelengths are not affected.  What exceeds the Float range is
 * written as +-FLT_MAX.
 * Materials: mat == NULL: every unit uses single_id, which must be a live spectral RGL material (MRL_KIND_RGL_SPECTRAL;
 * MRL_ERR_MATERIAL otherwise).  mat != NULL: one id per unit; a unit whose id names anything else (out of range, negative, released,
 * a table, GGX, n-channel or RGB RGL material) gets zeros in all outputs.  Files of different shapes and wavelength grids may meet
 * in one launch.
 * Identities, as for RGB files: grad_wi[u] . wi[u] = 0 and grad_wo[u] . wo[u] = 0 to rounding, the gradients scale with 1 / |w|,
 * and on Symmetry-reduced files a pair and its mirrored pair return mirrored direction gradients and the same grad_wavelengths,
 * with identical bits.  A spectral file with three nodes that holds an RGB file's arrays, called with wavelengths == NULL, returns
 * mrl_rgl_grad_dir_batch's bits.
 * Pointers all host or all device (MRL_ERR_POINTER_MIX).  Device pointers: asynchronous on the context's stream; no workspace, no
 * reduction, no atomics.  n == 0 / capacity == 0: MRL_OK, nothing is touched.
 * mrl_rgl_grad_dir_spectral_batch takes host arrays as well, through the staged chunk loop (MRL_OPT_HOST_CHUNK, and at most 256 MiB
 * of staging slot, as mrl_eval_spectral_batch), mat included.
 * mrl_rgl_grad_dir_spectral_queue follows mrl_eval_spectral_queue: device pointers only; it processes the slots queue[0 ..
 * min(*queue_count, capacity)), reads a slot's inputs from and writes its outputs to the slot named, leaves every other slot
 * untouched; capacity <= 2^32; capturable in a HIP graph (the count is read on the device at run time).
 * DETERMINISM (a contract of these calls): a unit's output bits depend on its own inputs and its material alone — the whole-array,
 * material-id, queue and host-array forms return identical bits for the same unit, whatever n, the grid or the unit's position;
 * each output has the same bits whichever of the other outputs are requested.  Contraction is off and the FMAs are explicit in the
 * per-unit function.
 * Not offered: device groups (mrl_group_*), the one-unit paths, second derivatives, gradients of pdf and sample.  The adjoint in
 * the file's values (fitting a file's spectra) is merl_hip_fit_rgl_spectral.h. */
int mrl_rgl_grad_dir_spectral_batch(mrl_ctx *ctx, const float *wi, const float *wo,
                                    const float *wavelengths, int n_wavelengths, const float *grad_values,
                                    const int32_t *mat, int32_t single_id, size_t n,
                                    float *grad_wi, float *grad_wo, float *grad_wavelengths);
int mrl_rgl_grad_dir_spectral_queue(mrl_ctx *ctx, const float *wi, const float *wo,
                                    const float *wavelengths, int n_wavelengths, const float *grad_values,
                                    const int32_t *mat, int32_t single_id,
                                    const uint32_t *queue, const uint32_t *queue_count, size_t capacity,
                                    float *grad_wi, float *grad_wo, float *grad_wavelengths);

#ifdef __cplusplus
}
#endif
#endif
