/* merl_hip_fit_rgl_spectral.h — fitting the measured spectra of spectral RGL materials (MRL_KIND_RGL_SPECTRAL:
 * mrl_material_upload_rgl_spectral): the adjoint of eval_spectral in a file's `spectra` array, with a material id per unit and over
 * wavefront queues, onto several target materials in one launch, and new spectra for a resident material in place.  The spectral twin
 * of merl_hip_fit_rgl.h; it includes merl_hip.h (contexts, materials, status codes, options) and the library exports both sets.  Calls
 * added here are listed in host.FIT_RGL_SPECTRAL_ABI_SYMBOLS and checked against this header by
 * tests/test_rgl_spectral_values_grad_cpu.py.  DESIGN.md §5s. */
#ifndef MERL_HIP_FIT_RGL_SPECTRAL_H
#define MERL_HIP_FIT_RGL_SPECTRAL_H

#include "merl_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The most targets one call takes: the targets' descriptors, 40 B each, travel by value in the kernel arguments, so that a queue
 * call copies nothing from host memory at call time, and every lane compares its id with every one. */
#define MRL_RGL_SPECTRAL_GRAD_MAX_TARGETS 16

/* ---- the operator ----
 * Let R be a spectral RGL file's spectra array as uploaded, [n_phi][n_theta][n_wl][ny][nx] f32 (stored unnormalised: the image holds
 * the same bits).  For a live unit and its wavelength k < W mrl_eval_spectral_batch rounds
 *     v(node) = sum_s ws_s sum_j wc_j R[slice_s][node][corner_j]
 *     v_k     = lerp(t_k, v(c0), v(c0 + 1))        (a file with one node, or wavelengths == NULL: v_k = v(k), c0 = k, t_k = 0)
 *     E_k     = max(0, v_k) J
 * with s over the 1 / 2 / 4 slices of the (phi_i, theta_i) bracket, j over the four corners of the cell at s = vndf.invert(u_m),
 * [c0, c0 + 1] eval's bracket of lambda_k among the file's wavelength nodes, t_k its position in it clamped to [0, 1]
 * (merl_hip_diff_rgl_spectral.h), and J = ndf(u_m) / (4 sigma(u_wi)) if the file's jacobian flag is set, else 1.  Per target material
 * the calls compute
 *     G[slice_s][c0    ][corner_j] += g_k [v_k >= 0] J (1 - t_k) ws_s wc_j
 *     G[slice_s][c0 + 1][corner_j] += g_k [v_k >= 0] J      t_k  ws_s wc_j
 * G f64 in the layout of R, ACCUMULATED into (G += (dE/dR)^T g), the products formed in f64.
 * Value clamp: decided on the interpolated value v_k, formed with eval's own operations — a wavelength whose interpolated value is
 * below 0 contributes nothing to either node.
 * Clamped wavelength: a wavelength outside the nodes (t_k = 0 or 1; +-inf included: eval's bracket, clamped) gives its whole weight to
 * the end node; the other node receives no term.  The same holds for a wavelength exactly on a node: it gives its whole weight to
 * that node (on the file's last node eval's own quotient may round to 1 - 2^-53; the weights take 1, the clamp decision stays eval's).
 * NaN wavelength of a live unit: contributes nothing for that k; the unit's other wavelengths are unaffected.
 * Dead units — eval's guard: wi.z <= 0, wo.z <= 0, a NaN / inf component, a failed normalisation — contribute nothing, whatever their
 * grad_values and wavelengths hold (NaN and inf included).
 * A term that is exactly 0 is not added: a texel nothing reaches keeps its bits (-0.0 included).
 * On a file whose spectra are all >= 0 nothing is clamped, eval_spectral(R) = A R is linear and the call is A^T g.
 * NOT touched: vndf, ndf, sigma, luminance, the parameter grids and the wavelength nodes are neither differentiated nor updated by
 * anything in this header.
 * Wavelengths: wavelengths is [n][n_wavelengths] f32, n_wavelengths = W in 1..4096, grad_values [n][W] f32.  wavelengths == NULL
 * ("the file's own nodes", channel k is node k) is allowed only with mat == NULL and W equal to the material's node count; a call with
 * mat != NULL needs wavelengths (its materials may have different node grids): MRL_ERR_INVALID otherwise.
 * Targets and layout: target_ids is ALWAYS a host array of n_targets material ids.  grad_spectra holds the targets end to end at the
 * offsets mrl_rgl_spectral_values_grad_layout gives, target k in the layout of its own spectra array.
 * Material of a unit: mat != NULL: mat[i] (the queue form: mat[slot]); mat == NULL: every unit uses single_id.
 * Non-target units: a unit whose id is not among the targets adds nothing — an RGB RGL file, a table, GGX, n-channel or other spectral
 * material, a released, negative or out-of-range id.  Files of different shapes and node grids may meet in one launch.
 * Pointers — wi, wo, wavelengths, grad_values, mat, grad_spectra — all host or all device: MRL_ERR_POINTER_MIX.
 * mrl_rgl_spectral_values_grad_batch takes host arrays through the staged chunk loop (MRL_OPT_HOST_CHUNK); such a call returns when
 * grad_spectra is complete.  mrl_rgl_spectral_values_grad_queue follows mrl_eval_spectral_queue: device pointers only; it processes
 * the slots queue[0 .. min(*queue_count, capacity)), the count read on the device; a slot listed twice adds twice; capacity <= 2^32
 * (MRL_ERR_INVALID above).  It copies nothing from pageable host memory and is capturable in a HIP graph once the workspace below has
 * its size (a first call outside the capture sees to that).
 * n == 0 / capacity == 0: MRL_OK, nothing is touched, whatever the other arguments are.
 * Errors: MRL_ERR_MATERIAL: a target that is not a live MRL_KIND_RGL_SPECTRAL material.  MRL_ERR_INVALID: a target listed twice;
 * n_targets < 1 or above MRL_RGL_SPECTRAL_GRAD_MAX_TARGETS; NULL wi, wo, grad_values, target_ids or grad_spectra (the queue form: NULL
 * queue or queue_count); n_wavelengths outside 1..4096; the two wavelength rules above; more than 2^31 - 1 (workspace record, node)
 * pairs over all targets.  MRL_ERR_POINTER_MIX.  MRL_ERR_OOM: a workspace that does not fit.
 * Workspace: one gradient brick per (bracket, cell) of every target — n_wl S 4 doubles in the slot order [node][slice][corner], so
 * that what one unit adds for one node is one contiguous run of 4 S doubles (32 / 64 / 128 B) — in the grow-only workspace
 * mrl_table_grad_batch owns, cleared once and folded once per call: sum over the targets of records x n_wl x S x 32 B, records =
 * (n_phi - 1 or 1) (n_theta - 1 or 1) (ny - 1) (nx - 1).  An isotropic 8 x 32 x 32 file with 195 nodes takes 84 MB, a large
 * anisotropic one over a gigabyte; form 1 below needs none.  mrl_memory_info reports it; it is not counted against
 * MRL_OPT_MEMORY_LIMIT_MB; MRL_ERR_OOM where it does not fit.
 * MRL_OPT_TABLE_GRAD_KERNEL selects the same four forms as for the table adjoint: 0 bricks, merged per wave when at least 4 lanes share
 * the first live lane's (record, node); 1 plain planar atomics (the baseline, no workspace); 2 / 3 bricks never / always merged.  The
 * sums are f64 atomics in no fixed order: two calls, and the four forms, agree to f64 rounding, not bit for bit.  A (unit, node) run
 * is a quarter of the RGB brick's size; form 0 still beats form 1 on scattered pairs, 5 to 7 times on MI355X, and merging buys
 * nothing at this run size: forms 0 and 2 take the same time, form 3 is never the fastest (DESIGN.md §5s has the table).
 * Out of scope: device groups (mrl_group_*); the one-unit paths; plugin properties; rebuilding luminance; gradients in vndf / ndf /
 * sigma / the wavelength nodes; updates that change a file's shape or node grid; gradients of pdf and sample. */
int mrl_rgl_spectral_values_grad_batch(mrl_ctx *ctx, const float *wi, const float *wo, const float *wavelengths, int n_wavelengths,
                                       const float *grad_values, const int32_t *mat, int32_t single_id, size_t n,
                                       const int32_t *target_ids, int n_targets, double *grad_spectra);
int mrl_rgl_spectral_values_grad_queue(mrl_ctx *ctx, const float *wi, const float *wo, const float *wavelengths, int n_wavelengths,
                                       const float *grad_values, const int32_t *mat, int32_t single_id,
                                       const uint32_t *queue, const uint32_t *queue_count, size_t capacity,
                                       const int32_t *target_ids, int n_targets, double *grad_spectra);

/* The shape of a live spectral RGL material's spectra array: n_phi, n_theta, n_wl, ny, nx.  MRL_ERR_MATERIAL for any other id. */
int mrl_rgl_spectral_values_shape(const mrl_ctx *ctx, int id, int shape[5]);

/* Where each target's slice of grad_spectra starts — the arithmetic the two calls use, without a context or a device: shapes is
 * [n_targets][5] as mrl_rgl_spectral_values_shape reports them; offsets_out (may be NULL) receives n_targets + 1 values in doubles,
 * offsets_out[n_targets] the size of grad_spectra.  MRL_ERR_INVALID, and offsets_out is then not to be used: NULL shapes; n_targets < 1
 * or above MRL_RGL_SPECTRAL_GRAD_MAX_TARGETS; n_phi or n_theta below 1, n_wl outside 1..4096, ny or nx below 2; more than 2^31 - 1
 * (record, node) pairs — records x n_wl per target — over all targets. */
int mrl_rgl_spectral_values_grad_layout(const int *shapes, int n_targets, size_t *offsets_out);

/* ---- new spectra in place ----
 * mrl_material_update_rgl_values' contract (merl_hip_fit_rgl.h) for a spectral RGL material.  spectra: a host or device pointer in the
 * file's own spectra layout.  The id, the addresses, the material's entry in the device array and the accounted bytes are unchanged;
 * graphs and queues see the new values on their next replay — single-material launches included: the RGL descriptor that travels in
 * the kernel arguments holds POINTERS into the image.
 * Stream-ordered: from a device pointer the call is kernel launches on the context's stream and nothing else, and is capturable.  It
 * drains the one-unit mailbox service first and leaves mrl_host_table snapshots as they are.
 * The image is written by a small kernel, one thread per float4 of the bracket-major value bricks; values are stored unnormalised, so
 * there is no arithmetic and the result has the bits of a fresh upload.
 * Sampling: the luminance distribution is NOT rebuilt: pdf and the sampled directions keep their bits, and sample's reported values
 * and weights use the new spectra.
 * Non-finite values: an update from a host pointer refuses them (MRL_ERR_INVALID, material untouched).  An update from a device
 * pointer cannot look without a synchronisation: finite values are the caller's responsibility.
 * MRL_ERR_INVALID: flags other than 0, NULL spectra.  MRL_ERR_MATERIAL: an RGB RGL material, a table, a GGX material, a released id. */
int mrl_material_update_rgl_spectral_values(mrl_ctx *ctx, int id, const float *spectra, int flags);

#ifdef __cplusplus
}
#endif
#endif
