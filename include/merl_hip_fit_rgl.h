/* merl_hip_fit_rgl.h — fitting the measured values of RGB RGL materials (MRL_KIND_RGL: mrl_material_upload_rgl / mrl_material_load_rgl):
 * the adjoint of eval in a file's `rgb` array, with a material id per unit and over wavefront queues, onto several target materials in
 * one launch, and new values for a resident material in place.  The RGL twin of merl_hip_fit_table.h and merl_hip_update.h; it
 * includes merl_hip.h (contexts, materials, status codes, options) and the library exports both sets.  Calls added here are listed in
 * host.FIT_RGL_ABI_SYMBOLS and checked against this header by tests/test_rgl_values_grad_cpu.py.  DESIGN.md §5r. */
#ifndef MERL_HIP_FIT_RGL_H
#define MERL_HIP_FIT_RGL_H

#include "merl_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The most targets one call takes: the targets' (id, workspace base) descriptors, 40 B each, travel by value in the kernel
 * arguments, so that a queue call copies nothing from host memory at call time, and every lane compares its id with every one. */
#define MRL_RGL_GRAD_MAX_TARGETS 16

/* ---- the operator ----
 * Let R be an RGB RGL file's rgb array as uploaded, [n_phi][n_theta][3][ny][nx] f32 (stored unnormalised: the image holds the same
 * bits).  For a live unit mrl_eval_batch rounds
 *     V_c = sum_k ws_k sum_j wc_j R[slice_k][c][corner_j]        E_c = max(0, V_c) J
 * with k over the 1 / 2 / 4 slices of the (phi_i, theta_i) bracket, j over the four corners of the cell at s = vndf.invert(u_m) and
 * J = ndf(u_m) / (4 sigma(u_wi)) if the file's jacobian flag is set, else 1.  Per target material the calls compute
 *     G[slice_k][c][corner_j] += g_c [V_c >= 0] J ws_k wc_j
 * G f64 in the layout of R, ACCUMULATED into (G += (dE/dR)^T g), the products formed in f64.  A channel whose blended value is below
 * 0 contributes 0 (the clamp rule of merl_hip_diff_rgl.h).  This is the exact derivative of the piecewise function in the cells eval
 * selects; on a file whose values are all >= 0 nothing is clamped, eval(R) = A R is linear and the call is A^T g.
 * The cell, the bracket, the slice weights, the inverse warp and J are eval's own functions; the sign reduction of a symmetry-reduced
 * file is applied before the lookup, as in eval (it does not touch values).  A texel nothing reaches keeps its bits.
 * NOT touched: vndf, ndf, sigma, luminance and the parameter grids are neither differentiated nor updated by anything in this header.
 * Dead units — eval's guard: wi.z <= 0, wo.z <= 0, a NaN / inf component, a failed normalisation — contribute nothing, whatever
 * their grad_rgb holds (NaN and inf included).
 * Targets and layout: target_ids is ALWAYS a host array of n_targets material ids.  grad_values holds the targets end to end at the
 * offsets mrl_rgl_values_grad_layout gives, target k in the layout of its own rgb array.
 * Material of a unit: mat != NULL: mat[i] (the queue form: mat[slot]); mat == NULL: every unit uses single_id.
 * Non-target units: a unit whose id is not among the targets adds nothing — a table, GGX, n-channel, spectral or other RGL material,
 * a released, negative or out-of-range id.  Files of different shapes, isotropic and anisotropic, may meet in one launch.
 * Pointers — wi, wo, grad_rgb, mat, grad_values — all host or all device: MRL_ERR_POINTER_MIX.  mrl_rgl_values_grad_batch takes host
 * arrays through the staged chunk loop (MRL_OPT_HOST_CHUNK); such a call returns when grad_values is complete.
 * mrl_rgl_values_grad_queue follows mrl_eval_queue: device pointers only; it processes the slots queue[0 .. min(*queue_count,
 * capacity)), the count read on the device; a slot listed twice adds twice; capacity <= 2^32 (MRL_ERR_INVALID above).  It copies
 * nothing from pageable host memory and is capturable in a HIP graph once the workspace below has its size (a first call outside the
 * capture sees to that).
 * n == 0 / capacity == 0: MRL_OK, nothing is touched, whatever the other arguments are.
 * Errors: MRL_ERR_MATERIAL: a target that is not a live MRL_KIND_RGL material.  MRL_ERR_INVALID: a target listed twice; n_targets < 1
 * or above MRL_RGL_GRAD_MAX_TARGETS; NULL wi, wo, grad_rgb, target_ids or grad_values (the queue form: NULL queue or queue_count); more
 * than 2^31 - 1 workspace records over all targets.  MRL_ERR_OOM: a workspace that does not fit.
 * Workspace: one gradient brick per (bracket, cell) of every target — 12 S doubles in the slot order [channel][slice][corner], padded
 * to 16 S (128 / 256 / 512 B for S = 1 / 2 / 4 slices) — in the grow-only workspace mrl_table_grad_batch owns, cleared once and folded
 * once per call; mrl_memory_info reports it; it is not counted against MRL_OPT_MEMORY_LIMIT_MB.
 * MRL_OPT_TABLE_GRAD_KERNEL selects the same four forms as for the table adjoint: 0 bricks, merged per wave when at least 4 lanes share
 * the first live lane's brick; 1 plain planar atomics (the measured baseline); 2 / 3 bricks never / always merged.  The sums are f64
 * atomics in no fixed order: two calls, and the four forms, agree to f64 rounding, not bit for bit.
 * Out of scope: spectral RGL files here (their twin is merl_hip_fit_rgl_spectral.h); device groups (mrl_group_*); the one-unit paths; plugin properties; rebuilding luminance;
 * gradients in vndf / ndf / sigma; updates that change a file's shape. */
int mrl_rgl_values_grad_batch(mrl_ctx *ctx, const float *wi, const float *wo, const float *grad_rgb,
                              const int32_t *mat, int32_t single_id, size_t n,
                              const int32_t *target_ids, int n_targets, double *grad_values);
int mrl_rgl_values_grad_queue(mrl_ctx *ctx, const float *wi, const float *wo, const float *grad_rgb,
                              const int32_t *mat, int32_t single_id,
                              const uint32_t *queue, const uint32_t *queue_count, size_t capacity,
                              const int32_t *target_ids, int n_targets, double *grad_values);

/* The shape of a live RGB RGL material's rgb array: n_phi, n_theta, 3, ny, nx.  MRL_ERR_MATERIAL for any other id. */
int mrl_rgl_values_shape(const mrl_ctx *ctx, int id, int shape[5]);

/* Where each target's slice of grad_values starts — the arithmetic the two calls use, without a context or a device: shapes is
 * [n_targets][5] as mrl_rgl_values_shape reports them; offsets_out (may be NULL) receives n_targets + 1 values in doubles,
 * offsets_out[n_targets] the size of grad_values.  MRL_ERR_INVALID, and offsets_out is then not to be used: NULL shapes; n_targets < 1
 * or above MRL_RGL_GRAD_MAX_TARGETS; n_phi or n_theta below 1, a channel count other than 3, ny or nx below 2; more than 2^31 - 1
 * workspace records ((n_phi - 1 or 1) (n_theta - 1 or 1) (ny - 1) (nx - 1) per target) over all targets. */
int mrl_rgl_values_grad_layout(const int *shapes, int n_targets, size_t *offsets_out);

/* ---- new values in place ----
 * mrl_material_update_table's contract (merl_hip_update.h) for an RGB RGL material.  rgb: a host or device pointer in the file's own
 * rgb layout.  The id, the addresses, the material's entry in the device array and the accounted bytes are unchanged; graphs and
 * queues see the new values on their next replay — single-material launches included: the RGL descriptor that travels in the kernel
 * arguments holds POINTERS into the image, unlike the GGX descriptor, which holds the parameters themselves.
 * Stream-ordered: from a device pointer the call is kernel launches on the context's stream and nothing else, and is capturable.  It
 * drains the one-unit mailbox service first and leaves mrl_host_table snapshots as they are, exactly as mrl_material_update_table does.
 * The image is written by a small kernel, one thread per float4 of the bracket-major value bricks; values are stored unnormalised, so
 * there is no arithmetic and the result has the bits of a fresh upload.
 * Sampling: the luminance distribution is NOT rebuilt.  A stale proposal is still a valid one: pdf and the sampled directions keep their
 * bits, and sample's reported eval and weight use the new values (weight = eval / pdf stays an unbiased estimator's weight).
 * Non-finite values: an upload refuses them on the host, and so does an update from a host pointer (MRL_ERR_INVALID, material
 * untouched).  An update from a device pointer cannot look without a synchronisation: finite values are the caller's responsibility.
 * MRL_ERR_INVALID: flags other than 0, NULL rgb.  MRL_ERR_MATERIAL: a spectral RGL material, a table, a GGX material, a released id. */
int mrl_material_update_rgl_values(mrl_ctx *ctx, int id, const float *rgb, int flags);

#ifdef __cplusplus
}
#endif
#endif
