/* merl_hip_fit_ggx.h — the parameter gradient of eval on GGX conductors with a material id per unit and over wavefront queues,
 * onto several target materials in one launch: the multi-material twin of mrl_ggx_grad_batch of merl_hip_fit.h, which it includes
 * together with merl_hip.h (contexts, materials, status codes, options); the library exports all sets.  Calls added here are listed
 * in host.FIT_GGX_ABI_SYMBOLS and checked against this header by tests/test_ggx_grad_mat_cpu.py.  DESIGN.md §5m. */
#ifndef MERL_HIP_FIT_GGX_H
#define MERL_HIP_FIT_GGX_H

#include "merl_hip.h"
#include "merl_hip_fit.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The most targets one call takes.  The targets' ids travel by value in the kernel arguments, so that a queue call copies nothing
 * from host memory at call time; every lane compares its id with every target, and every wave keeps one 256-B row of sums per
 * target in LDS (4 KB at 16), so the bound also bounds the per-unit search and the LDS of a block. */
#define MRL_GGX_GRAD_MAX_TARGETS 16

/* ---- the operator ----
 * With p = (alpha, eta_r, eta_g, eta_b, k_r, k_g, k_b) and J_uc = d eval_c(wi_u, wo_u) / d p exactly as merl_hip_fit.h defines them
 * for mrl_ggx_grad_batch — taken at the stored Float parameters of the unit's OWN material, evaluated in f64 — the calls compute for
 * every target t
 *     grad_params[t][7]   += sum_u sum_c g_uc J_uc             g = grad_rgb = dL / d eval
 *     normal[t][7][7]     += sum_u sum_c h_uc J_uc J_uc^T      h = curv_rgb = d2L / d eval2, NULL = 1; normal may be NULL
 * over the units u whose material is target_ids[t].  One launch serves all targets; the streams are read once.  Both outputs are
 * ACCUMULATED into: the caller zeroes them, a second call adds to the first.  The entries of normal[t] that couple two different
 * channels are structurally zero and are never touched; both triangles of the others get the same value.  wi, wo, grad_rgb,
 * curv_rgb: [n][3] f32; grad_params: [n_targets][7] f64; normal: [n_targets][7][7] f64.
 * Material of a unit: mat != NULL: mat[i] (the queue form: mat[slot]); mat == NULL: every unit uses single_id.
 * Units that add nothing, whatever their grad_rgb and curv_rgb hold (NaN and inf included):
 *   - a unit whose id is not among the targets — a table, n-channel, RGL or spectral material, a GGX material that is not a target,
 *     a released, negative or out-of-range id;
 *   - a unit eval masks (cos(theta_i) <= 0, cos(theta_o) <= 0, a NaN / inf / zero-length direction), or one for which one of eval's
 *     own D / G1 selects returns 0.
 * A target that no unit names keeps the bits of its rows of grad_params and normal.
 * Targets: target_ids is ALWAYS a host array of n_targets material ids.  Every target must be a live GGX material:
 * MRL_ERR_MATERIAL otherwise (a table, n-channel, RGL, spectral, released or unknown id).  MRL_ERR_INVALID: a target listed twice;
 * n_targets < 1 or above MRL_GGX_GRAD_MAX_TARGETS; NULL wi, wo, grad_rgb, target_ids or grad_params (the queue form: NULL queue or
 * queue_count); a queue capacity above 2^32.
 * Pointers — wi, wo, grad_rgb, curv_rgb, mat and the outputs, which count as arrays — all host or all device: MRL_ERR_POINTER_MIX.
 * n == 0 / capacity == 0: MRL_OK, nothing is touched, whatever the other arguments are.
 * mrl_ggx_grad_batch_mat takes host arrays as well, through the staged chunk loop (MRL_OPT_HOST_CHUNK); mat and curv_rgb are further
 * streams.  Every chunk adds to one device array of [n_targets][7 + 49] doubles, which is added to the caller's arrays at the end.
 * Device pointers: asynchronous on the context's stream.
 * mrl_ggx_grad_queue follows mrl_eval_queue: device pointers only (MRL_ERR_POINTER_MIX); it processes the slots
 * queue[0 .. min(*queue_count, capacity)) and reads a slot's wi, wo, grad_rgb, curv_rgb and mat from the slot named; a slot listed
 * twice adds twice.  The count is read on the device at run time and the call copies nothing from pageable host memory, so it is
 * capturable in a HIP graph once the workspace below has its size (a first call outside the capture sees to that).
 * DETERMINISM (a contract of both calls): there are no atomics.  Every wave sums its units per target in a fixed order, every
 * block writes one row of partial sums per target to a workspace with plain stores, and one block per target adds the rows up in a
 * fixed order.  The grid and the order of every sum depend on n (or the capacity), n_targets and the device alone — and, of course,
 * on which unit names which target — so two device-pointer calls with the same inputs on the same device return bit-identical
 * outputs, and grad_params has the same bits with and without normal.  A unit's terms are the bits mrl_ggx_grad_batch computes for
 * it; the sums of the two calls differ by the order of their f64 additions only.
 * Workspace: grid x n_targets rows of 256 B, kept by the context in a buffer of its own (mrl_ggx_grad_batch keeps its workspace:
 * what a graph captured from either call points at stays valid), sized once for 16 targets; mrl_memory_info reports it as
 * workspace, and it is not counted against MRL_OPT_MEMORY_LIMIT_MB; if it does not fit: MRL_ERR_OOM.
 * Not offered: device groups (mrl_group_*), the one-unit paths.  (An autograd wrapper for the parameters: diff.ggx_eval(params=),
 * over mrl_material_update_ggx of merl_hip_update.h.) */
int mrl_ggx_grad_batch_mat(mrl_ctx *ctx, const float *wi, const float *wo, const float *grad_rgb, const float *curv_rgb,
                           const int32_t *mat, int32_t single_id, size_t n,
                           const int32_t *target_ids, int n_targets, double *grad_params, double *normal);
int mrl_ggx_grad_queue(mrl_ctx *ctx, const float *wi, const float *wo, const float *grad_rgb, const float *curv_rgb,
                       const int32_t *mat, int32_t single_id,
                       const uint32_t *queue, const uint32_t *queue_count, size_t capacity,
                       const int32_t *target_ids, int n_targets, double *grad_params, double *normal);

#ifdef __cplusplus
}
#endif
#endif
