/* merl_hip_fit_table.h — the table adjoint of eval with a material id per unit and over wavefront queues, onto several target
 * tables in one launch: the multi-material twin of mrl_table_grad_batch of merl_hip.h, which it includes (contexts, materials,
 * status codes, options); the library exports both sets.  Calls added here are listed in host.FIT_TABLE_ABI_SYMBOLS and checked
 * against this header by tests/test_table_grad_mat_cpu.py.  DESIGN.md §5l. */
#ifndef MERL_HIP_FIT_TABLE_H
#define MERL_HIP_FIT_TABLE_H

#include "merl_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The most targets one call takes.  The targets' descriptors (48 B each) travel by value in the kernel arguments, so that a queue
 * call copies nothing from host memory at call time; 16 of them keep the arguments below 1 KiB of the 4 KiB a kernel may take,
 * and every lane compares its id with every descriptor, so the bound also bounds the per-unit search. */
#define MRL_TABLE_GRAD_MAX_TARGETS 16

/* ---- the operator ----
 * For every target table k the calls compute G_k += A_k^T g, where A_k is the operator of mrl_table_grad_batch (merl_hip.h) for
 * target k — guard x (cos(theta_o), or 1 with MRL_OPT_COSINE_FACTOR = 1) x scale_k[c] x the Float corner weights of eval's own
 * lookup under target k's dims and parameterisation and the context's MRL_OPT_LOOKUP / MRL_OPT_NODE — restricted to the units
 * whose material is target k.  One launch serves all targets; the streams are read once.
 * Targets and layout: target_ids is ALWAYS a host array of n_targets material ids, the tables whose gradient the caller wants.
 * grad_planar holds the targets end to end: target k occupies 3 n_th n_td n_pd doubles laid out like mrl_material_upload_table's
 * input ([3][n_th][n_td][n_pd]) at the offset sum_{j<k} of the earlier targets' sizes.  It is ACCUMULATED into, exactly as
 * mrl_table_grad_batch does; a texel that nothing reaches keeps its bits.
 * Material of a unit: mat != NULL: mat[i] (the queue form: mat[slot]); mat == NULL: every unit uses single_id.
 * Non-target units: a unit whose id is not among the targets contributes nothing, whatever its grad_rgb holds (NaN and inf
 * included) — another table, a GGX, n-channel, RGL or spectral material, a released, negative or out-of-range id.  Dead units are
 * masked as in mrl_table_grad_batch: eval's guard (wi.z <= 0, wo.z <= 0, a NaN / inf component), whatever their grad_rgb holds.
 * Mixed tables: targets of different dims and parameterisations may meet in one launch.  The lookup, node and cosine options are
 * the context's.
 * Target validation: every target must be a live MERL / customized_measurement RGB table that carries its channel scales (not one
 * restored from an image file): MRL_ERR_MATERIAL otherwise.  MRL_ERR_INVALID: a target listed twice; n_targets < 1 or above
 * MRL_TABLE_GRAD_MAX_TARGETS; more than 2^31 - 1 cells over all targets; NULL wi, wo, grad_rgb, target_ids or grad_planar (the
 * queue form: NULL queue or queue_count); MRL_OPT_NEGATIVE = 2 (renormalise: eval is not linear in the table).
 * Pointers — wi, wo, grad_rgb, mat, grad_planar — all host or all device: MRL_ERR_POINTER_MIX.
 * n == 0 / capacity == 0: MRL_OK, nothing is touched, whatever the other arguments are.
 * mrl_table_grad_batch_mat takes host arrays as well, through the staged chunk loop (MRL_OPT_HOST_CHUNK); mat is one more 4-byte
 * stream.  A host-array call returns when grad_planar is complete and holds a device copy of it (24 B per cell) for its duration.
 * mrl_table_grad_queue follows mrl_eval_queue: device pointers only (MRL_ERR_POINTER_MIX); it processes the slots
 * queue[0 .. min(*queue_count, capacity)) and reads a slot's wi, wo, grad_rgb and mat from the slot named; a slot listed twice
 * contributes twice; capacity <= 2^32 (MRL_ERR_INVALID above).  The count is read on the device at run time and the call copies
 * nothing from pageable host memory, so it is capturable in a HIP graph once the workspace below has its size (a first call
 * outside the capture sees to that).
 * Workspace: the gradient bricks of all targets live in the workspace mrl_table_grad_batch uses, 256 B per cell of every target,
 * cleared once and folded once per call (into the targets' slices of grad_planar and nothing else); mrl_memory_info reports it;
 * it is not counted against MRL_OPT_MEMORY_LIMIT_MB; if it does not fit: MRL_ERR_OOM.
 * Accuracy: as mrl_table_grad_batch — the sums are f64 atomics in no fixed order: two calls agree to f64 rounding, not bit for bit.
 * Two units are added together before they reach memory only when they share target and cell.  All four
 * MRL_OPT_TABLE_GRAD_KERNEL values serve these calls and give the same sums up to f64 rounding.
 * n-channel tables: merl_hip_fit_nch.h.  RGB RGL materials: merl_hip_fit_rgl.h.  Not offered: device groups (mrl_group_*), the one-unit paths.  The GGX parameter gradient with
 * ids and over queues is mrl_ggx_grad_batch_mat / mrl_ggx_grad_queue of merl_hip_fit_ggx.h. */
int mrl_table_grad_batch_mat(mrl_ctx *ctx, const float *wi, const float *wo, const float *grad_rgb,
                             const int32_t *mat, int32_t single_id, size_t n,
                             const int32_t *target_ids, int n_targets, double *grad_planar);

/* Where each target's slice of grad_planar starts — the arithmetic the two calls use, without a context or a device: dims is
 * [n_targets][3] (n_th, n_td, n_pd of target k, as mrl_material_info reports them); offsets_out (may be NULL) receives
 * n_targets + 1 values in doubles: offsets_out[k] = 3 sum_{j<k} cells_j, and offsets_out[n_targets] the size of grad_planar.
 * MRL_ERR_INVALID, and offsets_out is then not to be used: NULL dims; n_targets < 1 or above MRL_TABLE_GRAD_MAX_TARGETS; a dim
 * below 1; more than 2^31 - 1 cells over all targets — the kernels address the targets' cells with one int index.  The two calls
 * above refuse exactly the targets this function refuses. */
int mrl_table_grad_layout(const int *dims, int n_targets, size_t *offsets_out);
int mrl_table_grad_queue(mrl_ctx *ctx, const float *wi, const float *wo, const float *grad_rgb,
                         const int32_t *mat, int32_t single_id,
                         const uint32_t *queue, const uint32_t *queue_count, size_t capacity,
                         const int32_t *target_ids, int n_targets, double *grad_planar);

#ifdef __cplusplus
}
#endif
#endif
