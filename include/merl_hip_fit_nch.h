/* merl_hip_fit_nch.h — the table adjoint of eval on N-CHANNEL TABLE materials (mrl_material_upload_table_nch /
 * mrl_material_load_table_nch: 1..32 channels — monochrome, RGB + alpha, spectral), over whole arrays, with a material id per unit and
 * over wavefront queues, onto several target tables in one launch: the n-channel twin of merl_hip_fit_table.h, which it includes (and
 * with it merl_hip.h: contexts, materials, status codes, options); the library exports all sets.  Calls added here are listed in
 * host.FIT_NCH_ABI_SYMBOLS and checked against this header by tests/test_table_grad_nch_cpu.py.  DESIGN.md §5n. */
#ifndef MERL_HIP_FIT_NCH_H
#define MERL_HIP_FIT_NCH_H

#include "merl_hip_fit_table.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- the operator ----
 * For every target table k the calls compute G_k += A_k^T g.  Row u of A_k holds, per channel c of the n_channels channels of the
 * call, guard x kappa x scale_k[c] x the corner weights mrl_eval_batch_nch itself blends with: kappa is the raw Float wo.z, or 1 with
 * MRL_OPT_COSINE_FACTOR = 1; the weights are the F64 products of the f64 fractions (not the Float weights of the RGB path) at the
 * cell eval's own lookup selects under target k's dims and parameterisation and the context's MRL_OPT_LOOKUP / MRL_OPT_NODE; a
 * nearest lookup puts all weight on corner 0.  A_k is restricted to the units whose material is target k.  One launch serves all
 * targets and all channels; the streams are read once and the coordinate transform is computed once per unit.
 * Everything else is the contract of merl_hip_fit_table.h, word for word, with these differences:
 * Arrays: grad_values is [n][n_channels] f32 with a unit's channels adjacent, like out_values of mrl_eval_batch_nch (rows are 4-byte
 * aligned only: a 5-channel row starts at any multiple of 4 bytes).  grad_planar holds the targets end to end: target k is
 * [n_channels][n_th][n_td][n_pd] f64, the layout of mrl_material_upload_table_nch's input, at the offset n_channels sum_{j<k}
 * cells_j.  It is ACCUMULATED into; a texel that nothing reaches keeps its bits (-0 and NaN payloads survive).
 * Materials: target_ids is ALWAYS a host array.  Every target must be a live n-channel table of exactly n_channels channels that
 * carries its channel scales (not one restored from an image file): MRL_ERR_MATERIAL otherwise.  mat != NULL: mat[i] (the queue
 * form: mat[slot]); mat == NULL: every unit uses single_id.  A unit whose id is not among the targets contributes nothing, whatever
 * its grad_values hold (NaN and inf included) — a table of another width, an RGB table, a GGX, RGL or spectral material, a
 * released, negative or out-of-range id.  Dead units — eval's guard: wi.z <= 0, wo.z <= 0, a NaN / inf component — contribute
 * nothing either, whatever their grad_values hold.  Targets of different dims and parameterisations may meet in one launch.
 * n_channels: 1..32, otherwise what mrl_eval_batch_nch returns for it (MRL_ERR_INVALID); n_channels == 3 forwards to
 * mrl_table_grad_batch_mat / mrl_table_grad_queue (RGB materials, Float weights), as every *_nch call does.
 * MRL_ERR_INVALID: a target listed twice; n_targets < 1 or above MRL_TABLE_GRAD_MAX_TARGETS; targets that
 * mrl_table_grad_layout_nch refuses; NULL wi, wo, grad_values, target_ids or grad_planar (the queue form: NULL queue or
 * queue_count); MRL_OPT_NEGATIVE = 2 (renormalise: eval is not linear in the table).
 * Pointers — wi, wo, grad_values, mat, grad_planar — all host or all device: MRL_ERR_POINTER_MIX.
 * n == 0 / capacity == 0: MRL_OK, nothing is touched, whatever the other arguments are.
 * mrl_table_grad_batch_nch takes host arrays as well, through the staged chunk loop (MRL_OPT_HOST_CHUNK): grad_values is a stream of
 * 4 n_channels bytes per unit, mat one more 4-byte stream.  A host-array call returns when grad_planar is complete and holds a
 * device copy of it (8 n_channels bytes per cell) for its duration.
 * mrl_table_grad_queue_nch follows mrl_eval_queue_nch: device pointers only (MRL_ERR_POINTER_MIX); it processes the slots
 * queue[0 .. min(*queue_count, capacity)) and reads a slot's wi, wo, grad_values and mat from the slot named; a slot listed twice
 * contributes twice; capacity <= 2^32 (MRL_ERR_INVALID above).  The count is read on the device at run time and the call copies
 * nothing from host memory — the channel scales are applied by the fold, which takes them by value —, so it is capturable in a
 * HIP graph once the workspace below has its size (a first call outside the capture sees to that).
 * Workspace: gradient bricks per (cell, channel group of 4) — 256 B times ceil(n_channels / 4) per cell of every target, for every
 * width, 1 and 2 included — in the workspace mrl_table_grad_batch uses; cleared once and folded once per call (into the targets'
 * slices of grad_planar and nothing else); mrl_memory_info reports it; it is not counted against MRL_OPT_MEMORY_LIMIT_MB; if it
 * does not fit: MRL_ERR_OOM.  MERL dims (90 x 90 x 180 = 1,458,000 cells): 16 channels 1.49 GB, 32 channels 2.99 GB.
 * Accuracy: the sums are f64 atomics in no fixed order: two calls agree to f64 rounding, not bit for bit.  Two units are added
 * together before they reach memory only when they share target and cell.
 * MRL_OPT_TABLE_GRAD_KERNEL: 0 auto (lanes of a wave that share a cell are summed first when at least four share the first live
 * lane's), 2 never, 3 always.  Value 1, the plain planar form of the RGB calls, is not built for n-channel tables: it behaves as 2.
 * RGB RGL materials: merl_hip_fit_rgl.h.  Not offered: device groups (mrl_group_*), spectral RGL materials, the one-unit paths.  (An autograd wrapper that returns a table gradient:
 * diff.table_eval_nch(tables=), over mrl_material_update_table of merl_hip_update.h.) */
int mrl_table_grad_batch_nch(mrl_ctx *ctx, const float *wi, const float *wo, const float *grad_values,
                             const int32_t *mat, int32_t single_id, size_t n, int n_channels,
                             const int32_t *target_ids, int n_targets, double *grad_planar);
int mrl_table_grad_queue_nch(mrl_ctx *ctx, const float *wi, const float *wo, const float *grad_values,
                             const int32_t *mat, int32_t single_id,
                             const uint32_t *queue, const uint32_t *queue_count, size_t capacity, int n_channels,
                             const int32_t *target_ids, int n_targets, double *grad_planar);

/* Where each target's slice of grad_planar starts — the arithmetic the two calls use, without a context or a device: dims is
 * [n_targets][3]; offsets_out (may be NULL) receives n_targets + 1 values in doubles: offsets_out[k] = n_channels sum_{j<k} cells_j,
 * and offsets_out[n_targets] the size of grad_planar.  MRL_ERR_INVALID, and offsets_out is then not to be used: everything
 * mrl_table_grad_layout refuses; n_channels outside 1..32; sum_k cells_k x ceil(n_channels / 4) above 2^31 - 1 — the kernels address
 * a brick of a call with one int index.  n_channels == 3 returns mrl_table_grad_layout's offsets.  The two calls above refuse exactly
 * the targets this function refuses. */
int mrl_table_grad_layout_nch(const int *dims, int n_targets, int n_channels, size_t *offsets_out);

#ifdef __cplusplus
}
#endif
#endif
