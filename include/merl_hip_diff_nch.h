/* merl_hip_diff_nch.h — the direction gradient of eval on N-CHANNEL TABLE materials (mrl_material_upload_table_nch /
 * mrl_material_load_table_nch: 1..32 channels — monochrome, RGB + alpha, spectral): the n-channel twin of merl_hip_diff_table.h, which
 * it includes (and with it merl_hip_diff.h and merl_hip.h: contexts, materials, status codes, options); the library exports all four
 * sets.  Calls added here are listed in host.DIFF_NCH_ABI_SYMBOLS and checked against this header by tests/test_nch_dir_grad_cpu.py.
 * DESIGN.md §5k. */
#ifndef MERL_HIP_DIFF_NCH_H
#define MERL_HIP_DIFF_NCH_H

#include "merl_hip_diff_table.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- the operator ----
 * The one of merl_hip_diff_table.h with c running over the n_channels channels of the call: E_c(wi, wo) = T_c(x(a, b)) kappa is the
 * real-valued function mrl_eval_batch_nch rounds — a = wi / |wi|, b = wo / |wo|, x the table coordinates of the material's
 * parameterisation, T_c the trilinear interpolant of the material's STORED Float texels with eval's cell selection, its clamped and
 * periodic axes and the half-texel shift of MRL_OPT_NODE = 1, kappa the raw Float wo.z or 1 under MRL_OPT_COSINE_FACTOR = 1.  Per
 * unit u the calls write the vector-Jacobian products
 *     grad_wi[u] = sum_c grad_values[u][c] dE_c / d wi          grad_wo[u] = sum_c grad_values[u][c] dE_c / d wo
 * wi, wo, grad_wi, grad_wo: [n][3] f32; grad_values: [n][n_channels] f32 with a unit's channels adjacent, like out_values of
 * mrl_eval_batch_nch (rows are 4-byte aligned only).  The outputs are OVERWRITTEN per unit, not accumulated into.
 * What is differentiated is the exact interpolant, not eval's rounded arithmetic.  Per channel the cell's texels are first taken
 * relative to corner 0 in f64 (the difference of two Floats is exact there) and only then meet grad_values; the channels are summed
 * in ascending order in one chain of fused multiply-adds: the rounding error scales with the variation of each channel inside the
 * cell, never with a channel's magnitude, and a channel whose grad_values entry is 0 changes nothing — an RGB table stored in
 * three channels of a wider table returns the numbers of mrl_table_grad_dir_batch.  Padding channels of the device image never
 * enter.
 * Everything else is the contract of mrl_table_grad_dir_batch / mrl_table_grad_dir_queue, word for word:
 * T is piecewise trilinear: the gradient is the one of the cell eval selects.  A clamped fraction has derivative 0 while its clamp
 * is active; the padded upper end has derivative 0 through its equal texels.  Where a coordinate map has no derivative — half / diff:
 * h == n, retro-reflection, px == py == 0; the standard forms: a direction exactly at the normal — that coordinate's term is dropped.
 * Every output is finite for every finite input: a component beyond the Float range is written as +-FLT_MAX, and one that a
 * grad_values entry near FLT_MAX turns into inf - inf inside is written as 0.
 * MRL_OPT_LOOKUP = 0 (nearest): grad_wi = 0, grad_wo = (d kappa / d wo.z) sum_c g_c T_c e_z.  MRL_OPT_NEGATIVE = 1 (keep)
 * differentiates the raw texels; MRL_OPT_NEGATIVE = 2 (renormalise): MRL_ERR_INVALID.
 * Identities: grad_wi[u] . wi[u] = 0; grad_wo[u] . wo[u] = sum_c grad_values[u][c] E_c (Euler's identity) with the cosine factor, 0
 * without it; for unnormalised inputs grad_wi scales with 1 / |w|.
 * Dead units — eval's: wi.z <= 0, wo.z <= 0, a NaN / inf component — get exactly +0.0f in both outputs, whatever their grad_values
 * hold (NaN and inf included).
 * n_channels: 1..32, otherwise what mrl_eval_batch_nch returns for it (MRL_ERR_INVALID); n_channels == 3 forwards to
 * mrl_table_grad_dir_batch / mrl_table_grad_dir_queue (RGB materials), as every *_nch call does.
 * Materials: mat == NULL: every unit uses single_id, which must be a live n-channel table of exactly n_channels channels
 * (MRL_ERR_MATERIAL otherwise).  mat != NULL: one id per unit; a unit whose id names no live n-channel table of exactly n_channels
 * channels (out of range, negative, released, another width, an RGB table, a GGX, RGL or spectral material) gets zeros.  Tables of
 * different dims and parameterisations may meet in one launch.
 * One of grad_wi / grad_wo may be NULL: that gradient is then not written; both NULL: MRL_ERR_INVALID.  NULL wi, wo or grad_values:
 * MRL_ERR_INVALID.  Pointers all host or all device (MRL_ERR_POINTER_MIX).  Device pointers: asynchronous on the context's stream;
 * no workspace, no reduction, no atomics.  n == 0 / capacity == 0: MRL_OK, nothing is touched.
 * mrl_table_grad_dir_batch_nch takes host arrays as well, through the staged chunk loop (MRL_OPT_HOST_CHUNK), mat included.
 * mrl_table_grad_dir_queue_nch follows mrl_eval_queue_nch: device pointers only; it processes the slots queue[0 .. min(*queue_count,
 * capacity)), reads a slot's inputs from and writes its outputs to the slot named, leaves every other slot untouched;
 * capacity <= 2^32; capturable in a HIP graph (the count is read on the device at run time).
 * DETERMINISM (a contract of these calls): a unit's output bits depend on its own inputs, its material and the context's options
 * alone — the whole-array, material-id, queue and host-array forms return identical bits for the same unit, whatever n, the grid
 * or the unit's position; grad_wi has the same bits with and without grad_wo.
 * Not offered: spectral RGL materials (RGB RGL materials: merl_hip_diff_rgl.h), device groups (mrl_group_*), the one-unit paths, second derivatives, gradients of pdf
 * and sample, the renormalising blend (MRL_OPT_NEGATIVE = 2).  The adjoint in an n-channel table's texels: merl_hip_fit_nch.h. */
int mrl_table_grad_dir_batch_nch(mrl_ctx *ctx, const float *wi, const float *wo, const float *grad_values,
                                 const int32_t *mat, int32_t single_id, size_t n, int n_channels,
                                 float *grad_wi, float *grad_wo);
int mrl_table_grad_dir_queue_nch(mrl_ctx *ctx, const float *wi, const float *wo, const float *grad_values,
                                 const int32_t *mat, int32_t single_id,
                                 const uint32_t *queue, const uint32_t *queue_count, size_t capacity, int n_channels,
                                 float *grad_wi, float *grad_wo);

#ifdef __cplusplus
}
#endif
#endif
