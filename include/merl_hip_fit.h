/* merl_hip_fit.h — the fitting extension of the C ABI of libmerl_hip.so: calls that turn measurements into analytic materials.
 * It includes merl_hip.h (contexts, materials, status codes, mrl_eval_batch) and adds to it; the library exports both sets.
 * The core header's function list is what the host-binding tests pin one by one; calls added here are listed in
 * host.FIT_ABI_SYMBOLS and checked against this header by tests/test_ggx_grad_cpu.py. */
#ifndef MERL_HIP_FIT_H
#define MERL_HIP_FIT_H

#include "merl_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- fitting a GGX conductor: the parameter gradient of eval ----
 * The seven parameters of a GGX material, in the order p = (alpha, eta_r, eta_g, eta_b, k_r, k_g, k_b).  With
 *     J_uc = d eval_c(wi_u, wo_u) / d p      (a 7-vector per unit u and channel c)
 * taken at the material's stored Float parameters and evaluated in f64, where eval is exactly what mrl_eval_batch returns for a
 * GGX id — F D G1(i) G1(o) / (4 cos(theta_i)), the cosine of wo folded in; GGX ignores MRL_OPT_COSINE_FACTOR — the call computes
 *     grad_params[7]   += sum_u sum_c g_uc J_uc             g = grad_rgb = dL / d eval
 *     normal[7][7]     += sum_u sum_c h_uc J_uc J_uc^T      h = curv_rgb = d2L / d eval2, NULL = 1; normal may be NULL
 *   - grad_params alone is the vector-Jacobian product: what Adam / L-BFGS on any loss, or the backward pass of a differentiable
 *     renderer, need;
 *   - grad_params with normal is one Gauss-Newton / Levenberg-Marquardt step for any separable loss (sum w (eval - y)^2: g = 2 w r,
 *     h = 2 w).
 * Both outputs are ACCUMULATED into: the caller zeroes them, a second call adds to the first.  Channel c depends on alpha, eta_c
 * and k_c only: the entries of normal that couple two different channels are structurally zero and are not touched; both
 * triangles of the others are written (with the same value: normal stays symmetric bit for bit if it was).  wi, wo, grad_rgb,
 * curv_rgb: [n][3] f32.
 * A unit that eval masks (cos(theta_i) <= 0, cos(theta_o) <= 0, a NaN / inf / zero-length direction), or for which one of eval's
 * own D / G1 selects returns 0, contributes nothing, whatever its grad_rgb and curv_rgb hold (NaN and inf included).
 * id: a live GGX material; table, n-channel, RGL, spectral, released and unknown ids: MRL_ERR_MATERIAL.  NULL wi, wo, grad_rgb or
 * grad_params: MRL_ERR_INVALID; pointers (the outputs count as one more array) all host or all device (MRL_ERR_POINTER_MIX);
 * n == 0 is MRL_OK and touches nothing.  Device pointers: asynchronous on the context's stream.  Host arrays go through the
 * staged chunk loop (MRL_OPT_HOST_CHUNK); every chunk adds to one device array of 7 + 49 doubles, which is added to the caller's
 * at the end.
 * DETERMINISM (a contract of this call): there are no atomics — every block writes one row of partial sums to a workspace, one
 * block adds the rows up in a fixed order — and the grid depends on n and the device alone, so two device-pointer calls with the
 * same inputs on the same device and options return bit-identical outputs, and grad_params has the same bits with and without
 * normal.  The workspace (256 B per block, 3 blocks per compute unit: 196 KB on 256 CUs) is kept by the context, reported by
 * mrl_memory_info as workspace and, like the other workspaces, not counted against MRL_OPT_MEMORY_LIMIT_MB.
 * With a material id per unit and over wavefront queues, onto several GGX materials at once: mrl_ggx_grad_batch_mat /
 * mrl_ggx_grad_queue of merl_hip_fit_ggx.h.  Not offered: device groups (mrl_group_*), the one-unit paths.  The gradient with
 * respect to the directions wi, wo is mrl_ggx_grad_dir_batch / mrl_ggx_grad_dir_queue of merl_hip_diff.h. */
int mrl_ggx_grad_batch(mrl_ctx *ctx, const float *wi, const float *wo, const float *grad_rgb, const float *curv_rgb,
                       int32_t id, size_t n, double grad_params[7], double *normal);

#ifdef __cplusplus
}
#endif
#endif
