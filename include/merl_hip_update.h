/* merl_hip_update.h — new values for a resident material, in place: the planar array of a table or an n-channel table, the
 * parameters of a GGX conductor; and the read-back of a table's row marginal.  Includes merl_hip.h (contexts, materials, status
 * codes, options); the library exports both sets.  Calls added here are listed in host.UPDATE_ABI_SYMBOLS and checked against this
 * header by tests/test_update_cpu.py.  DESIGN.md §5o. */
#ifndef MERL_HIP_UPDATE_H
#define MERL_HIP_UPDATE_H

#include "merl_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* flags of mrl_material_update_table */
#define MRL_UPDATE_KEEP_SAMPLING 1   /* leave both sampling tables as they are */

/* ---- tables ----
 * Rewrites the image of a live MERL / customized_measurement RGB table (either layout) or n-channel table (1..32 channels) from
 * `planar`, which has the layout and size of what the material was uploaded from: [n_channels][n_th][n_td][n_pd] f64.  `planar` is
 * a host or a device pointer, told apart as the batch calls tell their arrays apart.  Dims, layout, parameterisation, channel
 * scales and kind stay the material's own; the context's MRL_OPT_NEGATIVE applies as at upload.
 * IN PLACE: the id, the addresses of the texels and of both sampling tables, the material's entry in the device array, the arena
 * placement and the material bytes of mrl_memory_info are unchanged.  Captured graphs and queues that name the material see the
 * new values on their next replay.  The texels are written by the kernels an upload uses: the image is the one a fresh upload of
 * `planar` would give, bit for bit.
 * STREAM-ORDERED on the context's stream.  A device-pointer call allocates nothing, synchronises nothing and copies nothing from
 * pageable host memory, so it can be captured in a HIP graph — once the material's workspace exists (below): a first call outside
 * the capture sees to that.  Exception: a context whose one-unit mailbox service has been opened (the mrl_scalar_* calls) drains its
 * stream at the end of every update, since the service runs on a stream of its own and must not meet a half-written image;
 * inside a stream capture that wait is left out, and so is every guarantee about one-unit calls that overlap a replay.
 * A host-pointer call stages the array through the context's grow-only staging workspace (no allocation per call once it has its
 * size) and returns when the update has run, so the source may be reused at once.
 * SAMPLING: unless MRL_UPDATE_KEEP_SAMPLING is set, the row marginal (the cdf and c parts of s | cdf | c) is rebuilt on the device
 * from `planar`: per row the sum over its cells and channels of w_ch max(v scale_ch, 0) — the luminance weights for RGB tables, 1 /
 * n_channels otherwise — then the 1 % floor, the flat lobe of the parameterisations whose rows are not theta_h, and the flat
 * marginal of an all-non-positive table, as at upload.  The sums are deterministic: no atomics, rows cut into segments of a fixed
 * length and combined in a fixed order that does not depend on the launch's grid, so two updates from the same values give the same
 * bits.  They are NOT the bits of an upload's marginal, which the host sums in another order: cdf and c agree with it to rounding
 * (all terms are non-negative: about (n_channels n_td n_pd + 2 n_th) 2^-53 relative).  The s part depends on n_th alone and is
 * left untouched.  The conditional rows P(theta_h | theta_i) of an RGB table are then rebuilt from the new texels by the kernels an
 * upload uses — they read the texels and s only, so they ARE a fresh upload's bits — under the context's current lookup / node
 * options.
 * With MRL_UPDATE_KEEP_SAMPLING both are skipped: a loop that only evaluates does not pay for them, and a stale proposal is still
 * a valid one — pdf and sample read the same tables, so weight == eval / pdf holds.
 * WORKSPACE: per material, allocated by its first update and never moved or resized afterwards (row-segment sums, the work array
 * of the conditional rows, an n-channel table's scales); freed with the material.  mrl_memory_info reports it as workspace; it is
 * not counted against MRL_OPT_MEMORY_LIMIT_MB.  If it does not fit: MRL_ERR_OOM, the material untouched.
 * HOST IMAGES: an mrl_host_table taken earlier is an immutable snapshot and keeps the old values; one taken afterwards has the new
 * ones.  The update pauses the one-unit mailbox service as an upload does.
 * Refused with MRL_ERR_MATERIAL, the material untouched: a GGX, RGL or spectral material; a released, negative or out-of-range id; a
 * table restored from an image file (it carries no channel scales — the table adjoint refuses it for the same reason).
 * MRL_ERR_INVALID: NULL planar, unknown flag bits.
 * The measured values of an RGB RGL material: mrl_material_update_rgl_values of merl_hip_fit_rgl.h (this call refuses the kind).
 * Not offered: device groups, spectral RGL materials, plugin properties, an update that changes dims, layout or channel count. */
int mrl_material_update_table(mrl_ctx *ctx, int id, const double *planar, int flags);

/* ---- GGX conductors ----
 * New parameters for a live GGX material, validated exactly as mrl_material_ggx validates them (same statuses); any other id:
 * MRL_ERR_MATERIAL.  Rewrites the host descriptor, and the material's entry in the device array by a one-thread kernel on the
 * context's stream (nothing is read from host memory at run time).
 * ONE ASYMMETRY: a single-material launch takes the descriptor BY VALUE in its kernel arguments, so a graph captured over a
 * single-id GGX call holds the parameters of its capture.  Calls with a material id per unit read the device array and see the
 * update on their next replay. */
int mrl_material_update_ggx(mrl_ctx *ctx, int id, float alpha, const float eta[3], const float k[3]);

/* ---- read-back ----
 * The row marginal of a table material (RGB or n-channel) as the device holds it: s[n_th + 1] | cdf[n_th + 1] | c[n_th], 3 n_th + 2
 * doubles; the twin of mrl_material_sampling2d.  Waits for the context's stream first.  out == NULL: MRL_OK if the material has
 * one.  MRL_ERR_MATERIAL: not a live table material; MRL_ERR_INVALID: max_doubles too small. */
int mrl_material_sampling(mrl_ctx *ctx, int id, double *out, size_t max_doubles);

#ifdef __cplusplus
}
#endif
#endif
