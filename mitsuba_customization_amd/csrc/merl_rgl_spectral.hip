// merl_rgl_spectral.hip — spectral RGL materials ("optional spectral channels, RGL/.bsdf"): the calls.
// A spectral file of the RGL material database holds "spectra" [n_phi][n_theta][n_wavelengths][res][res] over a "wavelengths" grid
// where the *_rgb.bsdf variant holds "rgb"; upstream Mitsuba 3's `measured` plugin, in its spectral variants, evaluates it with the
// ray's wavelengths as a third interpolated parameter.  So do these entry points: W values per unit at the wavelengths the caller
// passes per unit (wavelengths [n][W] — what hero-wavelength rendering carries per ray), or at the file's own nodes (wavelengths ==
// NULL, W = the number of nodes); pdf and the sampled direction are wavelength-free.  Three forms: whole arrays of one material
// (*_spectral_batch), whole arrays with a material id per unit (*_spectral_batch_mat), a wavefront queue with or without ids
// (*_spectral_queue) — what a spectral wavefront integrator holds: per-slot hero wavelengths, a queue of the slots per material.
// PARITY UNPINNED: no spectral file, no upstream source exists offline (oracle/rgl_oracle.c, rgl_eval_pdf_spectral, is the checker).
#include "merl_ctx.hpp"

using namespace mrlabi;

namespace {

// a spectral call: W values per unit at the wavelengths wl [n][W] (NULL: the file's own nodes).  Any mode but MODE_PDF (the RGB pdf call
// serves these materials); n is the number of units, in the queue form the capacity of the slot arrays
BatchCall spectral(BatchCall c, const float *wl, int W)
{
    c.wl = wl; c.n_ch = W;
    return c;
}

// checks and launches the three forms: whole arrays of one material (mrl_*_spectral_batch), whole arrays with ids (*_spectral_batch_mat),
// a wavefront queue with or without ids (*_spectral_queue: units queue[0 .. min(*queue_count, n)))
int run_spectral(mrl_ctx *ctx, const BatchCall &c, bool queued = false, const uint32_t *queue = nullptr, const uint32_t *queue_count = nullptr)
{
    if (!ctx) return MRL_ERR_INVALID;
    MRL_GUARD(ctx);
    if (c.n == 0) return MRL_OK;
    const int W = c.n_ch;
    const StreamList streams = streams_of(c);
    if (first_null(streams) || (queued && (!queue || !queue_count))) return fail(ctx, MRL_ERR_INVALID, "null array argument");
    if (queued && c.n > ((size_t)1 << 32)) return fail(ctx, MRL_ERR_INVALID, "queue capacity exceeds 2^32 (indices are uint32)");
    const MaterialHost *single = nullptr;
    if (c.mat) {
        // the materials of one call may have different wavelength grids: "the file's own nodes" names no one set of wavelengths
        if (!c.wl) return fail(ctx, MRL_ERR_INVALID, "a call with material ids needs per-unit wavelengths");
        if (W < 1 || W > 4096) return fail(ctx, MRL_ERR_INVALID, "1..4096 wavelengths per unit");
    } else {
        if (c.single_id < 0 || (size_t)c.single_id >= ctx->materials.size() || ctx->materials[(size_t)c.single_id].released) return fail(ctx, MRL_ERR_MATERIAL, "unknown material id");
        single = &ctx->materials[(size_t)c.single_id];
        if (single->dev.kind != mrl::KIND_RGL_SPECTRAL)
            return fail(ctx, MRL_ERR_MATERIAL, "the spectral entry points evaluate spectral RGL materials (mrl_material_upload_rgl_spectral)");
        if (W < 1 || W > 4096) return fail(ctx, MRL_ERR_INVALID, "1..4096 wavelengths per unit");
        if (!c.wl && W != single->rgl.n_wl)
            return fail(ctx, MRL_ERR_INVALID, "without a wavelength array the values are those at the file's " + std::to_string(single->rgl.n_wl) + " wavelength nodes");
    }
    MRL_HIP(ctx, hipSetDevice(ctx->device));
    const int kind = common_kind({ queue, queue_count }, streams);
    if (queued && kind != 1) return fail(ctx, MRL_ERR_POINTER_MIX, "queue calls take device pointers only");
    if (kind < 0) return fail(ctx, MRL_ERR_POINTER_MIX, "host and device pointers mixed in one call");
    auto launch = [&](const BatchCall &d) -> int {
        mrl::BatchArgs a = batch_args(ctx, d);
        a.idx = queue; a.idx_count = queue_count;
        MRL_HIP(ctx, mrl::launch_rgl_spectral_q(d.mode, a, single ? &single->rgl : nullptr, d.wl, W, ctx->rgl_search, ctx->compute_units, ctx->stream));
        return MRL_OK;
    };
    if (kind == 1) return launch(c);
    // host arrays: staged through HBM in chunks of at most 256 MiB of slot (W may be 4096; a renderer that holds spectral rays on the host
    // hands over a few million at a time)
    return run_host_staged(ctx, streams, c.n, (size_t)256 << 20, [&](char *const *addr, size_t m) { return launch(on_slot(c, addr, m)); });
}

} // namespace

extern "C" {

int mrl_eval_spectral_batch(mrl_ctx *ctx, const float *wi, const float *wo, const float *wavelengths, int n_wavelengths, int32_t id, size_t n, float *out_values)
{
    return run_spectral(ctx, spectral({ mrl::MODE_EVAL, wi, wo, nullptr, nullptr, id, n, out_values, nullptr, nullptr, nullptr, nullptr }, wavelengths, n_wavelengths));
}
int mrl_eval_pdf_spectral_batch(mrl_ctx *ctx, const float *wi, const float *wo, const float *wavelengths, int n_wavelengths, int32_t id, size_t n,
                                float *out_values, float *out_pdf)
{
    return run_spectral(ctx, spectral({ mrl::MODE_EVAL_PDF, wi, wo, nullptr, nullptr, id, n, out_values, out_pdf, nullptr, nullptr, nullptr }, wavelengths, n_wavelengths));
}
int mrl_sample_spectral_batch(mrl_ctx *ctx, const float *wi, const float *u, const float *wavelengths, int n_wavelengths, int32_t id, size_t n,
                              float *out_wo, float *out_pdf, float *out_weight)
{
    return run_spectral(ctx, spectral({ mrl::MODE_SAMPLE, wi, nullptr, u, nullptr, id, n, nullptr, nullptr, out_wo, out_pdf, out_weight }, wavelengths, n_wavelengths));
}
int mrl_eval_sample_spectral_batch(mrl_ctx *ctx, const float *wi, const float *wo, const float *u, const float *wavelengths, int n_wavelengths, int32_t id,
                                   size_t n, float *out_values, float *out_pdf, float *out_wo, float *out_pdf2, float *out_weight)
{
    return run_spectral(ctx, spectral({ mrl::MODE_EVAL_SAMPLE, wi, wo, u, nullptr, id, n, out_values, out_pdf, out_wo, out_pdf2, out_weight }, wavelengths, n_wavelengths));
}

// ---- over a wavefront queue (device pointers; mat == NULL: the material single_id) ----
int mrl_eval_spectral_queue(mrl_ctx *ctx, const float *wi, const float *wo, const float *wavelengths, int n_wavelengths, const int32_t *mat, int32_t single_id,
                            const uint32_t *queue, const uint32_t *queue_count, size_t capacity, float *out_values)
{
    return run_spectral(ctx, spectral({ mrl::MODE_EVAL, wi, wo, nullptr, mat, single_id, capacity, out_values, nullptr, nullptr, nullptr, nullptr }, wavelengths, n_wavelengths),
                        true, queue, queue_count);
}
int mrl_eval_pdf_spectral_queue(mrl_ctx *ctx, const float *wi, const float *wo, const float *wavelengths, int n_wavelengths, const int32_t *mat, int32_t single_id,
                                const uint32_t *queue, const uint32_t *queue_count, size_t capacity, float *out_values, float *out_pdf)
{
    return run_spectral(ctx, spectral({ mrl::MODE_EVAL_PDF, wi, wo, nullptr, mat, single_id, capacity, out_values, out_pdf, nullptr, nullptr, nullptr }, wavelengths, n_wavelengths),
                        true, queue, queue_count);
}
int mrl_sample_spectral_queue(mrl_ctx *ctx, const float *wi, const float *u, const float *wavelengths, int n_wavelengths, const int32_t *mat, int32_t single_id,
                              const uint32_t *queue, const uint32_t *queue_count, size_t capacity, float *out_wo, float *out_pdf, float *out_weight)
{
    return run_spectral(ctx, spectral({ mrl::MODE_SAMPLE, wi, nullptr, u, mat, single_id, capacity, nullptr, nullptr, out_wo, out_pdf, out_weight }, wavelengths, n_wavelengths),
                        true, queue, queue_count);
}
int mrl_eval_sample_spectral_queue(mrl_ctx *ctx, const float *wi, const float *wo, const float *u, const float *wavelengths, int n_wavelengths, const int32_t *mat,
                                   int32_t single_id, const uint32_t *queue, const uint32_t *queue_count, size_t capacity,
                                   float *out_values, float *out_pdf, float *out_wo, float *out_pdf2, float *out_weight)
{
    return run_spectral(ctx, spectral({ mrl::MODE_EVAL_SAMPLE, wi, wo, u, mat, single_id, capacity, out_values, out_pdf, out_wo, out_pdf2, out_weight }, wavelengths, n_wavelengths),
                        true, queue, queue_count);
}

// ---- whole arrays with a material id per unit (host or device pointers) ----
int mrl_eval_spectral_batch_mat(mrl_ctx *ctx, const float *wi, const float *wo, const float *wavelengths, int n_wavelengths, const int32_t *mat, size_t n,
                                float *out_values)
{
    return run_spectral(ctx, spectral({ mrl::MODE_EVAL, wi, wo, nullptr, mat, -1, n, out_values, nullptr, nullptr, nullptr, nullptr }, wavelengths, n_wavelengths));
}
int mrl_eval_pdf_spectral_batch_mat(mrl_ctx *ctx, const float *wi, const float *wo, const float *wavelengths, int n_wavelengths, const int32_t *mat, size_t n,
                                    float *out_values, float *out_pdf)
{
    return run_spectral(ctx, spectral({ mrl::MODE_EVAL_PDF, wi, wo, nullptr, mat, -1, n, out_values, out_pdf, nullptr, nullptr, nullptr }, wavelengths, n_wavelengths));
}
int mrl_sample_spectral_batch_mat(mrl_ctx *ctx, const float *wi, const float *u, const float *wavelengths, int n_wavelengths, const int32_t *mat, size_t n,
                                  float *out_wo, float *out_pdf, float *out_weight)
{
    return run_spectral(ctx, spectral({ mrl::MODE_SAMPLE, wi, nullptr, u, mat, -1, n, nullptr, nullptr, out_wo, out_pdf, out_weight }, wavelengths, n_wavelengths));
}
int mrl_eval_sample_spectral_batch_mat(mrl_ctx *ctx, const float *wi, const float *wo, const float *u, const float *wavelengths, int n_wavelengths, const int32_t *mat,
                                       size_t n, float *out_values, float *out_pdf, float *out_wo, float *out_pdf2, float *out_weight)
{
    return run_spectral(ctx, spectral({ mrl::MODE_EVAL_SAMPLE, wi, wo, u, mat, -1, n, out_values, out_pdf, out_wo, out_pdf2, out_weight }, wavelengths, n_wavelengths));
}

int mrl_material_wavelengths(mrl_ctx *ctx, int id, int *n_wavelengths, float *out, size_t max_floats)
{
    if (!ctx) return MRL_ERR_INVALID;
    MRL_GUARD(ctx);
    if (!n_wavelengths) return fail(ctx, MRL_ERR_INVALID, "null argument");
    if (id < 0 || (size_t)id >= ctx->materials.size() || ctx->materials[(size_t)id].released) return fail(ctx, MRL_ERR_MATERIAL, "unknown material id");
    const MaterialHost &mh = ctx->materials[(size_t)id];
    if (mh.dev.kind != mrl::KIND_RGL_SPECTRAL) return fail(ctx, MRL_ERR_MATERIAL, "not a spectral material");
    *n_wavelengths = mh.rgl.n_wl;
    if (out) {
        if (max_floats < (size_t)mh.rgl.n_wl) return fail(ctx, MRL_ERR_INVALID, "output array too small");
        MRL_HIP(ctx, hipSetDevice(ctx->device));
        MRL_HIP(ctx, hipMemcpy(out, mh.rgl.wavelengths, (size_t)mh.rgl.n_wl * sizeof(float), hipMemcpyDeviceToHost));
    }
    return MRL_OK;
}

} // extern "C"
