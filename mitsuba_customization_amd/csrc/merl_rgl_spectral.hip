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

struct SpectralCall {
    int mode;                                        // a mrl::Mode other than MODE_PDF (the RGB pdf call serves these materials)
    const float *wi, *wo, *u, *wl;
    int W;
    int32_t id;
    size_t n;                                        // units; the queue form: the capacity of the slot arrays
    float *out_values, *out_pdf, *out_wo, *out_pdf2, *out_weight;
    const int32_t *mat = nullptr;                    // a material id per unit (id is then unused)
    bool queued = false;                             // the queue form: units queue[0 .. min(*queue_count, n))
    const uint32_t *queue = nullptr, *queue_count = nullptr;
};

// checks and launches the three forms: whole arrays of one material (mrl_*_spectral_batch), whole arrays with ids (*_spectral_batch_mat),
// a wavefront queue with or without ids (*_spectral_queue)
int run_spectral(mrl_ctx *ctx, const SpectralCall &c)
{
    if (!ctx) return MRL_ERR_INVALID;
    MRL_GUARD(ctx);
    const bool has_eval = mrl::mode_eval(c.mode), has_pdf = mrl::mode_pdf(c.mode), has_sample = mrl::mode_sample(c.mode);
    if (c.n == 0) return MRL_OK;
    if (!c.wi || (has_eval && (!c.wo || !c.out_values)) || (has_pdf && !c.out_pdf) || (has_sample && (!c.u || !c.out_wo || !c.out_pdf2 || !c.out_weight)))
        return fail(ctx, MRL_ERR_INVALID, "null array argument");
    if (c.queued && (!c.queue || !c.queue_count)) return fail(ctx, MRL_ERR_INVALID, "null array argument");
    if (c.queued && c.n > ((size_t)1 << 32)) return fail(ctx, MRL_ERR_INVALID, "queue capacity exceeds 2^32 (indices are uint32)");
    const MaterialHost *single = nullptr;
    if (c.mat) {
        // the materials of one call may have different wavelength grids: "the file's own nodes" names no one set of wavelengths
        if (!c.wl) return fail(ctx, MRL_ERR_INVALID, "a call with material ids needs per-unit wavelengths");
        if (c.W < 1 || c.W > 4096) return fail(ctx, MRL_ERR_INVALID, "1..4096 wavelengths per unit");
    } else {
        if (c.id < 0 || (size_t)c.id >= ctx->materials.size() || ctx->materials[(size_t)c.id].released) return fail(ctx, MRL_ERR_MATERIAL, "unknown material id");
        single = &ctx->materials[(size_t)c.id];
        if (single->dev.kind != mrl::KIND_RGL_SPECTRAL)
            return fail(ctx, MRL_ERR_MATERIAL, "the spectral entry points evaluate spectral RGL materials (mrl_material_upload_rgl_spectral)");
        if (c.W < 1 || c.W > 4096) return fail(ctx, MRL_ERR_INVALID, "1..4096 wavelengths per unit");
        if (!c.wl && c.W != single->rgl.n_wl)
            return fail(ctx, MRL_ERR_INVALID, "without a wavelength array the values are those at the file's " + std::to_string(single->rgl.n_wl) + " wavelength nodes");
    }
    MRL_HIP(ctx, hipSetDevice(ctx->device));
    const int kind = common_kind({ c.wi, has_eval ? c.wo : nullptr, has_sample ? c.u : nullptr, c.wl, c.mat, has_eval ? c.out_values : nullptr, has_pdf ? c.out_pdf : nullptr,
                                   has_sample ? c.out_wo : nullptr, has_sample ? c.out_pdf2 : nullptr, has_sample ? c.out_weight : nullptr, c.queue, c.queue_count });
    if (c.queued && kind != 1) return fail(ctx, MRL_ERR_POINTER_MIX, "queue calls take device pointers only");
    if (kind < 0) return fail(ctx, MRL_ERR_POINTER_MIX, "host and device pointers mixed in one call");
    auto launch = [&](const float *wi, const float *wo, const float *u, const float *wl, const int32_t *mat, size_t n, float *values, float *pdf, float *wo2,
                      float *pdf2, float *w) {
        mrl::BatchArgs a;
        std::memset(&a, 0, sizeof a);
        a.wi = wi; a.wo = wo; a.u = u; a.mat = mat; a.n = n;
        a.out_rgb = values; a.out_pdf = pdf; a.out_wo = wo2; a.out_pdf2 = pdf2; a.out_weight = w;
        a.opts = ctx->opts;
        if (!c.mat && !c.queued) return mrl::launch_rgl_spectral(c.mode, a, single->rgl, wl, c.W, ctx->rgl_search, ctx->compute_units, ctx->stream);
        a.materials = ctx->d_materials;
        a.n_materials = (int)ctx->materials.size();
        a.idx = c.queue; a.idx_count = c.queue_count;
        return mrl::launch_rgl_spectral_q(c.mode, a, single ? &single->rgl : nullptr, c.queued, wl, c.W, ctx->rgl_search, ctx->compute_units, ctx->stream);
    };
    if (kind == 1) {
        MRL_HIP(ctx, launch(c.wi, c.wo, c.u, c.wl, c.mat, c.n, c.out_values, c.out_pdf, c.out_wo, c.out_pdf2, c.out_weight));
        return MRL_OK;
    }
    // host arrays: staged through HBM in chunks (a renderer that holds spectral rays on the host hands over a few million at a time)
    const size_t W = (size_t)c.W;
    const size_t unit_floats = 3 + 3 + 2 + W + W + 1 + 3 + 1 + W + 1;
    const size_t chunk = std::min(c.n, std::max<size_t>(1, std::min(ctx->host_chunk, ((size_t)256 << 20) / (unit_floats * 4))));
    float *d = nullptr;
    MRL_ALLOC(ctx, hipMalloc((void **)&d, chunk * unit_floats * sizeof(float)));
    float *d_wi = d, *d_wo = d_wi + 3 * chunk, *d_u = d_wo + 3 * chunk, *d_wl = d_u + 2 * chunk, *d_val = d_wl + W * chunk, *d_pdf = d_val + W * chunk,
          *d_wo2 = d_pdf + chunk, *d_pdf2 = d_wo2 + 3 * chunk, *d_w = d_pdf2 + chunk;
    int32_t *d_mat = (int32_t *)(d_w + W * chunk);
    hipError_t e = hipSuccess;
    for (size_t off = 0; off < c.n && e == hipSuccess; off += chunk) {
        const size_t m = std::min(chunk, c.n - off);
        e = hipMemcpyAsync(d_wi, c.wi + 3 * off, 12 * m, hipMemcpyHostToDevice, ctx->stream);
        if (e == hipSuccess && has_eval) e = hipMemcpyAsync(d_wo, c.wo + 3 * off, 12 * m, hipMemcpyHostToDevice, ctx->stream);
        if (e == hipSuccess && has_sample) e = hipMemcpyAsync(d_u, c.u + 2 * off, 8 * m, hipMemcpyHostToDevice, ctx->stream);
        if (e == hipSuccess && c.wl) e = hipMemcpyAsync(d_wl, c.wl + W * off, 4 * W * m, hipMemcpyHostToDevice, ctx->stream);
        if (e == hipSuccess && c.mat) e = hipMemcpyAsync(d_mat, c.mat + off, 4 * m, hipMemcpyHostToDevice, ctx->stream);
        if (e == hipSuccess) e = launch(d_wi, d_wo, d_u, c.wl ? d_wl : nullptr, c.mat ? d_mat : nullptr, m, d_val, d_pdf, d_wo2, d_pdf2, d_w);
        if (e == hipSuccess && has_eval) e = hipMemcpyAsync(c.out_values + W * off, d_val, 4 * W * m, hipMemcpyDeviceToHost, ctx->stream);
        if (e == hipSuccess && has_pdf) e = hipMemcpyAsync(c.out_pdf + off, d_pdf, 4 * m, hipMemcpyDeviceToHost, ctx->stream);
        if (e == hipSuccess && has_sample) {
            e = hipMemcpyAsync(c.out_wo + 3 * off, d_wo2, 12 * m, hipMemcpyDeviceToHost, ctx->stream);
            if (e == hipSuccess) e = hipMemcpyAsync(c.out_pdf2 + off, d_pdf2, 4 * m, hipMemcpyDeviceToHost, ctx->stream);
            if (e == hipSuccess) e = hipMemcpyAsync(c.out_weight + W * off, d_w, 4 * W * m, hipMemcpyDeviceToHost, ctx->stream);
        }
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    }
    (void)hipFree(d);
    if (e != hipSuccess) { (void)hipGetLastError(); return fail(ctx, MRL_ERR_HIP, std::string("spectral call: ") + hipGetErrorString(e)); }
    return MRL_OK;
}

SpectralCall queue_call(SpectralCall c, const int32_t *mat, const uint32_t *queue, const uint32_t *queue_count)
{
    c.mat = mat; c.queued = true; c.queue = queue; c.queue_count = queue_count;
    return c;
}

SpectralCall mat_call(SpectralCall c, const int32_t *mat)
{
    c.mat = mat;
    return c;
}

} // namespace

extern "C" {

int mrl_eval_spectral_batch(mrl_ctx *ctx, const float *wi, const float *wo, const float *wavelengths, int n_wavelengths, int32_t id, size_t n, float *out_values)
{
    return run_spectral(ctx, { mrl::MODE_EVAL, wi, wo, nullptr, wavelengths, n_wavelengths, id, n, out_values, nullptr, nullptr, nullptr, nullptr });
}
int mrl_eval_pdf_spectral_batch(mrl_ctx *ctx, const float *wi, const float *wo, const float *wavelengths, int n_wavelengths, int32_t id, size_t n,
                                float *out_values, float *out_pdf)
{
    return run_spectral(ctx, { mrl::MODE_EVAL_PDF, wi, wo, nullptr, wavelengths, n_wavelengths, id, n, out_values, out_pdf, nullptr, nullptr, nullptr });
}
int mrl_sample_spectral_batch(mrl_ctx *ctx, const float *wi, const float *u, const float *wavelengths, int n_wavelengths, int32_t id, size_t n,
                              float *out_wo, float *out_pdf, float *out_weight)
{
    return run_spectral(ctx, { mrl::MODE_SAMPLE, wi, nullptr, u, wavelengths, n_wavelengths, id, n, nullptr, nullptr, out_wo, out_pdf, out_weight });
}
int mrl_eval_sample_spectral_batch(mrl_ctx *ctx, const float *wi, const float *wo, const float *u, const float *wavelengths, int n_wavelengths, int32_t id,
                                   size_t n, float *out_values, float *out_pdf, float *out_wo, float *out_pdf2, float *out_weight)
{
    return run_spectral(ctx, { mrl::MODE_EVAL_SAMPLE, wi, wo, u, wavelengths, n_wavelengths, id, n, out_values, out_pdf, out_wo, out_pdf2, out_weight });
}

// ---- over a wavefront queue (device pointers; mat == NULL: the material single_id) ----
int mrl_eval_spectral_queue(mrl_ctx *ctx, const float *wi, const float *wo, const float *wavelengths, int n_wavelengths, const int32_t *mat, int32_t single_id,
                            const uint32_t *queue, const uint32_t *queue_count, size_t capacity, float *out_values)
{
    return run_spectral(ctx, queue_call({ mrl::MODE_EVAL, wi, wo, nullptr, wavelengths, n_wavelengths, single_id, capacity, out_values, nullptr, nullptr, nullptr, nullptr },
                                        mat, queue, queue_count));
}
int mrl_eval_pdf_spectral_queue(mrl_ctx *ctx, const float *wi, const float *wo, const float *wavelengths, int n_wavelengths, const int32_t *mat, int32_t single_id,
                                const uint32_t *queue, const uint32_t *queue_count, size_t capacity, float *out_values, float *out_pdf)
{
    return run_spectral(ctx, queue_call({ mrl::MODE_EVAL_PDF, wi, wo, nullptr, wavelengths, n_wavelengths, single_id, capacity, out_values, out_pdf, nullptr, nullptr, nullptr },
                                        mat, queue, queue_count));
}
int mrl_sample_spectral_queue(mrl_ctx *ctx, const float *wi, const float *u, const float *wavelengths, int n_wavelengths, const int32_t *mat, int32_t single_id,
                              const uint32_t *queue, const uint32_t *queue_count, size_t capacity, float *out_wo, float *out_pdf, float *out_weight)
{
    return run_spectral(ctx, queue_call({ mrl::MODE_SAMPLE, wi, nullptr, u, wavelengths, n_wavelengths, single_id, capacity, nullptr, nullptr, out_wo, out_pdf, out_weight },
                                        mat, queue, queue_count));
}
int mrl_eval_sample_spectral_queue(mrl_ctx *ctx, const float *wi, const float *wo, const float *u, const float *wavelengths, int n_wavelengths, const int32_t *mat,
                                   int32_t single_id, const uint32_t *queue, const uint32_t *queue_count, size_t capacity,
                                   float *out_values, float *out_pdf, float *out_wo, float *out_pdf2, float *out_weight)
{
    return run_spectral(ctx, queue_call({ mrl::MODE_EVAL_SAMPLE, wi, wo, u, wavelengths, n_wavelengths, single_id, capacity, out_values, out_pdf, out_wo, out_pdf2, out_weight },
                                        mat, queue, queue_count));
}

// ---- whole arrays with a material id per unit (host or device pointers) ----
int mrl_eval_spectral_batch_mat(mrl_ctx *ctx, const float *wi, const float *wo, const float *wavelengths, int n_wavelengths, const int32_t *mat, size_t n,
                                float *out_values)
{
    return run_spectral(ctx, mat_call({ mrl::MODE_EVAL, wi, wo, nullptr, wavelengths, n_wavelengths, -1, n, out_values, nullptr, nullptr, nullptr, nullptr }, mat));
}
int mrl_eval_pdf_spectral_batch_mat(mrl_ctx *ctx, const float *wi, const float *wo, const float *wavelengths, int n_wavelengths, const int32_t *mat, size_t n,
                                    float *out_values, float *out_pdf)
{
    return run_spectral(ctx, mat_call({ mrl::MODE_EVAL_PDF, wi, wo, nullptr, wavelengths, n_wavelengths, -1, n, out_values, out_pdf, nullptr, nullptr, nullptr }, mat));
}
int mrl_sample_spectral_batch_mat(mrl_ctx *ctx, const float *wi, const float *u, const float *wavelengths, int n_wavelengths, const int32_t *mat, size_t n,
                                  float *out_wo, float *out_pdf, float *out_weight)
{
    return run_spectral(ctx, mat_call({ mrl::MODE_SAMPLE, wi, nullptr, u, wavelengths, n_wavelengths, -1, n, nullptr, nullptr, out_wo, out_pdf, out_weight }, mat));
}
int mrl_eval_sample_spectral_batch_mat(mrl_ctx *ctx, const float *wi, const float *wo, const float *u, const float *wavelengths, int n_wavelengths, const int32_t *mat,
                                       size_t n, float *out_values, float *out_pdf, float *out_wo, float *out_pdf2, float *out_weight)
{
    return run_spectral(ctx, mat_call({ mrl::MODE_EVAL_SAMPLE, wi, wo, u, wavelengths, n_wavelengths, -1, n, out_values, out_pdf, out_wo, out_pdf2, out_weight }, mat));
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
