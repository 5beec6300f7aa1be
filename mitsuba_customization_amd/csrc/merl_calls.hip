// merl_calls.hip — the batch, queue and n-channel calls of the C ABI (include/merl_hip.h): argument checks, a call's arrays as a stream
// list, the staged and the pipelined mover of the host-array path, the launches.  No CPU evaluation path exists here: every entry point ends in a gfx950
// kernel launch or an error.
#include "merl_ctx.hpp"

namespace mrlabi {

// The arrays a call of this mode touches, in slot order: f(the call's pointer field, bytes per unit, written by the kernel?, name)
template <class F>
void for_each_stream(BatchCall &c, F &&f)
{
    const bool has_eval = mrl::mode_eval(c.mode), has_pdf = mrl::mode_pdf(c.mode), has_sample = mrl::mode_sample(c.mode);
    const size_t values = 4 * (size_t)(c.n_ch > 0 ? c.n_ch : 3);
    f(c.wi, 12, false, "wi");
    if (has_eval || has_pdf) f(c.wo, 12, false, "wo");
    if (has_sample) f(c.u, 8, false, "u");
    if (c.wl) f(c.wl, values, false, "wavelengths");
    if (c.mat) f(c.mat, 4, false, "mat");
    if (has_eval) f(c.out_rgb, values, true, "values");
    if (has_pdf) f(c.out_pdf, 4, true, "pdf");
    if (has_sample) { f(c.out_wo, 12, true, "out_wo"); f(c.out_pdf2, 4, true, "pdf of out_wo"); f(c.out_weight, values, true, "weight"); }
}

StreamList streams_of(const BatchCall &c)
{
    StreamList streams;
    BatchCall t = c;
    for_each_stream(t, [&](auto *&p, size_t unit_bytes, bool out, const char *name) { streams.push_back({ (void *)p, unit_bytes, out, name }); });
    return streams;
}

BatchCall on_slot(BatchCall c, char *const *addr, size_t m)
{
    for_each_stream(c, [&](auto *&p, size_t, bool, const char *) { p = (std::remove_reference_t<decltype(p)>)*addr++; });
    c.n = m;
    return c;
}

mrl::BatchArgs batch_args(const mrl_ctx *ctx, const BatchCall &c)
{
    mrl::BatchArgs a;
    std::memset(&a, 0, sizeof a);
    a.wi = c.wi; a.wo = c.wo; a.u = c.u; a.mat = c.mat; a.n = c.n;
    a.out_rgb = c.out_rgb; a.out_pdf = c.out_pdf; a.out_wo = c.out_wo; a.out_pdf2 = c.out_pdf2; a.out_weight = c.out_weight;
    a.materials = ctx->d_materials;
    a.n_materials = (int)ctx->materials.size();
    a.opts = ctx->opts;
    return a;
}

// kernel arguments of a call whose pointers are all device-accessible
struct DeviceCall {
    mrl::BatchArgs args;
    bool multi, has_ggx, has_table, has_rgl;
};

DeviceCall device_call(const mrl_ctx *ctx, const BatchCall &c)
{
    DeviceCall d;
    mrl::BatchArgs &a = d.args;
    a = batch_args(ctx, c);
    a.safe = tombstone_dev(ctx);
    a.block_map = ctx->block_map;
    d.multi = c.mat != nullptr;
    if (!d.multi) a.single = ctx->materials[(size_t)c.single_id].dev;
    d.has_ggx = d.has_table = d.has_rgl = false;
    a.any_standard = 0;
    for (const auto &m : ctx->materials) {
        if (m.released) continue;
        d.has_rgl = d.has_rgl || m.dev.kind == mrl::KIND_RGL;
        if (d.multi && m.dev.kind != mrl::KIND_GGX && m.dev.param != mrl::PARAM_HALF_DIFF) a.any_standard = 1;
        d.has_ggx = d.has_ggx || m.dev.kind == mrl::KIND_GGX;
        d.has_table = d.has_table || m.dev.kind == mrl::KIND_MERL || m.dev.kind == mrl::KIND_TABLE ||
                      (c.mode == mrl::MODE_PDF && m.dev.kind == mrl::KIND_TABLE_NCH);       // pdf serves n-channel tables too
    }
    if (!d.has_ggx && !d.has_table) d.has_table = true;        // only tombstones left: the table path renders them as zeros
    if (!d.multi && a.single.kind != mrl::KIND_GGX && a.single.param != mrl::PARAM_HALF_DIFF) a.any_standard = 1;
    return d;
}

// null-pointer and material checks shared by the whole-array and the queue entry points
int check_call(mrl_ctx *ctx, const BatchCall &c, const StreamList &streams)
{
    if (first_null(streams)) return fail(ctx, MRL_ERR_INVALID, "null array argument");
    if (ctx->materials.empty()) return fail(ctx, MRL_ERR_MATERIAL, "no material loaded");
    if (!c.mat && (c.single_id < 0 || (size_t)c.single_id >= ctx->materials.size() || ctx->materials[(size_t)c.single_id].released))
        return fail(ctx, MRL_ERR_MATERIAL, "unknown material id");
    if (!c.mat) {
        const mrl::MaterialDev &d = ctx->materials[(size_t)c.single_id].dev;
        if (d.kind == mrl::KIND_RGL) {
            if (c.n_ch > 0) return fail(ctx, MRL_ERR_MATERIAL, "an RGL material has three channels: use the RGB entry points");
            return MRL_OK;
        }
        if (d.kind == mrl::KIND_RGL_SPECTRAL) {                // the pdf is wavelength-free: the RGB pdf call serves it
            if (c.mode == mrl::MODE_PDF && c.n_ch == 0) return MRL_OK;
            return fail(ctx, MRL_ERR_MATERIAL, "a spectral RGL material: use the mrl_*_spectral_batch entry points");
        }
        if (c.n_ch == 0 && c.mode != mrl::MODE_PDF && !mrl::kind_is_rgb_path(d.kind))               // pdf is channel-free
            return fail(ctx, MRL_ERR_MATERIAL, "material has " + std::to_string(d.n_ch) + " channels: use the *_nch entry points");
        if (c.n_ch > 0 && c.mode != mrl::MODE_PDF && (d.kind != mrl::KIND_TABLE_NCH || d.n_ch != c.n_ch))
            return fail(ctx, MRL_ERR_MATERIAL, "material does not have " + std::to_string(c.n_ch) + " channels");
    }
    return MRL_OK;
}

// The launches of one call on device pointers, in order; queue != nullptr: over a caller's queue of unit indices (c.n = its capacity)
int launch_device(mrl_ctx *ctx, const BatchCall &c, const uint32_t *queue = nullptr, const uint32_t *queue_count = nullptr)
{
    DeviceCall d = device_call(ctx, c);
    mrl::BatchArgs &a = d.args;
    a.idx = queue; a.idx_count = queue_count;
    const int cus = ctx->compute_units;
    if (!d.multi && (a.single.kind == mrl::KIND_RGL || a.single.kind == mrl::KIND_RGL_SPECTRAL)) {     // adaptive-parameterisation material: its own kernel (spectral: pdf only)
        MRL_HIP(ctx, mrl::launch_rgl(c.mode, a, &ctx->materials[(size_t)c.single_id].rgl, ctx->rgl_search, cus, ctx->stream));
        return MRL_OK;
    }
    if (c.n_ch > 0 && c.mode != mrl::MODE_PDF) {                          // n-channel tables: their own kernels (pdf is channel-free)
        MRL_HIP(ctx, mrl::launch_batch_nch(c.mode, a, c.n_ch, cus, ctx->stream));
        return MRL_OK;
    }
    const mrl::BatchRoute route = { ctx->kernel_variant, ctx->table_layout, d.has_ggx, d.has_table, true };
    if (mrl::route_partitions(c.mode, a, route)) {             // count / scan / partition (no atomics), then each kind's dense queue
        uint32_t segments = 0, seg_len = 0;
        mrl::partition_geometry(c.n, cus, &segments, &seg_len);
        if (segments > kMaxSegments) return fail(ctx, MRL_ERR_INVALID, "partition geometry");
        DeviceBuf &queues = ctx->buf[mrl_ctx::BUF_QUEUES];
        int rc = queues.reserve(ctx, (2 * c.n + 4 * kMaxSegments + 2) * sizeof(uint32_t));
        if (rc != MRL_OK) return rc;
        uint32_t *q_table = (uint32_t *)queues.p, *q_ggx = q_table + c.n, *work = q_ggx + c.n;
        MRL_HIP(ctx, mrl::launch_partition_kinds(c.mat, c.n, ctx->d_materials, a.n_materials, q_table, q_ggx, work, segments, seg_len, ctx->stream));
        const uint32_t *totals = work + 4 * (size_t)segments;
        mrl::BatchArgs qa = a;
        qa.idx = q_table; qa.idx_count = totals;
        MRL_HIP(ctx, mrl::launch_batch(c.mode, qa, mrl::kind_queue_route(route, false), cus, ctx->stream));
        qa.idx = q_ggx; qa.idx_count = totals + 1;
        MRL_HIP(ctx, mrl::launch_batch(c.mode, qa, mrl::kind_queue_route(route, true), cus, ctx->stream));
    } else {
        MRL_HIP(ctx, mrl::launch_batch(c.mode, a, route, cus, ctx->stream));
    }
    // the context holds RGL materials: their units (zeros so far) are evaluated by a second launch on the same stream
    if (d.multi && d.has_rgl) MRL_HIP(ctx, mrl::launch_rgl(c.mode, a, nullptr, ctx->rgl_search, cus, ctx->stream));
    return MRL_OK;
}

// ---- the two movers of the chunk loop (merl_host_stage.hpp, run_chunks) ----
// Staged: one slot in the context's stage buffer; the copies ride the stream around the launch, one synchronise per chunk.
struct StagedMover {
    mrl_ctx *ctx;
    static constexpr size_t depth = 0;
    int prepare(size_t slot_bytes) { return ctx->buf[mrl_ctx::BUF_STAGE].reserve(ctx, slot_bytes); }
    char *slot(size_t) { return (char *)ctx->buf[mrl_ctx::BUF_STAGE].p; }
    int copy(const std::vector<CopySeg> &segs, hipMemcpyKind kind)
    {
        for (const CopySeg &sg : segs) {
            const hipError_t e = hipMemcpyAsync(sg.dst, sg.src, sg.bytes, kind, ctx->stream);
            if (e != hipSuccess) { (void)hipGetLastError(); return fail(ctx, MRL_ERR_HIP, std::string("staging copy of ") + sg.name + ": " + hipGetErrorString(e)); }
        }
        return MRL_OK;
    }
    int copy_in(size_t, const std::vector<CopySeg> &segs) { return copy(segs, hipMemcpyHostToDevice); }
    int launched(size_t) { return MRL_OK; }
    int copy_out(size_t, const std::vector<CopySeg> &segs)
    {
        const int rc = copy(segs, hipMemcpyDeviceToHost);
        if (rc != MRL_OK) return rc;
        MRL_HIP(ctx, hipStreamSynchronize(ctx->stream));       // the outputs are on the host, the slot is free for the next chunk
        return MRL_OK;
    }
    void drain() { (void)hipStreamSynchronize(ctx->stream); }
};

// Pipelined (see HostPipe): copy threads fill and drain two pinned slots that the kernel reads and writes over PCIe itself (zero
// copy), so that the copies of chunks k+1 / k-1 overlap the kernel of chunk k.
struct PipelinedMover {
    mrl_ctx *ctx;
    static constexpr size_t depth = 1;
    int prepare(size_t slot_bytes)
    {
        HostPipe &hp = ctx->pipe;
        if (slot_bytes > hp.slot_bytes) {
            auto release = [&]() { for (char *&p : hp.pin) { if (p) (void)hipHostFree(p); p = nullptr; } hp.slot_bytes = 0; };
            MRL_HIP(ctx, hipStreamSynchronize(ctx->stream));
            release();
            for (char *&p : hp.pin) {
                const hipError_t e = hipHostMalloc((void **)&p, slot_bytes, hipHostMallocMapped | hipHostMallocPortable);
                if (e == hipSuccess) continue;
                (void)hipGetLastError();
                release();
                return fail(ctx, MRL_ERR_OOM, std::string("pinned staging: ") + hipGetErrorString(e));
            }
            hp.slot_bytes = slot_bytes;
        }
        for (int s = 0; s < 2; ++s)
            if (!hp.done[s]) MRL_HIP(ctx, hipEventCreateWithFlags(&hp.done[s], hipEventDisableTiming));
        if (hp.threads != ctx->host_threads) {                   // the caller copies as well: n - 1 helpers
            hp.pool.stop();
            hp.pool.quit = false;
            hp.pool.start(std::max(0, ctx->host_threads - 1));
            hp.threads = ctx->host_threads;
        }
        return MRL_OK;
    }
    char *slot(size_t k) { return ctx->pipe.pin[k & 1]; }
    // slot k & 1 was last read by kernel k - 2, whose event copy_out(k - 2) waited for
    int copy_in(size_t, const std::vector<CopySeg> &segs) { ctx->pipe.pool.run(segs); return MRL_OK; }
    int launched(size_t k) { MRL_HIP(ctx, hipEventRecord(ctx->pipe.done[k & 1], ctx->stream)); return MRL_OK; }
    int copy_out(size_t k, const std::vector<CopySeg> &segs)
    {
        MRL_HIP(ctx, hipEventSynchronize(ctx->pipe.done[k & 1]));
        ctx->pipe.pool.run(segs);
        return MRL_OK;
    }
    void drain() { (void)hipStreamSynchronize(ctx->stream); }
};

int run_host_staged(mrl_ctx *ctx, const StreamList &streams, size_t n, size_t cap_bytes, const HostLaunch &launch)
{
    StagedMover mv{ ctx };
    return run_chunks(mv, streams, n, ctx->host_chunk, cap_bytes, launch);
}

int run_batch(mrl_ctx *ctx, const BatchCall &c)
{
    if (!ctx) return MRL_ERR_INVALID;
    MRL_GUARD(ctx);
    if (c.n == 0) return MRL_OK;
    const StreamList streams = streams_of(c);
    int rc = check_call(ctx, c, streams);
    if (rc != MRL_OK) return rc;
    MRL_HIP(ctx, hipSetDevice(ctx->device));

    const int kind = common_kind({}, streams);
    if (kind < 0) return fail(ctx, MRL_ERR_POINTER_MIX, "host and device pointers mixed in one call");
    if (kind == 1) return launch_device(ctx, c);

    // host pointers, chunk by chunk; returns when the outputs are on the host
    auto launch = [&](char *const *addr, size_t m) { return launch_device(ctx, on_slot(c, addr, m)); };
    if (ctx->host_threads > 0) {
        PipelinedMover mv{ ctx };
        rc = run_chunks(mv, streams, c.n, std::min(ctx->host_chunk, (size_t)1 << 20), 0, launch);
        if (rc != MRL_ERR_OOM) return rc;                     // no pinned memory to be had: fall back to the staged path
        (void)hipGetLastError();
    }
    return run_host_staged(ctx, streams, c.n, 0, launch);
}

// mrl_*_queue: a caller-built queue of unit indices with a device-side length
int run_queue(mrl_ctx *ctx, const BatchCall &c, const uint32_t *queue, const uint32_t *queue_count)
{
    if (!ctx) return MRL_ERR_INVALID;
    MRL_GUARD(ctx);
    if (c.n == 0) return MRL_OK;
    if (!queue || !queue_count) return fail(ctx, MRL_ERR_INVALID, "null array argument");
    const StreamList streams = streams_of(c);
    int rc = check_call(ctx, c, streams);
    if (rc != MRL_OK) return rc;
    if (c.n > ((size_t)1 << 32)) return fail(ctx, MRL_ERR_INVALID, "queue capacity exceeds 2^32 (indices are uint32)");
    MRL_HIP(ctx, hipSetDevice(ctx->device));
    if (common_kind({ queue, queue_count }, streams) != 1) return fail(ctx, MRL_ERR_POINTER_MIX, "queue calls take device pointers only");
    return launch_device(ctx, c, queue, queue_count);
}

// mrl_*_grad_dir_batch / _queue of every family (DirGradFamily); queued: over queue[0 .. min(*queue_count, n)), n its capacity
int grad_dir_call(mrl_ctx *ctx, const DirGradCall &c, const DirGradFamily &f)
{
    MRL_GUARD(ctx);
    if (c.n == 0) return MRL_OK;
    if (c.queued && (!c.queue || !c.queue_count)) return fail(ctx, MRL_ERR_INVALID, "null array argument");
    StreamList streams = { { (void *)c.wi, 12, false, "wi" }, { (void *)c.wo, f.second_bytes, false, f.second_name }, { (void *)c.g, f.g_bytes, false, f.g_name } };
    for (const DirGradExtra &x : c.extra) if (x.required) streams.push_back({ x.ptr, x.unit_bytes, x.out, x.name });
    if (first_null(streams)) return fail(ctx, MRL_ERR_INVALID, "null array argument");
    streams.resize(3);
    bool any_out = c.grad_wi || c.grad_wo;
    for (const DirGradExtra &x : c.extra) any_out = any_out || (x.out && x.ptr);
    if (!any_out) return fail(ctx, MRL_ERR_INVALID, c.extra.empty() ? "grad_wi and grad_wo are both null" : "every output is null");
    int at_mat = -1, at_wi = -1, at_wo = -1;
    if (c.mat) { at_mat = (int)streams.size(); streams.push_back({ (void *)c.mat, 4, false, "mat" }); }
    if (c.grad_wi) { at_wi = (int)streams.size(); streams.push_back({ c.grad_wi, 12, true, "grad_wi" }); }
    if (c.grad_wo) { at_wo = (int)streams.size(); streams.push_back({ c.grad_wo, 12, true, "grad_wo" }); }
    // the extra streams the call goes with: listed, so that they take part in the pointer kind and in the chunks of host arrays
    std::vector<int> at_extra(c.extra.size(), -1);
    std::vector<void *> extra(c.extra.size(), nullptr);
    for (size_t k = 0; k < c.extra.size(); ++k) {
        const DirGradExtra &x = c.extra[k];
        extra[k] = x.ptr;
        if (x.ptr) { at_extra[k] = (int)streams.size(); streams.push_back({ x.ptr, x.unit_bytes, x.out, x.name }); }
    }
    if (ctx->materials.empty()) return fail(ctx, MRL_ERR_MATERIAL, "no material loaded");
    if (!c.mat) {
        if (c.single_id < 0 || (size_t)c.single_id >= ctx->materials.size() || ctx->materials[(size_t)c.single_id].released)
            return fail(ctx, MRL_ERR_MATERIAL, "unknown material id");
        if (!f.evaluates(ctx->materials[(size_t)c.single_id])) return fail(ctx, MRL_ERR_MATERIAL, f.not_evaluated);
    }
    if (f.refuses_renormalise && ctx->opts.negative == mrl::NEGATIVE_RENORMALISE)
        return fail(ctx, MRL_ERR_INVALID, "MRL_OPT_NEGATIVE = renormalise: the direction gradient of the renormalising blend is not offered");
    if (c.queued && c.n > ((size_t)1 << 32)) return fail(ctx, MRL_ERR_INVALID, "queue capacity exceeds 2^32 (indices are uint32)");
    MRL_HIP(ctx, hipSetDevice(ctx->device));
    const int kind = c.queued ? common_kind({ c.queue, c.queue_count }, streams) : common_kind({}, streams);
    if (c.queued && kind != 1) return fail(ctx, MRL_ERR_POINTER_MIX, "queue calls take device pointers only");
    if (kind < 0) return fail(ctx, MRL_ERR_POINTER_MIX, "host and device pointers mixed in one call");

    mrl::BatchArgs a;
    std::memset(&a, 0, sizeof a);
    a.materials = ctx->d_materials;
    a.n_materials = (int)ctx->materials.size();
    a.safe = tombstone_dev(ctx);
    a.single = c.mat ? f.single_with_ids() : ctx->materials[(size_t)c.single_id].dev;
    a.opts = ctx->opts;
    a.idx = c.queue; a.idx_count = c.queue_count;
    if (kind == 1) {
        a.wi = c.wi; a.wo = c.wo; a.mat = c.mat; a.n = c.n;
        MRL_HIP(ctx, f.launch(a, c.g, c.grad_wi, c.grad_wo, extra.empty() ? nullptr : extra.data()));
        return MRL_OK;
    }
    return run_host_staged(ctx, streams, c.n, f.cap_bytes, [&](char *const *addr, size_t m) -> int {
        a.wi = (const float *)addr[0]; a.wo = (const float *)addr[1]; a.n = m;
        a.mat = at_mat >= 0 ? (const int32_t *)addr[at_mat] : nullptr;
        for (size_t k = 0; k < extra.size(); ++k) extra[k] = at_extra[k] >= 0 ? addr[at_extra[k]] : nullptr;
        MRL_HIP(ctx, f.launch(a, (const float *)addr[2], at_wi >= 0 ? (float *)addr[at_wi] : nullptr, at_wo >= 0 ? (float *)addr[at_wo] : nullptr,
                              extra.empty() ? nullptr : extra.data()));
        return MRL_OK;
    });
}

} // namespace mrlabi
using namespace mrlabi;

extern "C" {

int mrl_eval_batch(mrl_ctx *ctx, const float *wi, const float *wo, const int32_t *mat, int32_t single_id, size_t n, float *out_rgb)
{
    return run_batch(ctx, { mrl::MODE_EVAL, wi, wo, nullptr, mat, single_id, n, out_rgb, nullptr, nullptr, nullptr, nullptr });
}

int mrl_pdf_batch(mrl_ctx *ctx, const float *wi, const float *wo, const int32_t *mat, int32_t single_id, size_t n, float *out_pdf)
{
    return run_batch(ctx, { mrl::MODE_PDF, wi, wo, nullptr, mat, single_id, n, nullptr, out_pdf, nullptr, nullptr, nullptr });
}

int mrl_sample_batch(mrl_ctx *ctx, const float *wi, const float *u, const int32_t *mat, int32_t single_id, size_t n,
                     float *out_wo, float *out_pdf, float *out_weight)
{
    return run_batch(ctx, { mrl::MODE_SAMPLE, wi, nullptr, u, mat, single_id, n, nullptr, nullptr, out_wo, out_pdf, out_weight });
}

int mrl_eval_sample_batch(mrl_ctx *ctx, const float *wi, const float *wo, const float *u, const int32_t *mat, int32_t single_id,
                          size_t n, float *out_rgb, float *out_pdf, float *out_wo, float *out_pdf2, float *out_weight)
{
    return run_batch(ctx, { mrl::MODE_EVAL_SAMPLE, wi, wo, u, mat, single_id, n, out_rgb, out_pdf, out_wo, out_pdf2, out_weight });
}

int mrl_eval_pdf_batch(mrl_ctx *ctx, const float *wi, const float *wo, const int32_t *mat, int32_t single_id,
                       size_t n, float *out_rgb, float *out_pdf)
{
    return run_batch(ctx, { mrl::MODE_EVAL_PDF, wi, wo, nullptr, mat, single_id, n, out_rgb, out_pdf, nullptr, nullptr, nullptr });
}

int mrl_partition_by_material(mrl_ctx *ctx, const int32_t *mat, size_t n, uint32_t *queue_out, uint32_t *offsets_out, uint32_t *counts_out)
{
    if (!ctx) return MRL_ERR_INVALID;
    MRL_GUARD(ctx);
    if (!offsets_out || !counts_out || (n > 0 && (!mat || !queue_out))) return fail(ctx, MRL_ERR_INVALID, "null array argument");
    if (n > ((size_t)1 << 32)) return fail(ctx, MRL_ERR_INVALID, "more than 2^32 slots (queue entries are uint32)");
    const int K = (int)ctx->materials.size();
    if (K == 0) return fail(ctx, MRL_ERR_MATERIAL, "no material loaded");
    if (K > mrl::kMaxPartitionMaterials) return fail(ctx, MRL_ERR_INVALID, "too many materials for the partition kernel");
    MRL_HIP(ctx, hipSetDevice(ctx->device));
    if (common_kind({ mat, queue_out, offsets_out, counts_out }) != 1) return fail(ctx, MRL_ERR_POINTER_MIX, "partition takes device pointers only");
    if (n == 0) {                                     // nothing to partition: every group is empty
        MRL_HIP(ctx, hipMemsetAsync(offsets_out, 0, ((size_t)K + 1) * sizeof(uint32_t), ctx->stream));
        MRL_HIP(ctx, hipMemsetAsync(counts_out, 0, (size_t)K * sizeof(uint32_t), ctx->stream));
        return MRL_OK;
    }
    uint32_t chunks = 0, chunk_len = 0;
    mrl::material_partition_geometry(n, ctx->compute_units, &chunks, &chunk_len);
    DeviceBuf &work = ctx->buf[mrl_ctx::BUF_PART_WORK];
    const int rc = work.reserve(ctx, ((size_t)chunks * K + K) * sizeof(uint32_t));
    if (rc != MRL_OK) return rc;
    MRL_HIP(ctx, mrl::launch_partition_materials(mat, n, K, queue_out, offsets_out, counts_out, (uint32_t *)work.p, chunks, chunk_len,
                                                 ctx->compute_units, ctx->stream));
    return MRL_OK;
}

int mrl_eval_pdf_queue(mrl_ctx *ctx, const float *wi, const float *wo, const int32_t *mat, int32_t single_id,
                       const uint32_t *queue, const uint32_t *queue_count, size_t capacity, float *out_rgb, float *out_pdf)
{
    return run_queue(ctx, { mrl::MODE_EVAL_PDF, wi, wo, nullptr, mat, single_id, capacity, out_rgb, out_pdf, nullptr, nullptr, nullptr }, queue, queue_count);
}

int mrl_eval_queue(mrl_ctx *ctx, const float *wi, const float *wo, const int32_t *mat, int32_t single_id,
                   const uint32_t *queue, const uint32_t *queue_count, size_t capacity, float *out_rgb)
{
    return run_queue(ctx, { mrl::MODE_EVAL, wi, wo, nullptr, mat, single_id, capacity, out_rgb, nullptr, nullptr, nullptr, nullptr }, queue, queue_count);
}

int mrl_pdf_queue(mrl_ctx *ctx, const float *wi, const float *wo, const int32_t *mat, int32_t single_id,
                  const uint32_t *queue, const uint32_t *queue_count, size_t capacity, float *out_pdf)
{
    return run_queue(ctx, { mrl::MODE_PDF, wi, wo, nullptr, mat, single_id, capacity, nullptr, out_pdf, nullptr, nullptr, nullptr }, queue, queue_count);
}

int mrl_sample_queue(mrl_ctx *ctx, const float *wi, const float *u, const int32_t *mat, int32_t single_id,
                     const uint32_t *queue, const uint32_t *queue_count, size_t capacity,
                     float *out_wo, float *out_pdf, float *out_weight)
{
    return run_queue(ctx, { mrl::MODE_SAMPLE, wi, nullptr, u, mat, single_id, capacity, nullptr, nullptr, out_wo, out_pdf, out_weight }, queue, queue_count);
}

int mrl_eval_sample_queue(mrl_ctx *ctx, const float *wi, const float *wo, const float *u,
                          const int32_t *mat, int32_t single_id,
                          const uint32_t *queue, const uint32_t *queue_count, size_t capacity,
                          float *out_rgb, float *out_pdf, float *out_wo, float *out_pdf2, float *out_weight)
{
    return run_queue(ctx, { mrl::MODE_EVAL_SAMPLE, wi, wo, u, mat, single_id, capacity, out_rgb, out_pdf, out_wo, out_pdf2, out_weight }, queue, queue_count);
}

size_t mrl_batch_route(int mode, int variant, int layout, int lookup, int negative, int any_standard, int material, int queued,
                       int has_ggx, int has_table, size_t n, mrl_route_launch *out, size_t max_out)
{
    if (mode < mrl::MODE_EVAL || mode > mrl::MODE_EVAL_PDF) return 0;
    static const int32_t ids = 0;
    static const uint32_t queue = 0;
    mrl::BatchArgs a;
    std::memset(&a, 0, sizeof a);
    a.n = n; a.any_standard = any_standard; a.opts.lookup = lookup; a.opts.negative = negative;
    a.single.kind = material == MRL_ROUTE_ONE_GGX ? mrl::KIND_GGX : mrl::KIND_MERL;
    if (material == MRL_ROUTE_IDS) a.mat = &ids;                // (the route reads which pointers are set, never what they point to)
    if (queued) a.idx = a.idx_count = &queue;
    const mrl::BatchRoute route = { variant, layout, has_ggx != 0, has_table != 0, true };
    size_t count = 0;
    auto emit = [&](const std::string &kernel, int block, int blocks_per_cu, bool whole_xcds) {
        if (out && count < max_out) {
            mrl_route_launch &l = out[count];
            std::snprintf(l.kernel, sizeof l.kernel, "%s", kernel.c_str());
            l.block = block; l.blocks_per_cu = blocks_per_cu; l.whole_xcds = whole_xcds;
        }
        ++count;
    };
    auto emit_route = [&](const mrl::BatchRoute &r) {
        const mrl::KernelChoice k = mrl::route_batch(mode, a, r);
        emit(mrl::kernel_name(k), k.block, k.blocks_per_cu, k.whole_xcds);
    };
    if (mrl::route_partitions(mode, a, route)) {                // launch_partition_kinds, then launch_device's two queue launches
        emit("k_count_kinds", 256, 8, false); emit("k_scan_segments", 256, 0, false); emit("k_partition_kinds", 256, 8, false);
        a.idx = a.idx_count = &queue;
        emit_route(mrl::kind_queue_route(route, false));
        emit_route(mrl::kind_queue_route(route, true));
    } else {
        emit_route(route);
    }
    return count;
}

size_t mrl_rgl_route(int mode, int spectral, int ids, int queued, int search, size_t n, int n_phi, int n_theta, int nx, int ny, int n_wl,
                     size_t lds_limit, mrl_route_launch *out, size_t max_out)
{
    const mrl::RglRoute route = mrl::route_rgl(mode, spectral != 0, ids != 0, queued != 0, search, n, { n_phi, n_theta, nx, ny, n_wl }, lds_limit);
    for (size_t l = 0; out && l < (size_t)route.count && l < max_out; ++l) {
        const mrl::RglChoice &k = route.launch[l];
        std::snprintf(out[l].kernel, sizeof out[l].kernel, "%s", mrl::kernel_name(k).c_str());
        out[l].block = k.block; out[l].blocks_per_cu = k.blocks_per_cu; out[l].whole_xcds = 0;
    }
    return (size_t)route.count;
}

int mrl_generate_pairs(mrl_ctx *ctx, uint64_t seed, uint64_t first_index, size_t n, float *wi, float *wo, float *u)
{
    if (!ctx) return MRL_ERR_INVALID;
    MRL_GUARD(ctx);
    if (!wi || !wo || !u) return fail(ctx, MRL_ERR_INVALID, "null argument");
    MRL_HIP(ctx, hipSetDevice(ctx->device));
    if (common_kind({ wi, wo, u }) != 1) return fail(ctx, MRL_ERR_INVALID, "generator needs device pointers");
    MRL_HIP(ctx, mrl::launch_generate_pairs(seed, first_index, n, wi, wo, u, ctx->compute_units, ctx->stream));
    return MRL_OK;
}

int mrl_generate_materials(mrl_ctx *ctx, uint64_t seed, uint64_t first_index, size_t n, int n_materials, int32_t *mat)
{
    if (!ctx) return MRL_ERR_INVALID;
    MRL_GUARD(ctx);
    if (!mat || n_materials < 1) return fail(ctx, MRL_ERR_INVALID, "bad argument");
    MRL_HIP(ctx, hipSetDevice(ctx->device));
    if (pointer_kind(mat) != 1) return fail(ctx, MRL_ERR_INVALID, "generator needs device pointers");
    MRL_HIP(ctx, mrl::launch_generate_materials(seed, first_index, n, n_materials, mat, ctx->compute_units, ctx->stream));
    return MRL_OK;
}

static int nch_call(mrl_ctx *ctx, BatchCall c, int n_channels, bool queued = false, const uint32_t *queue = nullptr, const uint32_t *queue_count = nullptr)
{
    if (!ctx) return MRL_ERR_INVALID;
    if (n_channels < 1 || n_channels > mrl::kMaxChannels) return fail(ctx, MRL_ERR_INVALID, "channel count must be 1.." + std::to_string(mrl::kMaxChannels));
    c.n_ch = n_channels == 3 ? 0 : n_channels;           // three channels: the RGB path, RGB materials
    return queued ? run_queue(ctx, c, queue, queue_count) : run_batch(ctx, c);
}

int mrl_eval_queue_nch(mrl_ctx *ctx, const float *wi, const float *wo, const int32_t *mat, int32_t single_id, const uint32_t *queue,
                       const uint32_t *queue_count, size_t capacity, int n_channels, float *out_values)
{
    return nch_call(ctx, { mrl::MODE_EVAL, wi, wo, nullptr, mat, single_id, capacity, out_values, nullptr, nullptr, nullptr, nullptr }, n_channels, true, queue, queue_count);
}

int mrl_sample_queue_nch(mrl_ctx *ctx, const float *wi, const float *u, const int32_t *mat, int32_t single_id, const uint32_t *queue,
                         const uint32_t *queue_count, size_t capacity, int n_channels, float *out_wo, float *out_pdf, float *out_weight)
{
    return nch_call(ctx, { mrl::MODE_SAMPLE, wi, nullptr, u, mat, single_id, capacity, nullptr, nullptr, out_wo, out_pdf, out_weight }, n_channels, true, queue, queue_count);
}

int mrl_eval_pdf_queue_nch(mrl_ctx *ctx, const float *wi, const float *wo, const int32_t *mat, int32_t single_id, const uint32_t *queue,
                           const uint32_t *queue_count, size_t capacity, int n_channels, float *out_values, float *out_pdf)
{
    return nch_call(ctx, { mrl::MODE_EVAL_PDF, wi, wo, nullptr, mat, single_id, capacity, out_values, out_pdf, nullptr, nullptr, nullptr }, n_channels, true, queue, queue_count);
}

int mrl_eval_sample_queue_nch(mrl_ctx *ctx, const float *wi, const float *wo, const float *u, const int32_t *mat, int32_t single_id,
                              const uint32_t *queue, const uint32_t *queue_count, size_t capacity, int n_channels,
                              float *out_values, float *out_pdf, float *out_wo, float *out_pdf2, float *out_weight)
{
    return nch_call(ctx, { mrl::MODE_EVAL_SAMPLE, wi, wo, u, mat, single_id, capacity, out_values, out_pdf, out_wo, out_pdf2, out_weight }, n_channels, true, queue, queue_count);
}

int mrl_eval_batch_nch(mrl_ctx *ctx, const float *wi, const float *wo, const int32_t *mat, int32_t single_id, size_t n, int n_channels,
                       float *out_values)
{
    return nch_call(ctx, { mrl::MODE_EVAL, wi, wo, nullptr, mat, single_id, n, out_values, nullptr, nullptr, nullptr, nullptr }, n_channels);
}

int mrl_sample_batch_nch(mrl_ctx *ctx, const float *wi, const float *u, const int32_t *mat, int32_t single_id, size_t n, int n_channels,
                         float *out_wo, float *out_pdf, float *out_weight)
{
    return nch_call(ctx, { mrl::MODE_SAMPLE, wi, nullptr, u, mat, single_id, n, nullptr, nullptr, out_wo, out_pdf, out_weight }, n_channels);
}

int mrl_eval_pdf_batch_nch(mrl_ctx *ctx, const float *wi, const float *wo, const int32_t *mat, int32_t single_id, size_t n, int n_channels,
                           float *out_values, float *out_pdf)
{
    return nch_call(ctx, { mrl::MODE_EVAL_PDF, wi, wo, nullptr, mat, single_id, n, out_values, out_pdf, nullptr, nullptr, nullptr }, n_channels);
}

int mrl_eval_sample_batch_nch(mrl_ctx *ctx, const float *wi, const float *wo, const float *u, const int32_t *mat, int32_t single_id, size_t n,
                              int n_channels, float *out_values, float *out_pdf, float *out_wo, float *out_pdf2, float *out_weight)
{
    return nch_call(ctx, { mrl::MODE_EVAL_SAMPLE, wi, wo, u, mat, single_id, n, out_values, out_pdf, out_wo, out_pdf2, out_weight }, n_channels);
}

} // extern "C"
