// merl_grad_scatter.hip — the host side the four adjoints of eval share (merl_table_grad.hip, merl_table_grad_nch.hip,
// merl_rgl_values_grad.hip, merl_rgl_spectral_values_grad.hip; DESIGN.md "What the adjoints share"): grad_scatter_call, and the clear of their workspace.
//   k_grad_clear    zeros a call's gradient bricks (a kernel, not a memset: see there)
#include "merl_ctx.hpp"

namespace mrl {

namespace {

constexpr int kClearBlock = 256;

// The clear of the workspace, as a kernel and not a memset: a captured queue call is replayed many times, and a memset node of this
// size came back from its second replay on with denormal garbage in place of zeros (measured on ROCm 7.2: every replay after the
// first, the reached texels right and the unreached ones ~1e-308); plain 16-B stores replay like any kernel
__global__ __launch_bounds__(kClearBlock) void k_grad_clear(double2 *bricks, size_t pairs)
{
    const size_t stride = (size_t)gridDim.x * kClearBlock;
    for (size_t at = (size_t)blockIdx.x * kClearBlock + threadIdx.x; at < pairs; at += stride) bricks[at] = make_double2(0.0, 0.0);
}

} // namespace

} // namespace mrl

namespace mrlabi {

hipError_t launch_grad_clear(double *bricks, size_t bytes, int compute_units, hipStream_t stream)
{
    const size_t pairs = bytes / sizeof(double2);
    if (pairs == 0) return hipSuccess;
    hipLaunchKernelGGL(mrl::k_grad_clear, dim3(mrl::grid_blocks(pairs, mrl::kClearBlock, (size_t)compute_units * 8)), dim3(mrl::kClearBlock), 0,
                       stream, (double2 *)bricks, pairs);
    return hipGetLastError();
}

// mrl_table_grad_batch* / mrl_table_grad_queue* / mrl_rgl_values_grad_* / mrl_rgl_spectral_values_grad_* (GradScatterFamily); queued: over queue[0 .. min(*queue_count, n))
int grad_scatter_call(mrl_ctx *ctx, const GradScatterCall &c, const GradScatterFamily &f)
{
    MRL_GUARD(ctx);
    if (c.n == 0) return MRL_OK;
    StreamList streams = { { (void *)c.wi, 12, false, "wi" }, { (void *)c.wo, 12, false, "wo" }, { (void *)c.g, c.g_bytes, false, c.g_name } };
    if (first_null(streams) || !c.out || !c.target_ids || (c.queued && (!c.queue || !c.queue_count)))
        return fail(ctx, MRL_ERR_INVALID, "null array argument");
    if (c.mat) streams.push_back({ (void *)c.mat, 4, false, "mat" });
    if (c.extra) streams.push_back({ (void *)c.extra, c.extra_bytes, false, c.extra_name });
    if (c.n_targets < 1 || c.n_targets > c.max_targets) return fail(ctx, MRL_ERR_INVALID, "n_targets must be 1.." + std::to_string(c.max_targets));
    for (int k = 0; k < c.n_targets; ++k) {
        const int rc = f.check_target(c.target_ids[k]);
        if (rc != MRL_OK) return rc;
        for (int j = 0; j < k; ++j)
            if (c.target_ids[j] == c.target_ids[k]) return fail(ctx, MRL_ERR_INVALID, "a material is listed twice among the targets");
    }
    GradScatterLayout lay{};
    int rc = f.layout(lay);
    if (rc != MRL_OK) return rc;
    if (f.refuses_renormalise && ctx->opts.negative == mrl::NEGATIVE_RENORMALISE)
        return fail(ctx, MRL_ERR_INVALID, "MRL_OPT_NEGATIVE = renormalise makes eval non-linear in the table: no adjoint");
    if (c.queued && c.n > ((size_t)1 << 32)) return fail(ctx, MRL_ERR_INVALID, "queue capacity exceeds 2^32 (indices are uint32)");
    MRL_HIP(ctx, hipSetDevice(ctx->device));
    const int kind = c.queued ? common_kind({ c.out, c.queue, c.queue_count }, streams) : common_kind({ c.out }, streams);
    if (c.queued && kind != 1) return fail(ctx, MRL_ERR_POINTER_MIX, "queue calls take device pointers only");
    if (kind < 0) return fail(ctx, MRL_ERR_POINTER_MIX, "host and device pointers mixed in one call");
    if (lay.nothing_to_add) return MRL_OK;

    // the workspace is cleared once and folded once, target by target, into the targets' own slices and nothing else
    double *bricks = nullptr;
    if (lay.brick_bytes > 0) {
        DeviceBuf &buf = ctx->buf[mrl_ctx::BUF_GRAD_BRICKS];         // grown on demand, reused
        rc = buf.reserve(ctx, lay.brick_bytes);
        if (rc != MRL_OK) return rc;
        bricks = (double *)buf.p;
        MRL_HIP(ctx, launch_grad_clear(bricks, lay.brick_bytes, ctx->compute_units, ctx->stream));
    }
    if (kind == 1) {
        char *addr[5];
        for (size_t k = 0; k < streams.size(); ++k) addr[k] = (char *)streams[k].ptr;
        MRL_HIP(ctx, f.launch(addr, c.n, bricks, c.out));
        if (bricks) MRL_HIP(ctx, f.fold(bricks, c.out));
        return MRL_OK;
    }
    // host arrays: the inputs are staged chunk by chunk, the sums gathered in a device array and added to the caller's on the host
    double *d_out = nullptr;
    MRL_ALLOC(ctx, hipMalloc((void **)&d_out, lay.out_doubles * sizeof(double)));
    auto run = [&]() -> int {
        MRL_HIP(ctx, hipMemsetAsync(d_out, 0, lay.out_doubles * sizeof(double), ctx->stream));
        const int rs = run_host_staged(ctx, streams, c.n, c.cap_bytes, [&](char *const *addr, size_t m) -> int {
            MRL_HIP(ctx, f.launch(addr, m, bricks, d_out));
            return MRL_OK;
        });
        if (rs != MRL_OK) return rs;
        if (bricks) MRL_HIP(ctx, f.fold(bricks, d_out));
        std::vector<double> sums;
        try { sums.resize(lay.out_doubles); } catch (const std::bad_alloc &) { return fail(ctx, MRL_ERR_OOM, "gradient buffer"); }
        MRL_HIP(ctx, hipMemcpyAsync(sums.data(), d_out, lay.out_doubles * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
        MRL_HIP(ctx, hipStreamSynchronize(ctx->stream));
        for (size_t t = 0; t < lay.out_doubles; ++t)
            if (sums[t] != 0.0) c.out[t] += sums[t];                 // an entry nothing reached keeps its bits
        return MRL_OK;
    };
    rc = run();
    if (rc != MRL_OK) (void)hipStreamSynchronize(ctx->stream);
    (void)hipFree(d_out);
    return rc;
}

} // namespace mrlabi
