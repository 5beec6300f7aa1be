// merl_ggx_dir_grad.hip — the gradient of eval in the directions on GGX conductors (include/merl_hip_diff.h, mrl_ggx_grad_dir_batch and
// mrl_ggx_grad_dir_queue): grad_wi[u] = sum_c g_uc d eval_c / d wi_u and the same in wo_u, a per-unit OUTPUT — the
// third shape after the table adjoint (scattered) and the parameter gradient (reduced): nothing is summed over units, so there is
// no workspace, no second kernel and nothing to order.
//   k_ggx_grad_dir<PER_LANE, INDEXED>   persistent grid, grid-stride loop, one lane = one unit: fast::ggx_eval_dir_grad of
//                                       merl_ggx_fast.hpp; reads 36 B per unit (+ 4 with material ids, + 4 with a queue), writes 12 or 24
//   PER_LANE: the material comes from mat[i], its constants are built per lane from the context's material array (an id that names
//   no live GGX material: a constant material, outputs forced to zero); otherwise they are wave-uniform.  INDEXED: walks a queue.
// A unit's bits depend on its inputs and its material alone: all four instantiations inline the same contraction-free function.
#include "merl_ctx.hpp"
#include "../../include/merl_hip_diff.h"
#include "merl_ggx_fast.hpp"

namespace mrl {

namespace {

// Launch shape from the compiled register count.  The per-lane math is f64 throughout (two registers a value) and the kernels come
// out at 86 (material per lane), 92 (single material, queue) and 96 (single material, whole arrays) VGPRs under the bound below, no
// scratch, no LDS; left alone the compiler takes 116 for the last one, one wave per SIMD fewer.  Registers are allocated in granules
// of 8 out of 512 per SIMD lane, so <= 96 means five waves per SIMD: five 256-thread blocks (four waves, one per SIMD) per compute
// unit — and that is the grid, so every block of the persistent grid is resident at once and the loop strides over the rest.
constexpr int kDirBlock = 256;
constexpr int kDirBlocksPerCu = 5;

struct DirGradOut { const float *g; float *grad_wi, *grad_wo; };

template <bool PER_LANE, bool INDEXED>
__global__ __launch_bounds__(kDirBlock, kDirBlocksPerCu) void k_ggx_grad_dir(BatchArgs a, DirGradOut o)
{
#pragma clang fp contract(off)
    const size_t stride = (size_t)gridDim.x * kDirBlock;
    const size_t n_items = item_count<INDEXED>(a);
    for (size_t j = (size_t)blockIdx.x * kDirBlock + threadIdx.x; j < n_items; j += stride) {
        const size_t i = INDEXED ? (size_t)a.idx[j] : j;
        bool known = true;
        double alpha = a.single.alpha, eta[3] = { a.single.eta[0], a.single.eta[1], a.single.eta[2] },
               k[3] = { a.single.k[0], a.single.k[1], a.single.k[2] };
        if constexpr (PER_LANE) {
            const int id = a.mat[i];
            const bool in_range = id >= 0 && id < a.n_materials;
            const MaterialDev &m = a.materials[in_range ? id : 0];
            known = in_range && m.kind == KIND_GGX;
            // a.single is the constant material of a launch with ids
            alpha = known ? m.alpha : alpha;
#pragma unroll
            for (int c = 0; c < 3; ++c) { eta[c] = known ? m.eta[c] : eta[c]; k[c] = known ? m.k[c] : k[c]; }
        }
        const fast::GgxConsts g = fast::ggx_consts_exact(alpha, eta, k);
        float wix, wiy, wiz, wox, woy, woz, g32[3];
        load3s<true>(a.wi, i, wix, wiy, wiz);
        load3s<true>(a.wo, i, wox, woy, woz);
        load3s<true>(o.g, i, g32[0], g32[1], g32[2]);
        const fast::GgxDirGrad r = fast::ggx_eval_dir_grad(g, wix, wiy, wiz, wox, woy, woz, g32);
        if (o.grad_wi) {
            const float v[3] = { known ? r.wi[0] : 0.0f, known ? r.wi[1] : 0.0f, known ? r.wi[2] : 0.0f };
            store3s<true>(o.grad_wi, i, v);
        }
        if (o.grad_wo) {
            const float v[3] = { known ? r.wo[0] : 0.0f, known ? r.wo[1] : 0.0f, known ? r.wo[2] : 0.0f };
            store3s<true>(o.grad_wo, i, v);
        }
    }
}

// a.mat: a material id per unit; a.idx: a queue (a.n: its capacity); a.single: the material of a launch without ids
hipError_t launch_ggx_grad_dir(const BatchArgs &a, const DirGradOut &o, int compute_units, hipStream_t stream)
{
    const dim3 grid(grid_blocks(a.n, kDirBlock, (size_t)std::max(compute_units, 1) * kDirBlocksPerCu)), block(kDirBlock);
    if (a.mat) {
        if (a.idx) hipLaunchKernelGGL((k_ggx_grad_dir<true, true>), grid, block, 0, stream, a, o);
        else hipLaunchKernelGGL((k_ggx_grad_dir<true, false>), grid, block, 0, stream, a, o);
    } else {
        if (a.idx) hipLaunchKernelGGL((k_ggx_grad_dir<false, true>), grid, block, 0, stream, a, o);
        else hipLaunchKernelGGL((k_ggx_grad_dir<false, false>), grid, block, 0, stream, a, o);
    }
    return hipGetLastError();
}

} // namespace

} // namespace mrl

using namespace mrlabi;

namespace {

// what a unit with an id that names no live GGX material evaluates (its outputs are forced to zero)
mrl::MaterialDev constant_ggx()
{
    mrl::MaterialDev m;
    std::memset(&m, 0, sizeof m);
    m.kind = mrl::KIND_GGX;
    m.alpha = 0.5;
    for (int c = 0; c < 3; ++c) { m.eta[c] = 1.5; m.k[c] = 1.0; }
    return m;
}

// both calls; queued: over queue[0 .. min(*queue_count, n)), n its capacity
int grad_dir_call(mrl_ctx *ctx, const float *wi, const float *wo, const float *grad_rgb, const int32_t *mat, int32_t single_id, size_t n,
                  bool queued, const uint32_t *queue, const uint32_t *queue_count, float *grad_wi, float *grad_wo)
{
    if (!ctx) return MRL_ERR_INVALID;
    MRL_GUARD(ctx);
    if (n == 0) return MRL_OK;
    if (queued && (!queue || !queue_count)) return fail(ctx, MRL_ERR_INVALID, "null array argument");
    StreamList streams = { { (void *)wi, 12, false, "wi" }, { (void *)wo, 12, false, "wo" }, { (void *)grad_rgb, 12, false, "grad_rgb" } };
    if (first_null(streams)) return fail(ctx, MRL_ERR_INVALID, "null array argument");
    if (!grad_wi && !grad_wo) return fail(ctx, MRL_ERR_INVALID, "grad_wi and grad_wo are both null");
    int at_mat = -1, at_wi = -1, at_wo = -1;
    if (mat) { at_mat = (int)streams.size(); streams.push_back({ (void *)mat, 4, false, "mat" }); }
    if (grad_wi) { at_wi = (int)streams.size(); streams.push_back({ grad_wi, 12, true, "grad_wi" }); }
    if (grad_wo) { at_wo = (int)streams.size(); streams.push_back({ grad_wo, 12, true, "grad_wo" }); }
    if (ctx->materials.empty()) return fail(ctx, MRL_ERR_MATERIAL, "no material loaded");
    if (!mat) {
        if (single_id < 0 || (size_t)single_id >= ctx->materials.size() || ctx->materials[(size_t)single_id].released)
            return fail(ctx, MRL_ERR_MATERIAL, "unknown material id");
        if (ctx->materials[(size_t)single_id].dev.kind != mrl::KIND_GGX)
            return fail(ctx, MRL_ERR_MATERIAL, "the direction gradient is defined for GGX conductor materials");
    }
    if (queued && n > ((size_t)1 << 32)) return fail(ctx, MRL_ERR_INVALID, "queue capacity exceeds 2^32 (indices are uint32)");
    MRL_HIP(ctx, hipSetDevice(ctx->device));
    const int kind = queued ? common_kind({ queue, queue_count }, streams) : common_kind({}, streams);
    if (queued && kind != 1) return fail(ctx, MRL_ERR_POINTER_MIX, "queue calls take device pointers only");
    if (kind < 0) return fail(ctx, MRL_ERR_POINTER_MIX, "host and device pointers mixed in one call");

    mrl::BatchArgs a;
    std::memset(&a, 0, sizeof a);
    a.materials = ctx->d_materials;
    a.n_materials = (int)ctx->materials.size();
    a.single = mat ? constant_ggx() : ctx->materials[(size_t)single_id].dev;
    a.idx = queue; a.idx_count = queue_count;
    if (kind == 1) {
        a.wi = wi; a.wo = wo; a.mat = mat; a.n = n;
        MRL_HIP(ctx, mrl::launch_ggx_grad_dir(a, { grad_rgb, grad_wi, grad_wo }, ctx->compute_units, ctx->stream));
        return MRL_OK;
    }
    return run_host_staged(ctx, streams, n, 0, [&](char *const *addr, size_t m) -> int {
        a.wi = (const float *)addr[0]; a.wo = (const float *)addr[1]; a.n = m;
        a.mat = at_mat >= 0 ? (const int32_t *)addr[at_mat] : nullptr;
        const mrl::DirGradOut o = { (const float *)addr[2], at_wi >= 0 ? (float *)addr[at_wi] : nullptr, at_wo >= 0 ? (float *)addr[at_wo] : nullptr };
        MRL_HIP(ctx, mrl::launch_ggx_grad_dir(a, o, ctx->compute_units, ctx->stream));
        return MRL_OK;
    });
}

} // namespace

extern "C" {

int mrl_ggx_grad_dir_batch(mrl_ctx *ctx, const float *wi, const float *wo, const float *grad_rgb, const int32_t *mat, int32_t single_id, size_t n,
                           float *grad_wi, float *grad_wo)
{
    return grad_dir_call(ctx, wi, wo, grad_rgb, mat, single_id, n, false, nullptr, nullptr, grad_wi, grad_wo);
}

int mrl_ggx_grad_dir_queue(mrl_ctx *ctx, const float *wi, const float *wo, const float *grad_rgb, const int32_t *mat, int32_t single_id,
                           const uint32_t *queue, const uint32_t *queue_count, size_t capacity, float *grad_wi, float *grad_wo)
{
    return grad_dir_call(ctx, wi, wo, grad_rgb, mat, single_id, capacity, true, queue, queue_count, grad_wi, grad_wo);
}

} // extern "C"
