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
#include "merl_dir_grad.hpp"

namespace mrl {

namespace {

// Launch shape from the compiled register count.  The per-lane math is f64 throughout (two registers a value) and the kernels come
// out at 86 (material per lane), 92 (single material, queue) and 96 (single material, whole arrays) VGPRs under the bound below, no
// scratch, no LDS; left alone the compiler takes 116 for the last one, one wave per SIMD fewer.  Registers are allocated in granules
// of 8 out of 512 per SIMD lane, so <= 96 means five waves per SIMD: five 256-thread blocks (four waves, one per SIMD) per compute
// unit — and that is the grid, so every block of the persistent grid is resident at once and the loop strides over the rest.
constexpr int kDirBlock = 256;
constexpr int kDirBlocksPerCu = 5;

template <bool PER_LANE, bool INDEXED>
__global__ __launch_bounds__(kDirBlock, kDirBlocksPerCu) void k_ggx_grad_dir(BatchArgs a, DirGradOut o)
{
#pragma clang fp contract(off)
    dir_grad_loop<kDirBlock, INDEXED>(a, o, [&](size_t i, float (&r_wi)[3], float (&r_wo)[3]) {
        bool known = true;
        double alpha = a.single.alpha, eta[3] = { a.single.eta[0], a.single.eta[1], a.single.eta[2] },
               k[3] = { a.single.k[0], a.single.k[1], a.single.k[2] };
        if constexpr (PER_LANE) {
            const LaneMaterial lane = lane_material(a, i);
            const MaterialDev &m = lane.m;
            known = lane.in_range && m.kind == KIND_GGX;
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
#pragma unroll
        for (int c = 0; c < 3; ++c) { r_wi[c] = r.wi[c]; r_wo[c] = r.wo[c]; }
        return known;
    });
}

// a.mat: a material id per unit; a.idx: a queue (a.n: its capacity); a.single: the material of a launch without ids
hipError_t launch_ggx_grad_dir(const BatchArgs &a, const DirGradOut &o, int compute_units, hipStream_t stream)
{
    const dim3 grid(grid_blocks(a.n, kDirBlock, (size_t)std::max(compute_units, 1) * kDirBlocksPerCu)), block(kDirBlock);
    with_flags([&](auto per_lane, auto indexed) { hipLaunchKernelGGL((k_ggx_grad_dir<per_lane, indexed>), grid, block, 0, stream, a, o); },
               a.mat != nullptr, a.idx != nullptr);
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

// both calls: the checks, the staging of host arrays and the launch are grad_dir_call's (merl_calls.hip)
int ggx_grad_dir(mrl_ctx *ctx, const DirGradCall &c)
{
    if (!ctx) return MRL_ERR_INVALID;
    return grad_dir_call(ctx, c, { 12, "grad_rgb",
        [](const MaterialHost &m) { return m.dev.kind == mrl::KIND_GGX; }, "the direction gradient is defined for GGX conductor materials", false,
        constant_ggx,
        [&](const mrl::BatchArgs &a, const float *g, float *grad_wi, float *grad_wo, void *const *) {
            return mrl::launch_ggx_grad_dir(a, { g, grad_wi, grad_wo }, ctx->compute_units, ctx->stream);
        } });
}

} // namespace

extern "C" {

int mrl_ggx_grad_dir_batch(mrl_ctx *ctx, const float *wi, const float *wo, const float *grad_rgb, const int32_t *mat, int32_t single_id, size_t n,
                           float *grad_wi, float *grad_wo)
{
    return ggx_grad_dir(ctx, { wi, wo, grad_rgb, mat, single_id, n, false, nullptr, nullptr, grad_wi, grad_wo });
}

int mrl_ggx_grad_dir_queue(mrl_ctx *ctx, const float *wi, const float *wo, const float *grad_rgb, const int32_t *mat, int32_t single_id,
                           const uint32_t *queue, const uint32_t *queue_count, size_t capacity, float *grad_wi, float *grad_wo)
{
    return ggx_grad_dir(ctx, { wi, wo, grad_rgb, mat, single_id, capacity, true, queue, queue_count, grad_wi, grad_wo });
}

} // extern "C"
