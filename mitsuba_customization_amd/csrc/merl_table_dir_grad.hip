// merl_table_dir_grad.hip — the gradient of eval in the directions on RGB table materials (include/merl_hip_diff_table.h,
// mrl_table_grad_dir_batch and mrl_table_grad_dir_queue): grad_wi[u] = sum_c g_uc d eval_c / d wi_u and the same in wo_u,
// a per-unit output like the GGX direction gradient's (merl_ggx_dir_grad.hip): no workspace, no second kernel, nothing to order.
//   k_table_grad_dir<PER_LANE, INDEXED, LAYOUT>   persistent grid, grid-stride loop, one lane = one unit: fast::table_eval_dir_grad of
//                                                 merl_table_dir_grad.hpp.  Reads 36 B of streams per unit (+ 4 with material ids, + 4 with
//                                                 a queue) and one neighbourhood — six 16-B loads of one 128-B brick, or eight row texels,
//                                                 all issued before any use —, writes 12 or 24 B.
//   PER_LANE: the material comes from mat[i] (an id that names no live RGB table: BatchArgs::safe, outputs forced to zero; the code
//   stays branch-free); otherwise it is wave-uniform.  INDEXED: walks a queue.  The lookup mode and the node convention are
//   wave-uniform selects inside the per-lane function.
// A unit's bits depend on its inputs, its material and the options alone: every instantiation inlines the same contraction-free
// function, and the two layouts hand it the same 24 floats.
#include "merl_ctx.hpp"
#include "../../include/merl_hip_diff_table.h"
#include "merl_table_dir_grad.hpp"
#include "merl_dir_grad.hpp"

namespace mrl {

namespace {

// Launch shape from the compiled register count.  The per-lane math is f64 (two registers a value) on top of the cell's 24 floats:
// no scratch, no LDS, and under the bound below 136 to 142 VGPRs.  Registers are allocated in granules of 8 out of 512 per SIMD lane, so
// <= 168 means three waves per SIMD: three 256-thread blocks (four waves, one per SIMD) per compute unit — and that is the grid, so
// every block of the persistent grid is resident at once and the loop strides over the rest.  (Bounded to 128 registers for a fourth
// wave the kernels spill 28 B per lane.)
constexpr int kTableDirBlock = 256;
constexpr int kTableDirBlocksPerCu = 3;

template <bool PER_LANE, bool INDEXED, int LAYOUT>
__global__ __launch_bounds__(kTableDirBlock, kTableDirBlocksPerCu) void k_table_grad_dir(BatchArgs a, DirGradOut o)
{
#pragma clang fp contract(off)
    dir_grad_loop<kTableDirBlock, INDEXED>(a, o, [&](size_t i, float (&r_wi)[3], float (&r_wo)[3]) {
        bool known = true;
        // the fields the per-lane function reads; a.single is the safe material of a launch with ids
        MaterialDev m = a.single;
        if constexpr (PER_LANE) {
            const LaneMaterial lane = lane_material(a, i);
            const MaterialDev &s = lane.m;
            const int kind = s.kind;
            known = lane.in_range && (kind == KIND_MERL || kind == KIND_TABLE);
            m.n_th = known ? s.n_th : m.n_th; m.n_td = known ? s.n_td : m.n_td; m.n_pd = known ? s.n_pd : m.n_pd;
            m.row_td = known ? s.row_td : m.row_td; m.row_th = known ? s.row_th : m.row_th;
            m.texels = known ? s.texels : m.texels;
            m.param = known ? s.param : m.param;
        }
        float wix, wiy, wiz, wox, woy, woz, g32[3];
        load3s<true>(a.wi, i, wix, wiy, wiz);
        load3s<true>(a.wo, i, wox, woy, woz);
        load3s<true>(o.g, i, g32[0], g32[1], g32[2]);
        const fast::TableDirGrad r = fast::table_eval_dir_grad<LAYOUT>(m, a.opts, wix, wiy, wiz, wox, woy, woz, g32);
#pragma unroll
        for (int c = 0; c < 3; ++c) { r_wi[c] = r.wi[c]; r_wo[c] = r.wo[c]; }
        return known;
    });
}

// a.mat: a material id per unit; a.idx: a queue (a.n: its capacity); a.single: the material of a launch without ids, the safe one with
hipError_t launch_table_grad_dir(const BatchArgs &a, const DirGradOut &o, int layout, int compute_units, hipStream_t stream)
{
    const dim3 grid(grid_blocks(a.n, kTableDirBlock, (size_t)std::max(compute_units, 1) * kTableDirBlocksPerCu)), block(kTableDirBlock);
    with_flags([&](auto per_lane, auto indexed, auto brick) {
        hipLaunchKernelGGL((k_table_grad_dir<per_lane, indexed, brick ? LAYOUT_BRICK : LAYOUT_ROWS>), grid, block, 0, stream, a, o);
    }, a.mat != nullptr, a.idx != nullptr, layout == LAYOUT_BRICK);
    return hipGetLastError();
}

} // namespace

} // namespace mrl

using namespace mrlabi;

namespace {

// both calls: the checks, the staging of host arrays and the launch are grad_dir_call's (merl_calls.hip)
int table_grad_dir(mrl_ctx *ctx, const DirGradCall &c)
{
    if (!ctx) return MRL_ERR_INVALID;
    return grad_dir_call(ctx, c, { 12, "grad_rgb",
        [](const MaterialHost &m) { return m.dev.kind == mrl::KIND_MERL || m.dev.kind == mrl::KIND_TABLE; },
        "the table direction gradient is defined for RGB table materials (MERL / customized_measurement)", true,
        [&] { return tombstone_dev(ctx); },
        [&](const mrl::BatchArgs &a, const float *g, float *grad_wi, float *grad_wo, void *const *) {
            return mrl::launch_table_grad_dir(a, { g, grad_wi, grad_wo }, ctx->table_layout, ctx->compute_units, ctx->stream);
        } });
}

} // namespace

extern "C" {

int mrl_table_grad_dir_batch(mrl_ctx *ctx, const float *wi, const float *wo, const float *grad_rgb, const int32_t *mat, int32_t single_id, size_t n,
                             float *grad_wi, float *grad_wo)
{
    return table_grad_dir(ctx, { wi, wo, grad_rgb, mat, single_id, n, false, nullptr, nullptr, grad_wi, grad_wo });
}

int mrl_table_grad_dir_queue(mrl_ctx *ctx, const float *wi, const float *wo, const float *grad_rgb, const int32_t *mat, int32_t single_id,
                             const uint32_t *queue, const uint32_t *queue_count, size_t capacity, float *grad_wi, float *grad_wo)
{
    return table_grad_dir(ctx, { wi, wo, grad_rgb, mat, single_id, capacity, true, queue, queue_count, grad_wi, grad_wo });
}

} // extern "C"
