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

namespace mrl {

namespace {

// Launch shape from the compiled register count.  The per-lane math is f64 (two registers a value) on top of the cell's 24 floats:
// no scratch, no LDS, and under the bound below 136 to 142 VGPRs.  Registers are allocated in granules of 8 out of 512 per SIMD lane, so
// <= 168 means three waves per SIMD: three 256-thread blocks (four waves, one per SIMD) per compute unit — and that is the grid, so
// every block of the persistent grid is resident at once and the loop strides over the rest.  (Bounded to 128 registers for a fourth
// wave the kernels spill 28 B per lane.)
constexpr int kTableDirBlock = 256;
constexpr int kTableDirBlocksPerCu = 3;

struct TableDirGradOut { const float *g; float *grad_wi, *grad_wo; };

template <bool PER_LANE, bool INDEXED, int LAYOUT>
__global__ __launch_bounds__(kTableDirBlock, kTableDirBlocksPerCu) void k_table_grad_dir(BatchArgs a, TableDirGradOut o)
{
#pragma clang fp contract(off)
    const size_t stride = (size_t)gridDim.x * kTableDirBlock;
    const size_t n_items = item_count<INDEXED>(a);
    for (size_t j = (size_t)blockIdx.x * kTableDirBlock + threadIdx.x; j < n_items; j += stride) {
        const size_t i = INDEXED ? (size_t)a.idx[j] : j;
        bool known = true;
        // the fields the per-lane function reads; a.single is the safe material of a launch with ids
        MaterialDev m = a.single;
        if constexpr (PER_LANE) {
            const int id = a.mat[i];
            const bool in_range = id >= 0 && id < a.n_materials;
            const MaterialDev &s = a.materials[in_range ? id : 0];
            const int kind = s.kind;
            known = in_range && (kind == KIND_MERL || kind == KIND_TABLE);
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

template <bool PER_LANE, bool INDEXED>
void launch_layout(int layout, dim3 grid, dim3 block, hipStream_t stream, const BatchArgs &a, const TableDirGradOut &o)
{
    if (layout == LAYOUT_BRICK) hipLaunchKernelGGL((k_table_grad_dir<PER_LANE, INDEXED, LAYOUT_BRICK>), grid, block, 0, stream, a, o);
    else hipLaunchKernelGGL((k_table_grad_dir<PER_LANE, INDEXED, LAYOUT_ROWS>), grid, block, 0, stream, a, o);
}

// a.mat: a material id per unit; a.idx: a queue (a.n: its capacity); a.single: the material of a launch without ids, the safe one with
hipError_t launch_table_grad_dir(const BatchArgs &a, const TableDirGradOut &o, int layout, int compute_units, hipStream_t stream)
{
    const dim3 grid(grid_blocks(a.n, kTableDirBlock, (size_t)std::max(compute_units, 1) * kTableDirBlocksPerCu)), block(kTableDirBlock);
    if (a.mat) {
        if (a.idx) launch_layout<true, true>(layout, grid, block, stream, a, o);
        else launch_layout<true, false>(layout, grid, block, stream, a, o);
    } else {
        if (a.idx) launch_layout<false, true>(layout, grid, block, stream, a, o);
        else launch_layout<false, false>(layout, grid, block, stream, a, o);
    }
    return hipGetLastError();
}

} // namespace

} // namespace mrl

using namespace mrlabi;

namespace {

// both calls; queued: over queue[0 .. min(*queue_count, n)), n its capacity
int table_grad_dir_call(mrl_ctx *ctx, const float *wi, const float *wo, const float *grad_rgb, const int32_t *mat, int32_t single_id, size_t n,
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
        const int kind = ctx->materials[(size_t)single_id].dev.kind;
        if (kind != mrl::KIND_MERL && kind != mrl::KIND_TABLE)
            return fail(ctx, MRL_ERR_MATERIAL, "the table direction gradient is defined for RGB table materials (MERL / customized_measurement)");
    }
    if (ctx->opts.negative == mrl::NEGATIVE_RENORMALISE)
        return fail(ctx, MRL_ERR_INVALID, "MRL_OPT_NEGATIVE = renormalise: the direction gradient of the renormalising blend is not offered");
    if (queued && n > ((size_t)1 << 32)) return fail(ctx, MRL_ERR_INVALID, "queue capacity exceeds 2^32 (indices are uint32)");
    MRL_HIP(ctx, hipSetDevice(ctx->device));
    const int kind = queued ? common_kind({ queue, queue_count }, streams) : common_kind({}, streams);
    if (queued && kind != 1) return fail(ctx, MRL_ERR_POINTER_MIX, "queue calls take device pointers only");
    if (kind < 0) return fail(ctx, MRL_ERR_POINTER_MIX, "host and device pointers mixed in one call");

    mrl::BatchArgs a;
    std::memset(&a, 0, sizeof a);
    a.materials = ctx->d_materials;
    a.n_materials = (int)ctx->materials.size();
    a.safe = tombstone_dev(ctx);
    a.single = mat ? a.safe : ctx->materials[(size_t)single_id].dev;
    a.opts = ctx->opts;
    a.idx = queue; a.idx_count = queue_count;
    const int layout = ctx->table_layout;
    if (kind == 1) {
        a.wi = wi; a.wo = wo; a.mat = mat; a.n = n;
        MRL_HIP(ctx, mrl::launch_table_grad_dir(a, { grad_rgb, grad_wi, grad_wo }, layout, ctx->compute_units, ctx->stream));
        return MRL_OK;
    }
    return run_host_staged(ctx, streams, n, 0, [&](char *const *addr, size_t m) -> int {
        a.wi = (const float *)addr[0]; a.wo = (const float *)addr[1]; a.n = m;
        a.mat = at_mat >= 0 ? (const int32_t *)addr[at_mat] : nullptr;
        const mrl::TableDirGradOut o = { (const float *)addr[2], at_wi >= 0 ? (float *)addr[at_wi] : nullptr, at_wo >= 0 ? (float *)addr[at_wo] : nullptr };
        MRL_HIP(ctx, mrl::launch_table_grad_dir(a, o, layout, ctx->compute_units, ctx->stream));
        return MRL_OK;
    });
}

} // namespace

extern "C" {

int mrl_table_grad_dir_batch(mrl_ctx *ctx, const float *wi, const float *wo, const float *grad_rgb, const int32_t *mat, int32_t single_id, size_t n,
                             float *grad_wi, float *grad_wo)
{
    return table_grad_dir_call(ctx, wi, wo, grad_rgb, mat, single_id, n, false, nullptr, nullptr, grad_wi, grad_wo);
}

int mrl_table_grad_dir_queue(mrl_ctx *ctx, const float *wi, const float *wo, const float *grad_rgb, const int32_t *mat, int32_t single_id,
                             const uint32_t *queue, const uint32_t *queue_count, size_t capacity, float *grad_wi, float *grad_wo)
{
    return table_grad_dir_call(ctx, wi, wo, grad_rgb, mat, single_id, capacity, true, queue, queue_count, grad_wi, grad_wo);
}

} // extern "C"
