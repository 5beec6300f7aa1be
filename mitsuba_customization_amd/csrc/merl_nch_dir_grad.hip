// merl_nch_dir_grad.hip — the gradient of eval in the directions on n-channel table materials (include/merl_hip_diff_nch.h,
// mrl_table_grad_dir_batch_nch and mrl_table_grad_dir_queue_nch): grad_wi[u] = sum_c g_uc d eval_c / d wi_u over the
// n_channels channels of the call and the same in wo_u, a per-unit output like the RGB twin's (merl_table_dir_grad.hip): no
// workspace, no second kernel, nothing to order.
//   k_table_grad_dir_nch<PER_LANE, INDEXED, CPAD>   persistent grid, grid-stride loop, one lane = one unit: fast::nch_eval_dir_grad of
//                                                   merl_nch_dir_grad.hpp.  Reads 24 B of directions and 4 n_ch B of g per unit (+ 4
//                                                   with material ids, + 4 with a queue) and the cell's bricks — 32 B, 64 B, or
//                                                   ceil(n_ch / 4) contiguous 128-B lines, a group's loads issued before any use and
//                                                   the next group's before the current one is contracted —, writes 12 or 24 B.
//   PER_LANE: the material comes from mat[i].  An id that names no live n-channel table of exactly n_ch channels reads a.single
//   instead — the FIRST LIVE TABLE OF THAT WIDTH in the context, chosen by the host: the lane's cell is clamped into that table's own
//   dims, so what it reads is one cell of a table of the width the loop walks, inside a live allocation whatever its size — and its
//   outputs are forced to zero; the code stays branch-free.  (The RGB kernels' tombstone cell is 256 B and the material array's size
//   depends on the material count: neither is promised to hold the 1,024 B of a 32-channel cell.)  A context that holds no table of
//   that width has nothing to read: the launch then writes zeros under a wave-uniform flag.  INDEXED: walks a queue.
// A unit's bits depend on its inputs, its material and the options alone: every instantiation inlines the same contraction-free
// function; g is read by per-lane dword loads (its rows are 4-byte aligned only).
#include "merl_ctx.hpp"
#include "../../include/merl_hip_diff_nch.h"
#include "merl_nch_dir_grad.hpp"

namespace mrl {

namespace {

// Launch shape from the compiled register count, as merl_table_dir_grad.hip takes it.  The per-lane math is f64 on top of the texels
// in registers: no scratch, no LDS.  Registers are allocated in granules of 8 out of 512 per SIMD lane.
//   1 and 2 channels (one brick of 32 / 64 B): 128 to 138 VGPRs, <= 168: three waves per SIMD, three 256-thread blocks (four waves,
//   one per SIMD) per compute unit, the shape of k_table_grad_dir;
//   4 .. 32 channels: two groups' lines are live (one being contracted, one in flight: 64 + 8 registers): bounded to 168 the
//   kernels spill 12 to 36 B per lane, so they are bounded to 256: two waves per SIMD, two blocks per compute unit, each lane with up
//   to sixteen 16-B loads in flight.
// That is the grid, so every block of the persistent grid is resident at once and the loop strides over the rest.  The compiled
// counts per instantiation are in DESIGN.md §5k; tests/test_nch_dir_grad_cpu.py reads them off the ISA.
constexpr int kNchDirBlock = 256;
constexpr int kNchDirBlocksPerCu = 3;
constexpr int kNchDirBlocksPerCuWide = 2;
constexpr int nch_dir_blocks_per_cu(int cpad) { return cpad == 4 ? kNchDirBlocksPerCuWide : kNchDirBlocksPerCu; }

struct NchDirGradOut {
    const float *g;              // [n][n_ch]
    float *grad_wi, *grad_wo;
    int n_ch;
    int no_table;                // a launch with ids in a context without a live table of n_ch channels: every unit gets zeros
};

template <bool PER_LANE, bool INDEXED, int CPAD>
__global__ __launch_bounds__(kNchDirBlock, nch_dir_blocks_per_cu(CPAD)) void k_table_grad_dir_nch(BatchArgs a, NchDirGradOut o)
{
#pragma clang fp contract(off)
    const size_t stride = (size_t)gridDim.x * kNchDirBlock;
    const size_t n_items = item_count<INDEXED>(a);
    const int n_ch = o.n_ch;
    const float zero[3] = { 0.0f, 0.0f, 0.0f };
    for (size_t j = (size_t)blockIdx.x * kNchDirBlock + threadIdx.x; j < n_items; j += stride) {
        const size_t i = INDEXED ? (size_t)a.idx[j] : j;
        if (PER_LANE && o.no_table) {                            // wave-uniform
            if (o.grad_wi) store3s<true>(o.grad_wi, i, zero);
            if (o.grad_wo) store3s<true>(o.grad_wo, i, zero);
            continue;
        }
        bool known = true;
        // the fields the per-lane function reads; a.single is the safe table of a launch with ids
        MaterialDev m = a.single;
        if constexpr (PER_LANE) {
            const int id = a.mat[i];
            const bool in_range = id >= 0 && id < a.n_materials;
            const MaterialDev &s = a.materials[in_range ? id : 0];
            known = in_range && s.kind == KIND_TABLE_NCH && s.n_ch == n_ch;
            m.n_th = known ? s.n_th : m.n_th; m.n_td = known ? s.n_td : m.n_td; m.n_pd = known ? s.n_pd : m.n_pd;
            m.texels = known ? s.texels : m.texels;
            m.param = known ? s.param : m.param;
        }
        float wix, wiy, wiz, wox, woy, woz;
        load3s<true>(a.wi, i, wix, wiy, wiz);
        load3s<true>(a.wo, i, wox, woy, woz);
        const fast::TableDirGrad r = fast::nch_eval_dir_grad<CPAD>(m, a.opts, wix, wiy, wiz, wox, woy, woz, o.g + i * (size_t)n_ch, n_ch);
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
void launch_cpad(int compute_units, hipStream_t stream, const BatchArgs &a, const NchDirGradOut &o)
{
    const int cpad = o.n_ch == 1 ? 1 : o.n_ch == 2 ? 2 : 4;
    const dim3 grid(grid_blocks(a.n, kNchDirBlock, (size_t)std::max(compute_units, 1) * nch_dir_blocks_per_cu(cpad))), block(kNchDirBlock);
    if (o.n_ch == 1) hipLaunchKernelGGL((k_table_grad_dir_nch<PER_LANE, INDEXED, 1>), grid, block, 0, stream, a, o);
    else if (o.n_ch == 2) hipLaunchKernelGGL((k_table_grad_dir_nch<PER_LANE, INDEXED, 2>), grid, block, 0, stream, a, o);
    else hipLaunchKernelGGL((k_table_grad_dir_nch<PER_LANE, INDEXED, 4>), grid, block, 0, stream, a, o);
}

// a.mat: a material id per unit; a.idx: a queue (a.n: its capacity); a.single: the material of a launch without ids, the safe one with
hipError_t launch_table_grad_dir_nch(const BatchArgs &a, const NchDirGradOut &o, int compute_units, hipStream_t stream)
{
    if (o.n_ch < 1 || o.n_ch > kMaxChannels || o.n_ch == 3) return hipErrorInvalidValue;
    if (a.mat) {
        if (a.idx) launch_cpad<true, true>(compute_units, stream, a, o);
        else launch_cpad<true, false>(compute_units, stream, a, o);
    } else {
        if (a.idx) launch_cpad<false, true>(compute_units, stream, a, o);
        else launch_cpad<false, false>(compute_units, stream, a, o);
    }
    return hipGetLastError();
}

} // namespace

} // namespace mrl

using namespace mrlabi;

namespace {

bool live_nch(const MaterialHost &m, int n_ch) { return !m.released && m.dev.kind == mrl::KIND_TABLE_NCH && m.dev.n_ch == n_ch; }

// both calls; queued: over queue[0 .. min(*queue_count, n)), n its capacity
int nch_grad_dir_call(mrl_ctx *ctx, const float *wi, const float *wo, const float *grad_values, const int32_t *mat, int32_t single_id, size_t n,
                      bool queued, const uint32_t *queue, const uint32_t *queue_count, int n_ch, float *grad_wi, float *grad_wo)
{
    MRL_GUARD(ctx);
    if (n == 0) return MRL_OK;
    if (queued && (!queue || !queue_count)) return fail(ctx, MRL_ERR_INVALID, "null array argument");
    StreamList streams = { { (void *)wi, 12, false, "wi" }, { (void *)wo, 12, false, "wo" }, { (void *)grad_values, 4 * (size_t)n_ch, false, "grad_values" } };
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
        if (!live_nch(ctx->materials[(size_t)single_id], n_ch))
            return fail(ctx, MRL_ERR_MATERIAL, "material is not an n-channel table of " + std::to_string(n_ch) + " channels");
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
    a.opts = ctx->opts;
    a.idx = queue; a.idx_count = queue_count;
    int no_table = 0;
    if (mat) {
        // what a unit with another id reads: the first live table of this width (see the head of this file)
        const auto safe = std::find_if(ctx->materials.begin(), ctx->materials.end(), [&](const MaterialHost &m) { return live_nch(m, n_ch); });
        no_table = safe == ctx->materials.end();
        a.single = no_table ? a.safe : safe->dev;
    } else {
        a.single = ctx->materials[(size_t)single_id].dev;
    }
    if (kind == 1) {
        a.wi = wi; a.wo = wo; a.mat = mat; a.n = n;
        MRL_HIP(ctx, mrl::launch_table_grad_dir_nch(a, { grad_values, grad_wi, grad_wo, n_ch, no_table }, ctx->compute_units, ctx->stream));
        return MRL_OK;
    }
    return run_host_staged(ctx, streams, n, 0, [&](char *const *addr, size_t m) -> int {
        a.wi = (const float *)addr[0]; a.wo = (const float *)addr[1]; a.n = m;
        a.mat = at_mat >= 0 ? (const int32_t *)addr[at_mat] : nullptr;
        const mrl::NchDirGradOut o = { (const float *)addr[2], at_wi >= 0 ? (float *)addr[at_wi] : nullptr, at_wo >= 0 ? (float *)addr[at_wo] : nullptr,
                                       n_ch, no_table };
        MRL_HIP(ctx, mrl::launch_table_grad_dir_nch(a, o, ctx->compute_units, ctx->stream));
        return MRL_OK;
    });
}

// the channel count first, as every *_nch call checks it (merl_calls.hip, nch_call); three channels are the RGB twin's
int checked_channels(mrl_ctx *ctx, int n_channels)
{
    if (n_channels >= 1 && n_channels <= mrl::kMaxChannels) return MRL_OK;
    MRL_GUARD(ctx);
    return fail(ctx, MRL_ERR_INVALID, "channel count must be 1.." + std::to_string(mrl::kMaxChannels));
}

} // namespace

extern "C" {

int mrl_table_grad_dir_batch_nch(mrl_ctx *ctx, const float *wi, const float *wo, const float *grad_values, const int32_t *mat, int32_t single_id,
                                 size_t n, int n_channels, float *grad_wi, float *grad_wo)
{
    if (!ctx) return MRL_ERR_INVALID;
    if (const int rc = checked_channels(ctx, n_channels)) return rc;
    if (n_channels == 3) return mrl_table_grad_dir_batch(ctx, wi, wo, grad_values, mat, single_id, n, grad_wi, grad_wo);
    return nch_grad_dir_call(ctx, wi, wo, grad_values, mat, single_id, n, false, nullptr, nullptr, n_channels, grad_wi, grad_wo);
}

int mrl_table_grad_dir_queue_nch(mrl_ctx *ctx, const float *wi, const float *wo, const float *grad_values, const int32_t *mat, int32_t single_id,
                                 const uint32_t *queue, const uint32_t *queue_count, size_t capacity, int n_channels, float *grad_wi, float *grad_wo)
{
    if (!ctx) return MRL_ERR_INVALID;
    if (const int rc = checked_channels(ctx, n_channels)) return rc;
    if (n_channels == 3) return mrl_table_grad_dir_queue(ctx, wi, wo, grad_values, mat, single_id, queue, queue_count, capacity, grad_wi, grad_wo);
    return nch_grad_dir_call(ctx, wi, wo, grad_values, mat, single_id, capacity, true, queue, queue_count, n_channels, grad_wi, grad_wo);
}

} // extern "C"
