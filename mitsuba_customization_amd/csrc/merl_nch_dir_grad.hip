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
#include "merl_dir_grad.hpp"

namespace mrl {

namespace {

// Launch shape from the compiled register count, as merl_table_dir_grad.hip takes it.  The per-lane math is f64 on top of the texels
// in registers: no scratch, no LDS.  Registers are allocated in granules of 8 out of 512 per SIMD lane.
//   1 and 2 channels (one brick of 32 / 64 B): 126 to 134 VGPRs, <= 168: three waves per SIMD, three 256-thread blocks (four waves,
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

// no_table: a launch with ids in a context without a live table of n_ch channels: every unit gets zeros
template <bool PER_LANE, bool INDEXED, int CPAD>
__global__ __launch_bounds__(kNchDirBlock, nch_dir_blocks_per_cu(CPAD)) void k_table_grad_dir_nch(BatchArgs a, DirGradOut o, int n_ch, int no_table)
{
#pragma clang fp contract(off)
    dir_grad_loop<kNchDirBlock, INDEXED>(a, o, [&](size_t i, float (&r_wi)[3], float (&r_wo)[3]) {
        fast::TableDirGrad r = {};
        bool known = !(PER_LANE && no_table);                    // wave-uniform; no table: nothing is read, the loop stores zeros
        if (known) {
            // the fields the per-lane function reads; a.single is the safe table of a launch with ids
            MaterialDev m = a.single;
            if constexpr (PER_LANE) {
                const LaneMaterial lane = lane_material(a, i);
                const MaterialDev &s = lane.m;
                known = lane.in_range && s.kind == KIND_TABLE_NCH && s.n_ch == n_ch;
                m.n_th = known ? s.n_th : m.n_th; m.n_td = known ? s.n_td : m.n_td; m.n_pd = known ? s.n_pd : m.n_pd;
                m.texels = known ? s.texels : m.texels;
                m.param = known ? s.param : m.param;
            }
            float wix, wiy, wiz, wox, woy, woz;
            load3s<true>(a.wi, i, wix, wiy, wiz);
            load3s<true>(a.wo, i, wox, woy, woz);
            r = fast::nch_eval_dir_grad<CPAD>(m, a.opts, wix, wiy, wiz, wox, woy, woz, o.g + i * (size_t)n_ch, n_ch);
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) { r_wi[c] = r.wi[c]; r_wo[c] = r.wo[c]; }
        return known;
    });
}

// a.mat: a material id per unit; a.idx: a queue (a.n: its capacity); a.single: the material of a launch without ids, the safe one with;
// o.g: [n][n_ch]
hipError_t launch_table_grad_dir_nch(const BatchArgs &a, const DirGradOut &o, int n_ch, int no_table, int compute_units, hipStream_t stream)
{
    if (n_ch < 1 || n_ch > kMaxChannels || n_ch == 3) return hipErrorInvalidValue;
    const int cpad = n_ch == 1 ? 1 : n_ch == 2 ? 2 : 4;
    const dim3 grid(grid_blocks(a.n, kNchDirBlock, (size_t)std::max(compute_units, 1) * nch_dir_blocks_per_cu(cpad))), block(kNchDirBlock);
    with_flags([&](auto per_lane, auto indexed) {
        constexpr bool P = per_lane, I = indexed;
        if (cpad == 1) hipLaunchKernelGGL((k_table_grad_dir_nch<P, I, 1>), grid, block, 0, stream, a, o, n_ch, no_table);
        else if (cpad == 2) hipLaunchKernelGGL((k_table_grad_dir_nch<P, I, 2>), grid, block, 0, stream, a, o, n_ch, no_table);
        else hipLaunchKernelGGL((k_table_grad_dir_nch<P, I, 4>), grid, block, 0, stream, a, o, n_ch, no_table);
    }, a.mat != nullptr, a.idx != nullptr);
    return hipGetLastError();
}

} // namespace

} // namespace mrl

using namespace mrlabi;

namespace {

bool live_nch(const MaterialHost &m, int n_ch) { return !m.released && m.dev.kind == mrl::KIND_TABLE_NCH && m.dev.n_ch == n_ch; }

// both calls: the checks, the staging of host arrays and the launch are grad_dir_call's (merl_calls.hip)
int nch_grad_dir(mrl_ctx *ctx, const DirGradCall &c, int n_ch)
{
    int no_table = 0;
    return grad_dir_call(ctx, c, { 4 * (size_t)n_ch, "grad_values",
        [&](const MaterialHost &m) { return live_nch(m, n_ch); }, "material is not an n-channel table of " + std::to_string(n_ch) + " channels", true,
        [&] {
            // what a unit with another id reads: the first live table of this width (see the head of this file)
            const auto safe = std::find_if(ctx->materials.begin(), ctx->materials.end(), [&](const MaterialHost &m) { return live_nch(m, n_ch); });
            no_table = safe == ctx->materials.end();
            return no_table ? tombstone_dev(ctx) : safe->dev;
        },
        [&](const mrl::BatchArgs &a, const float *g, float *grad_wi, float *grad_wo, void *const *) {
            return mrl::launch_table_grad_dir_nch(a, { g, grad_wi, grad_wo }, n_ch, no_table, ctx->compute_units, ctx->stream);
        } });
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
    return nch_grad_dir(ctx, { wi, wo, grad_values, mat, single_id, n, false, nullptr, nullptr, grad_wi, grad_wo }, n_channels);
}

int mrl_table_grad_dir_queue_nch(mrl_ctx *ctx, const float *wi, const float *wo, const float *grad_values, const int32_t *mat, int32_t single_id,
                                 const uint32_t *queue, const uint32_t *queue_count, size_t capacity, int n_channels, float *grad_wi, float *grad_wo)
{
    if (!ctx) return MRL_ERR_INVALID;
    if (const int rc = checked_channels(ctx, n_channels)) return rc;
    if (n_channels == 3) return mrl_table_grad_dir_queue(ctx, wi, wo, grad_values, mat, single_id, queue, queue_count, capacity, grad_wi, grad_wo);
    return nch_grad_dir(ctx, { wi, wo, grad_values, mat, single_id, capacity, true, queue, queue_count, grad_wi, grad_wo }, n_channels);
}

} // extern "C"
