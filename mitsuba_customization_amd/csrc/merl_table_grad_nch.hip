// merl_table_grad_nch.hip — G_k += A_k^T g, the adjoint of eval on n-channel table materials (1..32 channels), over whole arrays, with a
// material id per unit and over wavefront queues, onto several target tables in one launch (include/merl_hip_fit_nch.h,
// mrl_table_grad_batch_nch / mrl_table_grad_queue_nch).  The n-channel twin of merl_table_grad.hip:
// the wave's scatter (merl_grad_scatter.hpp) and the host call with its clear (grad_scatter_call, merl_grad_scatter.hip) are the ones
// all adjoints share; the per-unit computation, the brick layout and the fold are this file's own.
//   k_grad_bricks_nch<LOOKUP, INDEXED>  one lane = one unit, always with targets: the f64 coordinate transform of eval and the eight
//                   F64 corner weights of nch_cell (merl_nch.hip: cell_weights<double> at trilinear_cell / nearest_cell), computed ONCE
//                   per unit and parked in LDS; the wave then loops over the channel groups of 4: each lane loads its up-to-4
//                   grad_values, forms kappa x g in f64, and the wave-transposed scatter adds the 32 values of two units per
//                   wave-instruction (two contiguous 256-B segments) as f64 atomic adds.  Lanes of a wave that share a cell are
//                   summed first when many do (the rule of k_grad_bricks, decided once per round)
//   k_grad_fold_nch per texel and channel group: the sum of the brick slots that map to the texel (clamp / wrap folding), times the
//                   target's channel scale, added into the caller's planar array
// Gradient brick of (cell, group): 32 doubles, slot 4 k + ch for corner k = 4 a + 2 b + c (cell_weights' order) and channel 4 group + ch:
// all 32 used in a full group; slots of channels >= n_ch in the last group are never added to and never folded.  Record index
// (cell_base + cell) * groups + group with groups = ceil(n_ch / 4) for every width: the mirror of the forward layout's "ceil(n_ch / 4)
// contiguous lines per cell".  The channel scales do not travel with the accumulate kernel (16 targets x 32 doubles would not fit the
// kernel arguments): the fold, launched once per target, takes that target's scales by value.
#include "merl_ctx.hpp"
#include "../../include/merl_hip_fit_nch.h"
#include "merl_table_fast.hpp"
#include "merl_grad_scatter.hpp"

namespace mrl {

namespace {

constexpr int kBlock = 256;
constexpr int kBrickSlots = 32;          // doubles per gradient brick (256 B): 8 corners x 4 channels
constexpr int kGroup = 4;                // channels per brick
constexpr int kMaxTargets = MRL_TABLE_GRAD_MAX_TARGETS;

// One target table of a launch: what the accumulate kernel needs of it, by value in the kernel arguments (a queue call is capturable
// in a HIP graph: nothing is copied from host memory at call time).  24 B; 16 of them are 384 B
struct NchGradTarget {
    int id;                              // the material id a unit must carry
    int n_th, n_td, n_pd, param;
    int cell_base;                       // cells of the targets before it
};

struct NchGradArgs {
    const float *wi, *wo, *g;            // g: [n][n_ch], rows 4-byte aligned
    size_t n;                            // units; of a queue launch the queue's capacity
    Options opts;
    double *bricks;                      // [cells of all targets][groups][kBrickSlots]
    int merge;                           // 0: wave-uniform choice, 1: never, 2: always
    int n_ch, groups;
    const int32_t *mat;                  // a unit's material is mat[i], or single_id where mat is null
    int32_t single_id;
    const uint32_t *idx, *idx_count;     // INDEXED: the units idx[0 .. min(*idx_count, n))
    int n_targets;
    NchGradTarget targets[kMaxTargets];
};

// the channel scales of one target, by value in the fold's arguments
struct NchScales { double s[kMaxChannels]; };

// The table a unit adds into; known: false for a unit whose id names no target — it computes on target 0's shape and is masked
struct NchGradShape { int n_th, n_td, n_pd, param, cell_base; bool known; };

// the target with this id: every lane walks all n_targets descriptors (a wave-uniform trip count, scalar loads) and selects
__device__ __forceinline__ NchGradShape target_shape(const NchGradArgs &a, int id)
{
    const NchGradTarget &t0 = a.targets[0];
    NchGradShape s = { t0.n_th, t0.n_td, t0.n_pd, t0.param, t0.cell_base, false };
    for (int k = 0; k < a.n_targets; ++k) {
        const NchGradTarget &t = a.targets[k];
        const bool hit = t.id == id;
        s.n_th = hit ? t.n_th : s.n_th; s.n_td = hit ? t.n_td : s.n_td; s.n_pd = hit ? t.n_pd : s.n_pd;
        s.param = hit ? t.param : s.param; s.cell_base = hit ? t.cell_base : s.cell_base;
        s.known = s.known || hit;
    }
    return s;
}

template <int LOOKUP, bool INDEXED>
__global__ __launch_bounds__(kBlock) void k_grad_bricks_nch(NchGradArgs a)
{
#pragma clang fp contract(off)
    // what the lanes of a wave hand to each other: k-major / channel-major, so that 64 lanes write 64 consecutive doubles.  The
    // transposed reads take one unit's values for all k (s_w[k][m]) and all four channels (s_s[ch][m]) in one instruction: the rows are
    // padded by one element so that those land on different LDS banks (a row stride of 2 kBlock words would put all of them on one)
    __shared__ int s_cell[kBlock];
    __shared__ double s_w[8][kBlock + 1];
    __shared__ double s_s[kGroup][kBlock + 1];
    const unsigned t = threadIdx.x, lane = t & 63u, wbase = t & ~63u;
    const unsigned slot = lane & 31u;                            // two units per wave-instruction, 32 slots each
    const unsigned k = slot >> 2, ch = slot & 3u;
    const bool corner_on = LOOKUP ? true : k == 0u;              // a nearest lookup has corner 0 only
    const unsigned kk = corner_on ? k : 0u;
    const int n_ch = a.n_ch, groups = a.groups;
    const size_t stride = (size_t)gridDim.x * kBlock;
    const size_t n_items = grad_items<INDEXED>(a.n, a.idx_count);
    const size_t rounds = (n_items + stride - 1) / stride;       // the same trip count for every thread: barriers inside
    for (size_t r = 0; r < rounds; ++r) {
        const size_t j = r * stride + (size_t)blockIdx.x * kBlock + t;
        const bool in_range = j < n_items;
        size_t i = j;
        if constexpr (INDEXED) i = in_range ? (size_t)a.idx[j] : 0;
        int id = a.single_id;
        if (a.mat) id = in_range ? a.mat[i] : -1;                // a position past the end names no target
        const NchGradShape shape = target_shape(a, id);
        const fast::TableMaps maps(shape.n_th, shape.n_td, shape.n_pd, shape.param);
        float wix = 0.0f, wiy = 0.0f, wiz = 0.0f, wox = 0.0f, woy = 0.0f, woz = 0.0f;
        if (in_range) {
            load3(a.wi, i, wix, wiy, wiz);
            load3(a.wo, i, wox, woy, woz);
        }
        // the factor eval multiplies by: Float wo.z (or 1), NaN when a component of either direction is not finite
        const float c32 = fast::cos_or_nan32((wix + wiy + wiz), wox, woy, woz, a.opts.cosine != 0);
        const bool live = in_range && shape.known && (wiz > 0.0f) && (woz > 0.0f) && (c32 == c32);
        const fast::Vec3 in = fast::normalize_f32(wix, wiy, wiz);
        const Coords c = maps(in, fast::dir_f32(wox, woy, woz));
        // eval's own cell and weights (nch_cell of merl_nch.hip; a nearest lookup: all weight on corner 0)
        TableCell tc = LOOKUP ? trilinear_cell(c, shape.n_th, shape.n_td, shape.n_pd, a.opts.node, shape.param)
                              : nearest_cell(c, shape.n_th, shape.n_td, shape.n_pd);
        const CellWeights cw = cell_weights<double>(tc.fh, tc.fd, tc.fp);
        // a dead unit's coordinates are garbage: whatever they are, the cell stays inside the table (nearest_cell's already does)
        if constexpr (LOOKUP) {
            tc.h0 = clampi(tc.h0, 0, shape.n_th - 1); tc.d0 = clampi(tc.d0, 0, shape.n_td - 1); tc.p0 = clampi(tc.p0, 0, shape.n_pd - 1);
        }
        // the global cell: two lanes are summed together only when they share target and cell
        const int cell = live ? shape.cell_base + cell_index<int>(tc, shape.n_td, shape.n_pd) : -1;
        const double kappa = (double)c32;
        s_cell[t] = cell;
#pragma unroll
        for (int q = 0; q < (LOOKUP ? 8 : 1); ++q) s_w[q][t] = live ? cw.w[q] : 0.0;
        __syncthreads();
        const uint64_t live_mask = __ballot(cell >= 0);          // wave-uniform, like everything decided from it
        const bool merged = wave_merge_rule(a.merge, cell, s_cell, wbase, live_mask);        // once per round, for every channel group
        const float *row = a.g + i * (size_t)n_ch;
        for (int group = 0; group < groups; ++group) {           // the same trip count for every thread
            const int first = kGroup * group;
            // masking is a select: a dead unit's g may be NaN
#pragma unroll
            for (int q = 0; q < kGroup; ++q) {
                float gq = 0.0f;
                if (in_range && first + q < n_ch) gq = row[first + q];
                s_s[q][t] = live ? kappa * (double)gq : 0.0;
            }
            __syncthreads();
            const bool slot_on = corner_on && first + (int)ch < n_ch;
            wave_scatter<32>(live_mask, merged, cell, s_cell, wbase, lane,
                [&](unsigned) { return slot_on; },
                [&](unsigned m, unsigned) { return s_w[kk][m] * s_s[ch][m]; },
                [&](double acc, unsigned m, unsigned) { return __builtin_fma(s_w[kk][m], s_s[ch][m], acc); },
                [&](unsigned ref) { return a.bricks + ((size_t)s_cell[ref] * (size_t)groups + (size_t)group) * kBrickSlots + slot; });
            __syncthreads();
        }
    }
}

// bricks / planar: the target's own; one thread per (texel, channel group), texels adjacent across lanes
__global__ __launch_bounds__(kBlock) void k_grad_fold_nch(const double *bricks, double *planar, int n_th, int n_td, int n_pd, int periodic_phi,
                                                          int n_ch, NchScales scales)
{
    const int groups = (n_ch + kGroup - 1) / kGroup;
    const size_t plane = (size_t)n_th * n_td * n_pd, total = plane * (size_t)groups;
    const size_t stride = (size_t)gridDim.x * kBlock;
    for (size_t at = (size_t)blockIdx.x * kBlock + threadIdx.x; at < total; at += stride) {
        const size_t t = at % plane;
        const int group = (int)(at / plane);
        const int p = (int)(t % (size_t)n_pd);
        const int d = (int)((t / (size_t)n_pd) % (size_t)n_td);
        const int h = (int)(t / ((size_t)n_pd * n_td));
        double acc[kGroup] = { 0.0, 0.0, 0.0, 0.0 };
#pragma unroll
        for (int sh = 0; sh < 3; ++sh) {
            int hc, ho;
            if (!fold_source(sh, h, n_th, false, hc, ho)) continue;
#pragma unroll
            for (int sd = 0; sd < 3; ++sd) {
                int dc, dO;
                if (!fold_source(sd, d, n_td, false, dc, dO)) continue;
#pragma unroll
                for (int sp = 0; sp < 3; ++sp) {
                    int pc, po;
                    if (!fold_source(sp, p, n_pd, periodic_phi != 0, pc, po)) continue;
                    const size_t cell = ((size_t)hc * n_td + dc) * n_pd + pc;
                    const double *b = bricks + (cell * (size_t)groups + (size_t)group) * kBrickSlots + kGroup * (4 * ho + 2 * dO + po);
#pragma unroll
                    for (int q = 0; q < kGroup; ++q) acc[q] += b[q];     // slots of channels >= n_ch hold the zeros of the clear
                }
            }
        }
        // a texel nothing reached keeps its bits (x + 0 would turn -0 into +0)
#pragma unroll
        for (int q = 0; q < kGroup; ++q) {
            const int channel = kGroup * group + q;
            if (channel < n_ch && acc[q] != 0.0) planar[(size_t)channel * plane + t] += acc[q] * scales.s[channel];
        }
    }
}

unsigned grad_grid(size_t n, int compute_units) { return grid_blocks(n, kBlock, (size_t)compute_units * 8); }

// variant: MRL_OPT_TABLE_GRAD_KERNEL (1, the plain planar form, is not built here: as 2).  Adds the units' values into a.bricks (zeroed
// by the caller); a.idx: over a queue of capacity a.n
hipError_t launch_table_grad_nch(NchGradArgs a, int variant, int compute_units, hipStream_t stream)
{
    if (a.n == 0) return hipSuccess;
    const dim3 grid(grad_grid(a.n, compute_units)), block(kBlock);
    a.merge = variant == 3 ? 2 : (variant == 0 ? 0 : 1);
    with_flags([&](auto tri, auto idx) { hipLaunchKernelGGL((k_grad_bricks_nch<tri ? 1 : 0, idx>), grid, block, 0, stream, a); },
               a.opts.lookup != 0, a.idx != nullptr);
    return hipGetLastError();
}

hipError_t launch_table_grad_fold_nch(const double *bricks, double *planar, const int dims[3], int param, int n_ch, const NchScales &scales,
                                      int compute_units, hipStream_t stream)
{
    const size_t total = (size_t)dims[0] * dims[1] * dims[2] * (size_t)((n_ch + kGroup - 1) / kGroup);
    hipLaunchKernelGGL(k_grad_fold_nch, dim3(grad_grid(total, compute_units)), dim3(kBlock), 0, stream, bricks, planar, dims[0], dims[1], dims[2],
                       param_phi_periodic(param) ? 1 : 0, n_ch, scales);
    return hipGetLastError();
}

} // namespace

} // namespace mrl

using namespace mrlabi;

namespace {

// is `id` a table the n-channel adjoint is defined for at this width?  MRL_OK, or the failure the header documents
int check_grad_table_nch(mrl_ctx *ctx, int32_t id, int n_ch)
{
    if (id < 0 || (size_t)id >= ctx->materials.size() || ctx->materials[(size_t)id].released) return fail(ctx, MRL_ERR_MATERIAL, "unknown material id");
    const MaterialHost &mh = ctx->materials[(size_t)id];
    if (mh.dev.kind != mrl::KIND_TABLE_NCH || mh.dev.n_ch != n_ch)
        return fail(ctx, MRL_ERR_MATERIAL, "a target is not an n-channel table of " + std::to_string(n_ch) + " channels");
    if (mh.nch_scale.size() != (size_t)n_ch) return fail(ctx, MRL_ERR_MATERIAL, "a table restored from an image file does not carry its channel scales");
    return MRL_OK;
}

// mrl_table_grad_batch_nch / mrl_table_grad_queue_nch, n_ch != 3: the checks, the workspace and the host-array path are
// grad_scatter_call's (merl_grad_scatter.hip)
int table_grad_nch(mrl_ctx *ctx, const GradScatterCall &c, int n_ch)
{
    mrl::NchGradArgs a;
    std::memset(&a, 0, sizeof a);
    std::vector<mrl::NchScales> scales;                          // per target: what its fold multiplies by
    return grad_scatter_call(ctx, c, {
        [&](int32_t id) { return check_grad_table_nch(ctx, id, n_ch); },
        [&](GradScatterLayout &lay) -> int {
            int dims[MRL_TABLE_GRAD_MAX_TARGETS][3];
            scales.assign((size_t)c.n_targets, mrl::NchScales{});
            for (int k = 0; k < c.n_targets; ++k) {
                const MaterialHost &mh = ctx->materials[(size_t)c.target_ids[k]];
                mrl::NchGradTarget &t = a.targets[k];
                t.id = c.target_ids[k];
                dims[k][0] = t.n_th = mh.dev.n_th; dims[k][1] = t.n_td = mh.dev.n_td; dims[k][2] = t.n_pd = mh.dev.n_pd; t.param = mh.dev.param;
                for (int ch = 0; ch < n_ch; ++ch) scales[(size_t)k].s[ch] = mh.nch_scale[(size_t)ch];
            }
            // where each target's bricks (cell_base * groups records into the workspace) and planar array (n_ch * cell_base doubles into
            // out) start: the one place that adds the cells up and bounds the brick index
            size_t offsets[MRL_TABLE_GRAD_MAX_TARGETS + 1];
            if (mrl_table_grad_layout_nch(&dims[0][0], c.n_targets, n_ch, offsets) != MRL_OK)
                return fail(ctx, MRL_ERR_INVALID, "the targets have more than 2^31 - 1 gradient bricks in all");
            for (int k = 0; k < c.n_targets; ++k) a.targets[k].cell_base = (int)(offsets[k] / (size_t)n_ch);
            a.n_targets = c.n_targets;
            a.n_ch = n_ch; a.groups = (n_ch + mrl::kGroup - 1) / mrl::kGroup;
            a.opts = ctx->opts;
            a.single_id = c.single_id;
            a.idx = c.queue; a.idx_count = c.queue_count;
            // one 256-B record per (cell, channel group); every variant goes through the bricks
            lay.brick_bytes = offsets[c.n_targets] / (size_t)n_ch * (size_t)a.groups * mrl::kBrickSlots * sizeof(double);
            lay.out_doubles = offsets[c.n_targets];
            return MRL_OK;
        },
        true,
        [&](char *const *addr, size_t m, double *bricks, double *) {
            a.wi = (const float *)addr[0]; a.wo = (const float *)addr[1]; a.g = (const float *)addr[2]; a.n = m;
            a.mat = c.mat ? (const int32_t *)addr[3] : nullptr;
            a.bricks = bricks;
            return mrl::launch_table_grad_nch(a, ctx->table_grad_kernel, ctx->compute_units, ctx->stream);
        },
        [&](const double *bricks, double *out) {
            hipError_t e = hipSuccess;
            for (int k = 0; k < c.n_targets && e == hipSuccess; ++k) {
                const mrl::NchGradTarget &t = a.targets[k];
                const int dims[3] = { t.n_th, t.n_td, t.n_pd };
                e = mrl::launch_table_grad_fold_nch(bricks + (size_t)t.cell_base * (size_t)a.groups * mrl::kBrickSlots, out + (size_t)n_ch * (size_t)t.cell_base,
                                                    dims, t.param, n_ch, scales[(size_t)k], ctx->compute_units, ctx->stream);
            }
            return e;
        } });
}

// the channel count every *_nch call takes: MRL_OK, or what mrl_eval_batch_nch returns for it
int check_channels(mrl_ctx *ctx, int n_channels)
{
    if (n_channels < 1 || n_channels > mrl::kMaxChannels) return fail(ctx, MRL_ERR_INVALID, "channel count must be 1.." + std::to_string(mrl::kMaxChannels));
    return MRL_OK;
}

} // namespace

extern "C" {

int mrl_table_grad_layout_nch(const int *dims, int n_targets, int n_channels, size_t *offsets_out)
{
    if (n_channels < 1 || n_channels > mrl::kMaxChannels) return MRL_ERR_INVALID;
    if (n_channels == 3) return mrl_table_grad_layout(dims, n_targets, offsets_out);
    // everything the RGB layout refuses (NULL dims, n_targets, a dim below 1, more than 2^31 - 1 cells): its offsets are 3 sum cells
    size_t rgb[MRL_TABLE_GRAD_MAX_TARGETS + 1];
    const int rc = mrl_table_grad_layout(dims, n_targets, rgb);
    if (rc != MRL_OK) return rc;
    const uint64_t groups = (uint64_t)((n_channels + mrl::kGroup - 1) / mrl::kGroup);
    if ((uint64_t)(rgb[n_targets] / 3) * groups > (uint64_t)INT32_MAX) return MRL_ERR_INVALID;      // at most 2^34: no wrap
    if (offsets_out)
        for (int k = 0; k <= n_targets; ++k) offsets_out[k] = (rgb[k] / 3) * (size_t)n_channels;
    return MRL_OK;
}

int mrl_table_grad_batch_nch(mrl_ctx *ctx, const float *wi, const float *wo, const float *grad_values, const int32_t *mat, int32_t single_id, size_t n,
                             int n_channels, const int32_t *target_ids, int n_targets, double *grad_planar)
{
    if (!ctx) return MRL_ERR_INVALID;
    const int rc = check_channels(ctx, n_channels);
    if (rc != MRL_OK) return rc;
    if (n_channels == 3) return mrl_table_grad_batch_mat(ctx, wi, wo, grad_values, mat, single_id, n, target_ids, n_targets, grad_planar);
    return table_grad_nch(ctx, { wi, wo, grad_values, 4 * (size_t)n_channels, "grad_values", mat, single_id, n, false, nullptr, nullptr, target_ids,
                                 n_targets, MRL_TABLE_GRAD_MAX_TARGETS, grad_planar }, n_channels);
}

int mrl_table_grad_queue_nch(mrl_ctx *ctx, const float *wi, const float *wo, const float *grad_values, const int32_t *mat, int32_t single_id,
                             const uint32_t *queue, const uint32_t *queue_count, size_t capacity, int n_channels, const int32_t *target_ids,
                             int n_targets, double *grad_planar)
{
    if (!ctx) return MRL_ERR_INVALID;
    const int rc = check_channels(ctx, n_channels);
    if (rc != MRL_OK) return rc;
    if (n_channels == 3) return mrl_table_grad_queue(ctx, wi, wo, grad_values, mat, single_id, queue, queue_count, capacity, target_ids, n_targets, grad_planar);
    return table_grad_nch(ctx, { wi, wo, grad_values, 4 * (size_t)n_channels, "grad_values", mat, single_id, capacity, true, queue, queue_count,
                                 target_ids, n_targets, MRL_TABLE_GRAD_MAX_TARGETS, grad_planar }, n_channels);
}

} // extern "C"
