// merl_table_grad_nch.hip — G_k += A_k^T g, the adjoint of eval on n-channel table materials (1..32 channels), over whole arrays, with a
// material id per unit and over wavefront queues, onto several target tables in one launch (include/merl_hip_fit_nch.h,
// mrl_table_grad_batch_nch / mrl_table_grad_queue_nch).  The n-channel twin of merl_table_grad.hip,
// whose kernels, workspace accounting and calls it leaves alone: its per-unit steps are restated here, not shared.
//   k_grad_bricks_nch<LOOKUP, INDEXED>  one lane = one unit, always with targets: the f64 coordinate transform of eval and the eight
//                   F64 corner weights of nch_cell (merl_nch.hip: cell_weights<double> at trilinear_cell / nearest_cell), computed ONCE
//                   per unit and parked in LDS; the wave then loops over the channel groups of 4: each lane loads its up-to-4
//                   grad_values, forms kappa x g in f64, and the wave-transposed scatter adds the 32 values of two units per
//                   wave-instruction (two contiguous 256-B segments) as f64 atomic adds.  Lanes of a wave that share a cell are
//                   summed first when many do (the rule of k_grad_bricks, decided once per round)
//   k_grad_clear_nch  zeros the call's gradient bricks (a kernel, not a memset: see there)
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

namespace mrl {

namespace {

constexpr int kBlock = 256;
constexpr int kBrickSlots = 32;          // doubles per gradient brick (256 B): 8 corners x 4 channels
constexpr int kGroup = 4;                // channels per brick
constexpr int kMergeMin = 4;             // merge a wave's lanes by cell when at least this many share the first live lane's cell
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

// f64 add without a compare-and-swap loop (global_atomic_add_f64); the destinations are device allocations
__device__ __forceinline__ void add_f64(double *p, double v) { (void)unsafeAtomicAdd(p, v); }

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
    const unsigned sub = lane >> 5, slot = lane & 31u;           // two units per wave-instruction, 32 slots each
    const unsigned k = slot >> 2, ch = slot & 3u;
    const bool corner_on = LOOKUP ? true : k == 0u;              // a nearest lookup has corner 0 only
    const unsigned kk = corner_on ? k : 0u;
    const int n_ch = a.n_ch, groups = a.groups;
    const size_t stride = (size_t)gridDim.x * kBlock;
    size_t n_items = a.n;
    if constexpr (INDEXED) { const size_t c = (size_t)*a.idx_count; n_items = c < a.n ? c : a.n; }   // every thread reads the same count
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
        bool merged = a.merge == 2;
        if (a.merge == 0 && live_mask != 0ull) {
            const int c0 = s_cell[wbase + (unsigned)__builtin_ctzll(live_mask)];
            merged = __popcll(__ballot(cell == c0)) >= kMergeMin;
        }
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
            if (live_mask != 0ull) {
                if (!merged) {
                    for (unsigned jj = 0; jj < 64u; jj += 2u) {
                        if (((live_mask >> jj) & 3ull) == 0ull) continue;
                        const unsigned m = wbase + jj + sub;
                        const int cm = s_cell[m];
                        if (slot_on && cm >= 0)
                            add_f64(a.bricks + ((size_t)cm * (size_t)groups + (size_t)group) * kBrickSlots + slot, s_w[kk][m] * s_s[ch][m]);
                    }
                } else {
                    // leader loop: the lanes that hold the first remaining lane's cell are summed by the slot lanes of each half
                    // (low half: members among lanes 0..31, high half: among 32..63), one atomic per slot and half
                    uint64_t rem = live_mask;
                    while (rem != 0ull) {
                        const int c0 = s_cell[wbase + (unsigned)__builtin_ctzll(rem)];
                        const uint64_t members = __ballot(cell == c0);
                        rem &= ~members;
                        uint32_t mm = sub ? (uint32_t)(members >> 32) : (uint32_t)members;
                        if (slot_on && mm != 0u) {
                            double acc = 0.0;
                            while (mm != 0u) {
                                const unsigned m = wbase + 32u * sub + (unsigned)__builtin_ctz(mm);
                                mm &= mm - 1u;
                                acc = __builtin_fma(s_w[kk][m], s_s[ch][m], acc);
                            }
                            add_f64(a.bricks + ((size_t)c0 * (size_t)groups + (size_t)group) * kBrickSlots + slot, acc);
                        }
                    }
                }
            }
            __syncthreads();
        }
    }
}

// The clear of the workspace, as a kernel of this unit and not a memset: a captured queue call is replayed many times, and a memset
// node of this size came back from its second replay on with denormal garbage in place of zeros (measured on ROCm 7.2: every
// replay after the first, the reached texels right and the unreached ones ~1e-308); plain 16-B stores replay like any kernel
__global__ __launch_bounds__(kBlock) void k_grad_clear_nch(double2 *bricks, size_t pairs)
{
    const size_t stride = (size_t)gridDim.x * kBlock;
    for (size_t at = (size_t)blockIdx.x * kBlock + threadIdx.x; at < pairs; at += stride) bricks[at] = make_double2(0.0, 0.0);
}

// the brick slots that reach texel i of an axis of n texels: source s = 0: cell i, corner offset 0; 1: cell i - 1, offset 1;
// 2: the folded corner index n — cell n - 1, offset 1 — onto texel n - 1 (clamped axis) or texel 0 (periodic axis)
__device__ __forceinline__ bool fold_source(int s, int i, int n, bool periodic, int &cell, int &off)
{
    cell = s == 0 ? i : (s == 1 ? i - 1 : n - 1);
    off = s == 0 ? 0 : 1;
    return s == 0 ? true : (s == 1 ? i >= 1 : (periodic ? i == 0 : i == n - 1));
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

hipError_t launch_table_grad_clear_nch(double *bricks, size_t records, int compute_units, hipStream_t stream)
{
    const size_t pairs = records * (kBrickSlots / 2);
    hipLaunchKernelGGL(k_grad_clear_nch, dim3(grad_grid(pairs, compute_units)), dim3(kBlock), 0, stream, (double2 *)bricks, pairs);
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

// One table of a call: its bricks start at cell_base * groups records into the workspace, its planar array at n_ch * cell_base doubles
struct NchGradTable { int dims[3]; int param; size_t cell_base; mrl::NchScales scales; };

// What both calls do once their arguments are checked.  streams: wi, wo, grad_values and (at_mat >= 0) mat; kind: 1 device pointers,
// 0 host arrays; a: everything but the arrays (a.idx: a queue — device pointers only); tables: the call's targets, `cells` cells in
// all.  The workspace is cleared once and folded once, table by table, into the tables' own slices and nothing else.
int run_table_grad_nch(mrl_ctx *ctx, mrl::NchGradArgs a, const StreamList &streams, int at_mat, size_t n, const std::vector<NchGradTable> &tables,
                       size_t cells, double *grad_planar, int kind)
{
    const int variant = ctx->table_grad_kernel;
    const size_t n_ch = (size_t)a.n_ch, brick_bytes = cells * (size_t)a.groups * mrl::kBrickSlots * sizeof(double);
    DeviceBuf &bricks = ctx->buf[mrl_ctx::BUF_GRAD_BRICKS];          // one 256-B record per (cell, channel group); grown on demand, reused
    int rc = bricks.reserve(ctx, brick_bytes);
    if (rc != MRL_OK) return rc;
    a.bricks = (double *)bricks.p;
    MRL_HIP(ctx, mrl::launch_table_grad_clear_nch(a.bricks, cells * (size_t)a.groups, ctx->compute_units, ctx->stream));
    auto on = [&](char *const *addr, size_t m) {
        a.wi = (const float *)addr[0]; a.wo = (const float *)addr[1]; a.g = (const float *)addr[2]; a.n = m;
        a.mat = at_mat >= 0 ? (const int32_t *)addr[at_mat] : nullptr;
    };
    auto fold = [&](double *planar) -> int {
        for (const NchGradTable &t : tables)
            MRL_HIP(ctx, mrl::launch_table_grad_fold_nch(a.bricks + t.cell_base * (size_t)a.groups * mrl::kBrickSlots, planar + n_ch * t.cell_base,
                                                         t.dims, t.param, a.n_ch, t.scales, ctx->compute_units, ctx->stream));
        return MRL_OK;
    };
    if (kind == 1) {
        char *addr[4];
        for (size_t k = 0; k < streams.size(); ++k) addr[k] = (char *)streams[k].ptr;
        on(addr, n);
        MRL_HIP(ctx, mrl::launch_table_grad_nch(a, variant, ctx->compute_units, ctx->stream));
        return fold(grad_planar);
    }
    // host arrays: the inputs are staged chunk by chunk, the sums gathered in a device array and added to the caller's on the host
    double *d_planar = nullptr;
    MRL_ALLOC(ctx, hipMalloc((void **)&d_planar, n_ch * cells * sizeof(double)));
    auto run = [&]() -> int {
        MRL_HIP(ctx, hipMemsetAsync(d_planar, 0, n_ch * cells * sizeof(double), ctx->stream));
        int rc2 = run_host_staged(ctx, streams, n, 0, [&](char *const *addr, size_t m) -> int {
            on(addr, m);
            MRL_HIP(ctx, mrl::launch_table_grad_nch(a, variant, ctx->compute_units, ctx->stream));
            return MRL_OK;
        });
        if (rc2 != MRL_OK) return rc2;
        rc2 = fold(d_planar);
        if (rc2 != MRL_OK) return rc2;
        std::vector<double> sums;
        try { sums.resize(n_ch * cells); } catch (const std::bad_alloc &) { return fail(ctx, MRL_ERR_OOM, "gradient buffer"); }
        MRL_HIP(ctx, hipMemcpyAsync(sums.data(), d_planar, n_ch * cells * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
        MRL_HIP(ctx, hipStreamSynchronize(ctx->stream));
        for (size_t t = 0; t < n_ch * cells; ++t)
            if (sums[t] != 0.0) grad_planar[t] += sums[t];
        return MRL_OK;
    };
    rc = run();
    if (rc != MRL_OK) (void)hipStreamSynchronize(ctx->stream);
    (void)hipFree(d_planar);
    return rc;
}

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

// mrl_table_grad_batch_nch / mrl_table_grad_queue_nch, n_ch != 3; queued: over queue[0 .. min(*queue_count, n)), n its capacity
int table_grad_targets_nch(mrl_ctx *ctx, const float *wi, const float *wo, const float *grad_values, const int32_t *mat, int32_t single_id, size_t n,
                           int n_ch, bool queued, const uint32_t *queue, const uint32_t *queue_count, const int32_t *target_ids, int n_targets,
                           double *grad_planar)
{
    MRL_GUARD(ctx);
    if (n == 0) return MRL_OK;
    StreamList streams = { { (void *)wi, 12, false, "wi" }, { (void *)wo, 12, false, "wo" }, { (void *)grad_values, 4 * (size_t)n_ch, false, "grad_values" } };
    if (first_null(streams) || !grad_planar || !target_ids || (queued && (!queue || !queue_count))) return fail(ctx, MRL_ERR_INVALID, "null array argument");
    int at_mat = -1;
    if (mat) { at_mat = (int)streams.size(); streams.push_back({ (void *)mat, 4, false, "mat" }); }
    if (n_targets < 1 || n_targets > MRL_TABLE_GRAD_MAX_TARGETS)
        return fail(ctx, MRL_ERR_INVALID, "n_targets must be 1.." + std::to_string(MRL_TABLE_GRAD_MAX_TARGETS));
    mrl::NchGradArgs a;
    std::memset(&a, 0, sizeof a);
    int dims[MRL_TABLE_GRAD_MAX_TARGETS][3];
    std::vector<NchGradTable> tables((size_t)n_targets);
    for (int k = 0; k < n_targets; ++k) {
        const int rc = check_grad_table_nch(ctx, target_ids[k], n_ch);
        if (rc != MRL_OK) return rc;
        for (int j = 0; j < k; ++j)
            if (target_ids[j] == target_ids[k]) return fail(ctx, MRL_ERR_INVALID, "a material is listed twice among the targets");
        const MaterialHost &mh = ctx->materials[(size_t)target_ids[k]];
        mrl::NchGradTarget &t = a.targets[k];
        t.id = target_ids[k];
        dims[k][0] = t.n_th = mh.dev.n_th; dims[k][1] = t.n_td = mh.dev.n_td; dims[k][2] = t.n_pd = mh.dev.n_pd; t.param = mh.dev.param;
        NchGradTable &g = tables[(size_t)k];
        g.dims[0] = t.n_th; g.dims[1] = t.n_td; g.dims[2] = t.n_pd; g.param = t.param;
        std::memset(&g.scales, 0, sizeof g.scales);
        for (int c = 0; c < n_ch; ++c) g.scales.s[c] = mh.nch_scale[(size_t)c];
    }
    // where each target's bricks and planar array start: the one place that adds the cells up and bounds the brick index
    size_t offsets[MRL_TABLE_GRAD_MAX_TARGETS + 1];
    if (mrl_table_grad_layout_nch(&dims[0][0], n_targets, n_ch, offsets) != MRL_OK)
        return fail(ctx, MRL_ERR_INVALID, "the targets have more than 2^31 - 1 gradient bricks in all");
    for (int k = 0; k < n_targets; ++k) {
        a.targets[k].cell_base = (int)(offsets[k] / (size_t)n_ch);
        tables[(size_t)k].cell_base = offsets[k] / (size_t)n_ch;
    }
    const size_t cells = offsets[n_targets] / (size_t)n_ch;
    a.n_targets = n_targets;
    a.n_ch = n_ch; a.groups = (n_ch + mrl::kGroup - 1) / mrl::kGroup;
    if (ctx->opts.negative == mrl::NEGATIVE_RENORMALISE)
        return fail(ctx, MRL_ERR_INVALID, "MRL_OPT_NEGATIVE = renormalise makes eval non-linear in the table: no adjoint");
    if (queued && n > ((size_t)1 << 32)) return fail(ctx, MRL_ERR_INVALID, "queue capacity exceeds 2^32 (indices are uint32)");
    MRL_HIP(ctx, hipSetDevice(ctx->device));
    const int kind = queued ? common_kind({ grad_planar, queue, queue_count }, streams) : common_kind({ grad_planar }, streams);
    if (queued && kind != 1) return fail(ctx, MRL_ERR_POINTER_MIX, "queue calls take device pointers only");
    if (kind < 0) return fail(ctx, MRL_ERR_POINTER_MIX, "host and device pointers mixed in one call");
    a.opts = ctx->opts;
    a.single_id = single_id;
    a.idx = queue; a.idx_count = queue_count;
    return run_table_grad_nch(ctx, a, streams, at_mat, n, tables, cells, grad_planar, kind);
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
    return table_grad_targets_nch(ctx, wi, wo, grad_values, mat, single_id, n, n_channels, false, nullptr, nullptr, target_ids, n_targets, grad_planar);
}

int mrl_table_grad_queue_nch(mrl_ctx *ctx, const float *wi, const float *wo, const float *grad_values, const int32_t *mat, int32_t single_id,
                             const uint32_t *queue, const uint32_t *queue_count, size_t capacity, int n_channels, const int32_t *target_ids,
                             int n_targets, double *grad_planar)
{
    if (!ctx) return MRL_ERR_INVALID;
    const int rc = check_channels(ctx, n_channels);
    if (rc != MRL_OK) return rc;
    if (n_channels == 3) return mrl_table_grad_queue(ctx, wi, wo, grad_values, mat, single_id, queue, queue_count, capacity, target_ids, n_targets, grad_planar);
    return table_grad_targets_nch(ctx, wi, wo, grad_values, mat, single_id, capacity, n_channels, true, queue, queue_count, target_ids, n_targets,
                                  grad_planar);
}

} // extern "C"
