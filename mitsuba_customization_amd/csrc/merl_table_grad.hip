// merl_table_grad.hip — G += A^T g, the adjoint of eval on RGB table materials: on one (include/merl_hip.h, mrl_table_grad_batch;
// DESIGN.md §5g) and, with a material id per unit or over a wavefront queue, onto several target tables in one launch
// (include/merl_hip_fit_table.h, mrl_table_grad_batch_mat / mrl_table_grad_queue).  The forward kernels gather;
// this one scatters, and its destinations collide where measured BRDFs are interesting.  The texels are never read: the call needs the material's dims, parameterisation and scale only, so one kernel
// serves both table layouts.
//   k_grad_bricks   one lane = one unit: the f64 coordinate transform of eval, the Float corner weights; the wave then transposes
//                   through LDS so that one wave-instruction carries the 24 values of two units (two contiguous 192-B segments of
//                   the gradient bricks) as f64 atomic adds.  Lanes of a wave that share a cell are summed first when many do
//                   (wave_merge_rule / wave_scatter of merl_grad_scatter.hpp, which every adjoint's kernel runs).
//   k_grad_fold     per texel: the sum of the brick slots that map to it (clamp / wrap folding), added into the caller's planar array
//   k_grad_naive    the A/B baseline: each lane adds its 24 values straight into the planar array (64 lanes, 64 rows)
// Gradient brick of cell (h0, d0, p0): 32 doubles, slot 3 k + ch for corner k = 4 a + 2 b + c (corner_weights' order), 24 used.
// Each kernel body is written once, as a device function templated on PER_LANE (the unit's table is the target its material id
// names: dims, parameterisation, scale and the first cell of the target's bricks come from a by-value descriptor array) and INDEXED
// (the launch walks a queue).  k_grad_bricks / k_grad_naive are the <false, false> bodies, the single-material call's code;
// k_grad_bricks_mat / k_grad_naive_mat<LOOKUP, INDEXED> the PER_LANE ones.  With targets the kernels work on a GLOBAL cell index,
// cell_base + cell: two lanes are summed together only when they share target and cell.
#include "merl_ctx.hpp"
#include "../../include/merl_hip_fit_table.h"
#include "merl_table_fast.hpp"
#include "merl_grad_scatter.hpp"

namespace mrl {

namespace {

constexpr int kBlock = 256;
constexpr int kBrickSlots = 32;          // doubles per gradient brick (256 B)

// One target table of a launch with material ids: what the kernels need of it, by value in the kernel arguments (a queue call is
// capturable in a HIP graph: nothing is copied from host memory at call time).  48 B
struct GradTarget {
    int id;                              // the material id a unit must carry
    int n_th, n_td, n_pd, param;
    int cell_base;                       // cells of the targets before it: its first brick, and a third of its planar offset
    double scale[3];
};
// MRL_TABLE_GRAD_MAX_TARGETS descriptors are 768 B: GradArgs stays below 1 KiB of the 4 KiB a kernel's arguments may take
constexpr int kMaxTargets = MRL_TABLE_GRAD_MAX_TARGETS;

struct GradArgs {
    const float *wi, *wo, *g;
    size_t n;                            // units; of a queue launch the queue's capacity
    int n_th, n_td, n_pd, param;         // the single-material launch's table
    Options opts;
    double scale[3];
    double *bricks;                      // [cells][kBrickSlots]; with targets: of all targets, end to end
    double *planar;                      // k_grad_naive: [3][n_th][n_td][n_pd]; with targets: the targets' planar arrays end to end
    int merge;                           // 0: wave-uniform choice, 1: never, 2: always
    // launches with targets (PER_LANE): a unit's material is mat[i], or single_id where mat is null
    const int32_t *mat;
    int32_t single_id;
    const uint32_t *idx, *idx_count;     // INDEXED: the units idx[0 .. min(*idx_count, n))
    int n_targets;
    GradTarget targets[kMaxTargets];
};

// The table a unit adds into; known: false for a unit whose id names no target — it computes on target 0's shape and is masked
struct GradShape {
    int n_th, n_td, n_pd, param, cell_base;
    double scale[3];
    bool known;
};
__device__ __forceinline__ GradShape single_shape(const GradArgs &a)
{
    return { a.n_th, a.n_td, a.n_pd, a.param, 0, { a.scale[0], a.scale[1], a.scale[2] }, true };
}
// the target with this id: every lane walks all n_targets descriptors (a wave-uniform trip count, scalar loads) and selects
__device__ __forceinline__ GradShape target_shape(const GradArgs &a, int id)
{
    const GradTarget &t0 = a.targets[0];
    GradShape s = { t0.n_th, t0.n_td, t0.n_pd, t0.param, t0.cell_base, { t0.scale[0], t0.scale[1], t0.scale[2] }, false };
    for (int k = 0; k < a.n_targets; ++k) {
        const GradTarget &t = a.targets[k];
        const bool hit = t.id == id;
        s.n_th = hit ? t.n_th : s.n_th; s.n_td = hit ? t.n_td : s.n_td; s.n_pd = hit ? t.n_pd : s.n_pd;
        s.param = hit ? t.param : s.param; s.cell_base = hit ? t.cell_base : s.cell_base;
        s.scale[0] = hit ? t.scale[0] : s.scale[0]; s.scale[1] = hit ? t.scale[1] : s.scale[1]; s.scale[2] = hit ? t.scale[2] : s.scale[2];
        s.known = s.known || hit;
    }
    return s;
}
// What unit i adds: the cell of its lookup (eval's own TableCell, kept inside the table; the kernels read its indices only), whether
// eval masks the unit, the Float corner weights and, per channel, scale x (cos(theta_o) or 1) x g in f64.  Masking is a select: a dead unit's g may be NaN.
struct GradUnit {
    TableCell cell;
    bool live;
    float w[8];
    double s[3];
};

// t: the unit's table (single_shape, or the target its id names), maps: that table's coordinate maps; in_range: unit i exists
template <int LOOKUP>
__device__ __forceinline__ GradUnit grad_unit(const GradArgs &a, const GradShape &t, const fast::TableMaps &maps, size_t i, bool in_range)
{
#pragma clang fp contract(off)
    float wix = 0.0f, wiy = 0.0f, wiz = 0.0f, wox = 0.0f, woy = 0.0f, woz = 0.0f, g0 = 0.0f, g1 = 0.0f, g2 = 0.0f;
    if (in_range) {
        load3(a.wi, i, wix, wiy, wiz);
        load3(a.wo, i, wox, woy, woz);
        load3(a.g, i, g0, g1, g2);
    }
    // the factor eval_tail multiplies by: Float wo.z (or 1), NaN when a component of either direction is not finite
    const float c32 = fast::cos_or_nan32((wix + wiy + wiz), wox, woy, woz, a.opts.cosine != 0);
    GradUnit u;
    u.live = in_range && t.known && (wiz > 0.0f) && (woz > 0.0f) && (c32 == c32);
    const fast::Vec3 in = fast::normalize_f32(wix, wiy, wiz);
    const Coords c = maps(in, fast::dir_f32(wox, woy, woz));
    // eval's own cell and weights (a nearest lookup: all weight on corner 0)
    u.cell = LOOKUP ? trilinear_cell(c, t.n_th, t.n_td, t.n_pd, a.opts.node, t.param) : nearest_cell(c, t.n_th, t.n_td, t.n_pd);
    const CornerWeights cw = corner_weights(u.cell.fh, u.cell.fd, u.cell.fp);
#pragma unroll
    for (int k = 0; k < 8; ++k) u.w[k] = u.live ? cw.w[k] : 0.0f;
    // a dead unit's coordinates are garbage: whatever they are, the cell stays inside the table (nearest_cell's already does)
    if constexpr (LOOKUP) {
        u.cell.h0 = clampi(u.cell.h0, 0, t.n_th - 1); u.cell.d0 = clampi(u.cell.d0, 0, t.n_td - 1); u.cell.p0 = clampi(u.cell.p0, 0, t.n_pd - 1);
    }
    const double cd = (double)c32;
    u.s[0] = u.live ? t.scale[0] * cd * (double)g0 : 0.0;
    u.s[1] = u.live ? t.scale[1] * cd * (double)g1 : 0.0;
    u.s[2] = u.live ? t.scale[2] * cd * (double)g2 : 0.0;
    return u;
}

// the table of the unit at queue position / index j (PER_LANE: its target's; a position past the end names no target)
template <bool PER_LANE>
__device__ __forceinline__ void unit_table(const GradArgs &a, size_t i, bool in_range, GradShape &shape, fast::TableMaps &maps)
{
    if constexpr (PER_LANE) {
        int id = a.single_id;
        if (a.mat) id = in_range ? a.mat[i] : -1;
        shape = target_shape(a, id);
        maps = fast::TableMaps(shape.n_th, shape.n_td, shape.n_pd, shape.param);
    }
}

template <int LOOKUP, bool PER_LANE, bool INDEXED>
__device__ __forceinline__ void grad_bricks(const GradArgs &a)
{
    // what the lanes of a wave hand to each other: k-major, so that 64 lanes write 64 consecutive words.  The transposed reads take
    // one unit's values for all k (s_w[k][m]) and all channels (s_s[ch][m]) in one instruction: the rows are padded by one element so
    // that those land on different LDS banks (a row stride of kBlock words would put all eight k on one bank)
    __shared__ int s_cell[kBlock];
    __shared__ float s_w[8][kBlock + 1];
    __shared__ double s_s[3][kBlock + 1];
    GradShape shape = single_shape(a);                           // !PER_LANE: wave-uniform, formed once
    fast::TableMaps maps(shape.n_th, shape.n_td, shape.n_pd, shape.param);
    const unsigned t = threadIdx.x, lane = t & 63u, wbase = t & ~63u;
    const unsigned slot = lane & 31u;                            // two units per wave-instruction, 32 slots each (24 used)
    const unsigned k = slot / 3u, ch = slot - 3u * k;
    const bool slot_on = slot < (LOOKUP ? 24u : 3u);             // a nearest lookup has corner 0 only
    const unsigned kk = slot_on ? k : 0u, cc = slot_on ? ch : 0u;
    const size_t stride = (size_t)gridDim.x * kBlock;
    const size_t n_items = grad_items<INDEXED>(a.n, a.idx_count);
    const size_t rounds = (n_items + stride - 1) / stride;       // the same trip count for every thread: barriers inside
    for (size_t r = 0; r < rounds; ++r) {
        const size_t j = r * stride + (size_t)blockIdx.x * kBlock + t;
        const bool in_range = j < n_items;
        size_t i = j;
        if constexpr (INDEXED) i = in_range ? (size_t)a.idx[j] : 0;
        unit_table<PER_LANE>(a, i, in_range, shape, maps);
        const GradUnit u = grad_unit<LOOKUP>(a, shape, maps, i, in_range);
        // the global cell: of a launch without targets the table's own (cell_base is 0)
        const int cell = u.live ? shape.cell_base + cell_index<int>(u.cell, shape.n_td, shape.n_pd) : -1;
        s_cell[t] = cell;
#pragma unroll
        for (int q = 0; q < (LOOKUP ? 8 : 1); ++q) s_w[q][t] = u.w[q];
        s_s[0][t] = u.s[0]; s_s[1][t] = u.s[1]; s_s[2][t] = u.s[2];
        __syncthreads();
        const uint64_t live = __ballot(cell >= 0);
        // lanes of a wave that share a cell are summed first when many do: an fma chain over a cell's members, one atomic per slot
        wave_scatter<32>(live, wave_merge_rule(a.merge, cell, s_cell, wbase, live), cell, s_cell, wbase, lane,
            [&](unsigned) { return slot_on; },
            [&](unsigned m, unsigned) { return (double)s_w[kk][m] * s_s[cc][m]; },
            [&](double acc, unsigned m, unsigned) { return __builtin_fma((double)s_w[kk][m], s_s[cc][m], acc); },
            [&](unsigned ref) { return a.bricks + (size_t)s_cell[ref] * kBrickSlots + slot; });
        __syncthreads();
    }
}

template <int LOOKUP>
__global__ __launch_bounds__(kBlock) void k_grad_bricks(GradArgs a) { grad_bricks<LOOKUP, false, false>(a); }
template <int LOOKUP, bool INDEXED>
__global__ __launch_bounds__(kBlock) void k_grad_bricks_mat(GradArgs a) { grad_bricks<LOOKUP, true, INDEXED>(a); }

__global__ __launch_bounds__(kBlock) void k_grad_fold(const double *bricks, double *planar, int n_th, int n_td, int n_pd, int periodic_phi)
{
    const size_t plane = (size_t)n_th * n_td * n_pd;
    const size_t stride = (size_t)gridDim.x * kBlock;
    for (size_t t = (size_t)blockIdx.x * kBlock + threadIdx.x; t < plane; t += stride) {
        const int p = (int)(t % (size_t)n_pd);
        const int d = (int)((t / (size_t)n_pd) % (size_t)n_td);
        const int h = (int)(t / ((size_t)n_pd * n_td));
        double acc[3] = { 0.0, 0.0, 0.0 };
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
                    const double *b = bricks + ((size_t)(hc * n_td + dc) * n_pd + pc) * kBrickSlots + 3 * (4 * ho + 2 * dO + po);
                    acc[0] += b[0]; acc[1] += b[1]; acc[2] += b[2];
                }
            }
        }
        // a texel nothing reached keeps its bits (x + 0 would turn -0 into +0)
        if (acc[0] != 0.0) planar[t] += acc[0];
        if (acc[1] != 0.0) planar[plane + t] += acc[1];
        if (acc[2] != 0.0) planar[2 * plane + t] += acc[2];
    }
}

template <int LOOKUP, bool PER_LANE, bool INDEXED>
__device__ __forceinline__ void grad_naive(const GradArgs &a)
{
    GradShape shape = single_shape(a);
    fast::TableMaps maps(shape.n_th, shape.n_td, shape.n_pd, shape.param);
    const size_t stride = (size_t)gridDim.x * kBlock;
    const size_t n_items = grad_items<INDEXED>(a.n, a.idx_count);
    for (size_t j = (size_t)blockIdx.x * kBlock + threadIdx.x; j < n_items; j += stride) {
        const size_t i = INDEXED ? (size_t)a.idx[j] : j;
        unit_table<PER_LANE>(a, i, true, shape, maps);
        const GradUnit u = grad_unit<LOOKUP>(a, shape, maps, i, true);
        if (!u.live) continue;
        const size_t plane = (size_t)shape.n_th * shape.n_td * shape.n_pd;
        const bool periodic = param_phi_periodic(shape.param);
        double *planar = a.planar + 3 * (size_t)shape.cell_base;       // the target's own planar array
#pragma unroll
        for (int k = 0; k < (LOOKUP ? 8 : 1); ++k) {
            int h = u.cell.h0 + (k >> 2), d = u.cell.d0 + ((k >> 1) & 1), p = u.cell.p0 + (k & 1);
            h = h == shape.n_th ? shape.n_th - 1 : h;
            d = d == shape.n_td ? shape.n_td - 1 : d;
            p = p == shape.n_pd ? (periodic ? 0 : shape.n_pd - 1) : p;
            const size_t texel = ((size_t)h * shape.n_td + d) * shape.n_pd + p;
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) {
                const double v = (double)u.w[k] * u.s[ch];
                if (v != 0.0) add_f64(planar + ch * plane + texel, v);
            }
        }
    }
}

template <int LOOKUP>
__global__ __launch_bounds__(kBlock) void k_grad_naive(GradArgs a) { grad_naive<LOOKUP, false, false>(a); }
template <int LOOKUP, bool INDEXED>
__global__ __launch_bounds__(kBlock) void k_grad_naive_mat(GradArgs a) { grad_naive<LOOKUP, true, INDEXED>(a); }

unsigned grad_grid(size_t n, int compute_units) { return grid_blocks(n, kBlock, (size_t)compute_units * 8); }

// variant: MRL_OPT_TABLE_GRAD_KERNEL.  Bricks: adds the units' values into a.bricks (zeroed by the caller); naive: into a.planar.
// a.n_targets > 0: the launch with targets (a.mat / a.single_id name a unit's table; a.idx: over a queue of capacity a.n)
hipError_t launch_table_grad(GradArgs a, int variant, int compute_units, hipStream_t stream)
{
    if (a.n == 0) return hipSuccess;
    const dim3 grid(grad_grid(a.n, compute_units)), block(kBlock);
    const bool trilinear = a.opts.lookup != 0, indexed = a.idx != nullptr;
    a.merge = variant == 2 ? 1 : (variant == 3 ? 2 : 0);
    if (a.n_targets > 0) {
        with_flags([&](auto tri, auto idx) {
            if (variant == 1) hipLaunchKernelGGL((k_grad_naive_mat<tri ? 1 : 0, idx>), grid, block, 0, stream, a);
            else hipLaunchKernelGGL((k_grad_bricks_mat<tri ? 1 : 0, idx>), grid, block, 0, stream, a);
        }, trilinear, indexed);
        return hipGetLastError();
    }
    with_flags([&](auto tri) {
        if (variant == 1) hipLaunchKernelGGL(k_grad_naive<tri ? 1 : 0>, grid, block, 0, stream, a);
        else hipLaunchKernelGGL(k_grad_bricks<tri ? 1 : 0>, grid, block, 0, stream, a);
    }, trilinear);
    return hipGetLastError();
}

hipError_t launch_table_grad_fold(const double *bricks, double *planar, const int dims[3], int param, int compute_units, hipStream_t stream)
{
    const size_t plane = (size_t)dims[0] * dims[1] * dims[2];
    hipLaunchKernelGGL(k_grad_fold, dim3(grad_grid(plane, compute_units)), dim3(kBlock), 0, stream, bricks, planar, dims[0], dims[1], dims[2],
                       param_phi_periodic(param) ? 1 : 0);
    return hipGetLastError();
}

} // namespace

} // namespace mrl

using namespace mrlabi;

namespace {

// is `id` a table the adjoint is defined for?  MRL_OK, or the failure mrl_table_grad_batch documents
int check_grad_table(mrl_ctx *ctx, int32_t id)
{
    if (id < 0 || (size_t)id >= ctx->materials.size() || ctx->materials[(size_t)id].released) return fail(ctx, MRL_ERR_MATERIAL, "unknown material id");
    const MaterialHost &mh = ctx->materials[(size_t)id];
    if (mh.dev.kind != mrl::KIND_MERL && mh.dev.kind != mrl::KIND_TABLE)
        return fail(ctx, MRL_ERR_MATERIAL, "the table gradient is defined for RGB table materials (MERL / customized_measurement)");
    if (!mh.has_scale) return fail(ctx, MRL_ERR_MATERIAL, "a table restored from an image file does not carry its channel scales");
    return MRL_OK;
}

// Every table-gradient call: the checks, the workspace and the host-array path are grad_scatter_call's (merl_grad_scatter.hip).
// with_targets: mrl_table_grad_batch_mat / mrl_table_grad_queue (include/merl_hip_fit_table.h); without: mrl_table_grad_batch, whose
// one table c.target_ids[0] names — the kernels without target descriptors, and no bound on the cells beyond the table's own
int table_grad(mrl_ctx *ctx, const GradScatterCall &c, bool with_targets)
{
    if (!ctx) return MRL_ERR_INVALID;
    mrl::GradArgs a;
    std::memset(&a, 0, sizeof a);
    int variant = 0;
    return grad_scatter_call(ctx, c, {
        [&](int32_t id) { return check_grad_table(ctx, id); },
        [&](GradScatterLayout &lay) -> int {
            int dims[MRL_TABLE_GRAD_MAX_TARGETS][3];
            for (int k = 0; k < c.n_targets; ++k) {
                const MaterialHost &mh = ctx->materials[(size_t)c.target_ids[k]];
                mrl::GradTarget &t = a.targets[k];
                t.id = c.target_ids[k];
                dims[k][0] = t.n_th = mh.dev.n_th; dims[k][1] = t.n_td = mh.dev.n_td; dims[k][2] = t.n_pd = mh.dev.n_pd; t.param = mh.dev.param;
                t.scale[0] = mh.scale[0]; t.scale[1] = mh.scale[1]; t.scale[2] = mh.scale[2];
            }
            // where each target's bricks (cell_base records into the workspace) and planar array (3 cell_base doubles into out) start:
            // the one place that adds the cells up and bounds the int global cell index.  The single table starts at 0
            size_t offsets[MRL_TABLE_GRAD_MAX_TARGETS + 1] = { 0, 3 * (size_t)dims[0][0] * dims[0][1] * dims[0][2] };
            if (with_targets && mrl_table_grad_layout(&dims[0][0], c.n_targets, offsets) != MRL_OK)
                return fail(ctx, MRL_ERR_INVALID, "the targets have more than 2^31 - 1 cells in all");
            for (int k = 0; k < c.n_targets; ++k) a.targets[k].cell_base = (int)(offsets[k] / 3);
            const size_t cells = offsets[c.n_targets] / 3;
            if (with_targets) a.n_targets = c.n_targets;
            else {                                                   // the kernels without targets read the table from the arguments' head
                const mrl::GradTarget &t = a.targets[0];
                a.n_th = t.n_th; a.n_td = t.n_td; a.n_pd = t.n_pd; a.param = t.param;
                a.scale[0] = t.scale[0]; a.scale[1] = t.scale[1]; a.scale[2] = t.scale[2];
            }
            a.opts = ctx->opts;
            a.single_id = c.single_id;
            a.idx = c.queue; a.idx_count = c.queue_count;
            variant = ctx->table_grad_kernel;
            lay.brick_bytes = variant == 1 ? 0 : cells * mrl::kBrickSlots * sizeof(double);      // one 256-B record per table cell
            lay.out_doubles = 3 * cells;
            return MRL_OK;
        },
        true,
        [&](char *const *addr, size_t m, double *bricks, double *out) {
            a.wi = (const float *)addr[0]; a.wo = (const float *)addr[1]; a.g = (const float *)addr[2]; a.n = m;
            a.mat = c.mat ? (const int32_t *)addr[3] : nullptr;
            a.bricks = bricks; a.planar = out;
            return mrl::launch_table_grad(a, variant, ctx->compute_units, ctx->stream);
        },
        [&](const double *bricks, double *out) {
            hipError_t e = hipSuccess;
            for (int k = 0; k < c.n_targets && e == hipSuccess; ++k) {
                const mrl::GradTarget &t = a.targets[k];
                const int dims[3] = { t.n_th, t.n_td, t.n_pd };
                e = mrl::launch_table_grad_fold(bricks + (size_t)t.cell_base * mrl::kBrickSlots, out + 3 * (size_t)t.cell_base, dims, t.param,
                                                ctx->compute_units, ctx->stream);
            }
            return e;
        } });
}

} // namespace

extern "C" {

int mrl_table_grad_batch(mrl_ctx *ctx, const float *wi, const float *wo, const float *grad_rgb, int32_t id, size_t n, double *grad_planar)
{
    return table_grad(ctx, { wi, wo, grad_rgb, 12, "grad_rgb", nullptr, id, n, false, nullptr, nullptr, &id, 1, 1, grad_planar }, false);
}

int mrl_table_grad_layout(const int *dims, int n_targets, size_t *offsets_out)
{
    if (!dims || n_targets < 1 || n_targets > MRL_TABLE_GRAD_MAX_TARGETS) return MRL_ERR_INVALID;
    uint64_t cells = 0;                                   // three ints multiply to at most 2^93: checked factor by factor
    for (int k = 0; k < n_targets; ++k) {
        const int *d = dims + 3 * k;
        if (d[0] < 1 || d[1] < 1 || d[2] < 1) return MRL_ERR_INVALID;
        const uint64_t rows = (uint64_t)d[0] * (uint64_t)d[1];
        if (rows > (uint64_t)INT32_MAX) return MRL_ERR_INVALID;
        if (offsets_out) offsets_out[k] = (size_t)(3 * cells);
        cells += rows * (uint64_t)d[2];                   // at most 2^62 + 2^31
        if (cells > (uint64_t)INT32_MAX) return MRL_ERR_INVALID;
    }
    if (offsets_out) offsets_out[n_targets] = (size_t)(3 * cells);
    return MRL_OK;
}

int mrl_table_grad_batch_mat(mrl_ctx *ctx, const float *wi, const float *wo, const float *grad_rgb, const int32_t *mat, int32_t single_id, size_t n,
                             const int32_t *target_ids, int n_targets, double *grad_planar)
{
    return table_grad(ctx, { wi, wo, grad_rgb, 12, "grad_rgb", mat, single_id, n, false, nullptr, nullptr, target_ids, n_targets,
                             MRL_TABLE_GRAD_MAX_TARGETS, grad_planar }, true);
}

int mrl_table_grad_queue(mrl_ctx *ctx, const float *wi, const float *wo, const float *grad_rgb, const int32_t *mat, int32_t single_id,
                         const uint32_t *queue, const uint32_t *queue_count, size_t capacity, const int32_t *target_ids, int n_targets,
                         double *grad_planar)
{
    return table_grad(ctx, { wi, wo, grad_rgb, 12, "grad_rgb", mat, single_id, capacity, true, queue, queue_count, target_ids, n_targets,
                             MRL_TABLE_GRAD_MAX_TARGETS, grad_planar }, true);
}

} // extern "C"
