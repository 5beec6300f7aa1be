// merl_table_grad.hip — G += A^T g, the adjoint of eval on one RGB table material (include/merl_hip.h, mrl_table_grad_batch;
// DESIGN.md §5g).  The forward kernels gather; this one scatters, and its destinations collide where measured BRDFs are
// interesting.  The texels are never read: the call needs the material's dims, parameterisation and scale only, so one kernel
// serves both table layouts.
//   k_grad_bricks   one lane = one unit: the f64 coordinate transform of eval, the Float corner weights; the wave then transposes
//                   through LDS so that one wave-instruction carries the 24 values of two units (two contiguous 192-B segments of
//                   the gradient bricks) as f64 atomic adds.  Lanes of a wave that share a cell are summed first when many do.
//   k_grad_fold     per texel: the sum of the brick slots that map to it (clamp / wrap folding), added into the caller's planar array
//   k_grad_naive    the A/B baseline: each lane adds its 24 values straight into the planar array (64 lanes, 64 rows)
// Gradient brick of cell (h0, d0, p0): 32 doubles, slot 3 k + ch for corner k = 4 a + 2 b + c (corner_weights' order), 24 used.
#include "merl_ctx.hpp"
#include "merl_table_fast.hpp"

namespace mrl {

namespace {

constexpr int kBlock = 256;
constexpr int kBrickSlots = 32;          // doubles per gradient brick (256 B)
constexpr int kMergeMin = 4;             // merge a wave's lanes by cell when at least this many share the first live lane's cell

struct GradArgs {
    const float *wi, *wo, *g;
    size_t n;
    int n_th, n_td, n_pd, param;
    Options opts;
    double scale[3];
    double *bricks;                      // [cells][kBrickSlots]
    double *planar;                      // k_grad_naive: [3][n_th][n_td][n_pd]
    int merge;                           // 0: wave-uniform choice, 1: never, 2: always
};

// f64 add without a compare-and-swap loop (global_atomic_add_f64 / flat_atomic_add_f64); the destinations are device allocations
__device__ __forceinline__ void add_f64(double *p, double v) { (void)unsafeAtomicAdd(p, v); }

// What unit i adds: the cell of its lookup (eval's own TableCell, kept inside the table; the kernels read its indices only), whether
// eval masks the unit, the Float corner weights and, per channel, scale x (cos(theta_o) or 1) x g in f64.  Masking is a select: a dead unit's g may be NaN.
struct GradUnit {
    TableCell cell;
    bool live;
    float w[8];
    double s[3];
};

template <int LOOKUP>
__device__ __forceinline__ GradUnit grad_unit(const GradArgs &a, const fast::TableMaps &maps, size_t i)
{
#pragma clang fp contract(off)
    float wix = 0.0f, wiy = 0.0f, wiz = 0.0f, wox = 0.0f, woy = 0.0f, woz = 0.0f, g0 = 0.0f, g1 = 0.0f, g2 = 0.0f;
    const bool in_range = i < a.n;
    if (in_range) {
        load3(a.wi, i, wix, wiy, wiz);
        load3(a.wo, i, wox, woy, woz);
        load3(a.g, i, g0, g1, g2);
    }
    // the factor eval_tail multiplies by: Float wo.z (or 1), NaN when a component of either direction is not finite
    const float c32 = fast::cos_or_nan32((wix + wiy + wiz), wox, woy, woz, a.opts.cosine != 0);
    GradUnit u;
    u.live = in_range && (wiz > 0.0f) && (woz > 0.0f) && (c32 == c32);
    const fast::Vec3 in = fast::normalize_f32(wix, wiy, wiz);
    const Coords c = maps(in, fast::dir_f32(wox, woy, woz));
    // eval's own cell and weights (a nearest lookup: all weight on corner 0)
    u.cell = LOOKUP ? trilinear_cell(c, a.n_th, a.n_td, a.n_pd, a.opts.node, a.param) : nearest_cell(c, a.n_th, a.n_td, a.n_pd);
    const CornerWeights cw = corner_weights(u.cell.fh, u.cell.fd, u.cell.fp);
#pragma unroll
    for (int k = 0; k < 8; ++k) u.w[k] = u.live ? cw.w[k] : 0.0f;
    // a dead unit's coordinates are garbage: whatever they are, the cell stays inside the table (nearest_cell's already does)
    if constexpr (LOOKUP) {
        u.cell.h0 = clampi(u.cell.h0, 0, a.n_th - 1); u.cell.d0 = clampi(u.cell.d0, 0, a.n_td - 1); u.cell.p0 = clampi(u.cell.p0, 0, a.n_pd - 1);
    }
    const double cd = (double)c32;
    u.s[0] = u.live ? a.scale[0] * cd * (double)g0 : 0.0;
    u.s[1] = u.live ? a.scale[1] * cd * (double)g1 : 0.0;
    u.s[2] = u.live ? a.scale[2] * cd * (double)g2 : 0.0;
    return u;
}

template <int LOOKUP>
__global__ __launch_bounds__(kBlock) void k_grad_bricks(GradArgs a)
{
    // what the lanes of a wave hand to each other: k-major, so that 64 lanes write 64 consecutive words.  The transposed reads take
    // one unit's values for all k (s_w[k][m]) and all channels (s_s[ch][m]) in one instruction: the rows are padded by one element so
    // that those land on different LDS banks (a row stride of kBlock words would put all eight k on one bank)
    __shared__ int s_cell[kBlock];
    __shared__ float s_w[8][kBlock + 1];
    __shared__ double s_s[3][kBlock + 1];
    const fast::TableMaps maps(a.n_th, a.n_td, a.n_pd, a.param);
    const unsigned t = threadIdx.x, lane = t & 63u, wbase = t & ~63u;
    const unsigned sub = lane >> 5, slot = lane & 31u;           // two units per wave-instruction, 32 slots each (24 used)
    const unsigned k = slot / 3u, ch = slot - 3u * k;
    const bool slot_on = slot < (LOOKUP ? 24u : 3u);             // a nearest lookup has corner 0 only
    const unsigned kk = slot_on ? k : 0u, cc = slot_on ? ch : 0u;
    const size_t stride = (size_t)gridDim.x * kBlock;
    const size_t rounds = (a.n + stride - 1) / stride;           // the same trip count for every thread: barriers inside
    for (size_t r = 0; r < rounds; ++r) {
        const size_t i = r * stride + (size_t)blockIdx.x * kBlock + t;
        const GradUnit u = grad_unit<LOOKUP>(a, maps, i);
        const int cell = u.live ? cell_index<int>(u.cell, a.n_td, a.n_pd) : -1;
        s_cell[t] = cell;
#pragma unroll
        for (int q = 0; q < (LOOKUP ? 8 : 1); ++q) s_w[q][t] = u.w[q];
        s_s[0][t] = u.s[0]; s_s[1][t] = u.s[1]; s_s[2][t] = u.s[2];
        __syncthreads();
        const uint64_t live = __ballot(cell >= 0);
        if (live != 0ull) {                                      // wave-uniform from here on
            bool merged = a.merge == 2;
            if (a.merge == 0) {
                const int c0 = s_cell[wbase + (unsigned)__builtin_ctzll(live)];
                merged = __popcll(__ballot(cell == c0)) >= kMergeMin;
            }
            if (!merged) {
                for (unsigned j = 0; j < 64u; j += 2u) {
                    if (((live >> j) & 3ull) == 0ull) continue;
                    const unsigned m = wbase + j + sub;
                    const int cm = s_cell[m];
                    if (slot_on && cm >= 0) add_f64(a.bricks + (size_t)cm * kBrickSlots + slot, (double)s_w[kk][m] * s_s[cc][m]);
                }
            } else {
                // leader loop: the lanes that hold the first remaining lane's cell are summed by the 24 slot lanes of each half
                // (low half: members among lanes 0..31, high half: among 32..63), one atomic per slot and half
                uint64_t rem = live;
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
                            acc = __builtin_fma((double)s_w[kk][m], s_s[cc][m], acc);
                        }
                        add_f64(a.bricks + (size_t)c0 * kBrickSlots + slot, acc);
                    }
                }
            }
        }
        __syncthreads();
    }
}

// the brick slots that reach texel i of an axis of n texels: source s = 0: cell i, corner offset 0; 1: cell i - 1, offset 1;
// 2: the folded corner index n — cell n - 1, offset 1 — onto texel n - 1 (clamped axis) or texel 0 (periodic axis)
__device__ __forceinline__ bool fold_source(int s, int i, int n, bool periodic, int &cell, int &off)
{
    cell = s == 0 ? i : (s == 1 ? i - 1 : n - 1);
    off = s == 0 ? 0 : 1;
    return s == 0 ? true : (s == 1 ? i >= 1 : (periodic ? i == 0 : i == n - 1));
}

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

template <int LOOKUP>
__global__ __launch_bounds__(kBlock) void k_grad_naive(GradArgs a)
{
    const fast::TableMaps maps(a.n_th, a.n_td, a.n_pd, a.param);
    const size_t plane = (size_t)a.n_th * a.n_td * a.n_pd;
    const bool periodic = param_phi_periodic(a.param);
    const size_t stride = (size_t)gridDim.x * kBlock;
    for (size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x; i < a.n; i += stride) {
        const GradUnit u = grad_unit<LOOKUP>(a, maps, i);
        if (!u.live) continue;
#pragma unroll
        for (int k = 0; k < (LOOKUP ? 8 : 1); ++k) {
            int h = u.cell.h0 + (k >> 2), d = u.cell.d0 + ((k >> 1) & 1), p = u.cell.p0 + (k & 1);
            h = h == a.n_th ? a.n_th - 1 : h;
            d = d == a.n_td ? a.n_td - 1 : d;
            p = p == a.n_pd ? (periodic ? 0 : a.n_pd - 1) : p;
            const size_t texel = ((size_t)h * a.n_td + d) * a.n_pd + p;
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) {
                const double v = (double)u.w[k] * u.s[ch];
                if (v != 0.0) add_f64(a.planar + ch * plane + texel, v);
            }
        }
    }
}

unsigned grad_grid(size_t n, int compute_units) { return grid_blocks(n, kBlock, (size_t)compute_units * 8); }

// variant: MRL_OPT_TABLE_GRAD_KERNEL.  Bricks: adds the units' values into a.bricks (zeroed by the caller); naive: into a.planar
hipError_t launch_table_grad(GradArgs a, int variant, int compute_units, hipStream_t stream)
{
    if (a.n == 0) return hipSuccess;
    const dim3 grid(grad_grid(a.n, compute_units)), block(kBlock);
    if (variant == 1) {
        with_flags([&](auto trilinear) { hipLaunchKernelGGL(k_grad_naive<trilinear ? 1 : 0>, grid, block, 0, stream, a); }, a.opts.lookup != 0);
        return hipGetLastError();
    }
    a.merge = variant == 2 ? 1 : (variant == 3 ? 2 : 0);
    with_flags([&](auto trilinear) { hipLaunchKernelGGL(k_grad_bricks<trilinear ? 1 : 0>, grid, block, 0, stream, a); }, a.opts.lookup != 0);
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

extern "C" {

int mrl_table_grad_batch(mrl_ctx *ctx, const float *wi, const float *wo, const float *grad_rgb, int32_t id, size_t n, double *grad_planar)
{
    if (!ctx) return MRL_ERR_INVALID;
    MRL_GUARD(ctx);
    if (n == 0) return MRL_OK;
    const StreamList streams = { { (void *)wi, 12, false, "wi" }, { (void *)wo, 12, false, "wo" }, { (void *)grad_rgb, 12, false, "grad_rgb" } };
    if (first_null(streams) || !grad_planar) return fail(ctx, MRL_ERR_INVALID, "null array argument");
    if (id < 0 || (size_t)id >= ctx->materials.size() || ctx->materials[(size_t)id].released) return fail(ctx, MRL_ERR_MATERIAL, "unknown material id");
    const MaterialHost &mh = ctx->materials[(size_t)id];
    if (mh.dev.kind != mrl::KIND_MERL && mh.dev.kind != mrl::KIND_TABLE)
        return fail(ctx, MRL_ERR_MATERIAL, "the table gradient is defined for RGB table materials (MERL / customized_measurement)");
    if (!mh.has_scale) return fail(ctx, MRL_ERR_MATERIAL, "a table restored from an image file does not carry its channel scales");
    if (ctx->opts.negative == mrl::NEGATIVE_RENORMALISE)
        return fail(ctx, MRL_ERR_INVALID, "MRL_OPT_NEGATIVE = renormalise makes eval non-linear in the table: no adjoint");
    MRL_HIP(ctx, hipSetDevice(ctx->device));
    const int kind = common_kind({ grad_planar }, streams);
    if (kind < 0) return fail(ctx, MRL_ERR_POINTER_MIX, "host and device pointers mixed in one call");

    const int dims[3] = { mh.dev.n_th, mh.dev.n_td, mh.dev.n_pd };
    const size_t plane = (size_t)dims[0] * dims[1] * dims[2];
    const int variant = ctx->table_grad_kernel;
    mrl::GradArgs a;
    std::memset(&a, 0, sizeof a);
    a.n_th = dims[0]; a.n_td = dims[1]; a.n_pd = dims[2]; a.param = mh.dev.param;
    a.opts = ctx->opts;
    a.scale[0] = mh.scale[0]; a.scale[1] = mh.scale[1]; a.scale[2] = mh.scale[2];
    if (variant != 1) {
        DeviceBuf &bricks = ctx->buf[mrl_ctx::BUF_GRAD_BRICKS];      // one 256-B record per table cell; grown on demand, reused
        const int rc = bricks.reserve(ctx, plane * mrl::kBrickSlots * sizeof(double));
        if (rc != MRL_OK) return rc;
        a.bricks = (double *)bricks.p;
        MRL_HIP(ctx, hipMemsetAsync(a.bricks, 0, plane * mrl::kBrickSlots * sizeof(double), ctx->stream));
    }
    if (kind == 1) {
        a.wi = wi; a.wo = wo; a.g = grad_rgb; a.n = n; a.planar = grad_planar;
        MRL_HIP(ctx, mrl::launch_table_grad(a, variant, ctx->compute_units, ctx->stream));
        if (variant != 1) MRL_HIP(ctx, mrl::launch_table_grad_fold(a.bricks, grad_planar, dims, a.param, ctx->compute_units, ctx->stream));
        return MRL_OK;
    }
    // host arrays: the inputs are staged chunk by chunk, the sums gathered in a device array and added to the caller's on the host
    double *d_planar = nullptr;
    MRL_ALLOC(ctx, hipMalloc((void **)&d_planar, 3 * plane * sizeof(double)));
    auto run = [&]() -> int {
        MRL_HIP(ctx, hipMemsetAsync(d_planar, 0, 3 * plane * sizeof(double), ctx->stream));
        a.planar = d_planar;
        const int rc = run_host_staged(ctx, streams, n, 0, [&](char *const *addr, size_t m) -> int {
            a.wi = (const float *)addr[0]; a.wo = (const float *)addr[1]; a.g = (const float *)addr[2]; a.n = m;
            MRL_HIP(ctx, mrl::launch_table_grad(a, variant, ctx->compute_units, ctx->stream));
            return MRL_OK;
        });
        if (rc != MRL_OK) return rc;
        if (variant != 1) MRL_HIP(ctx, mrl::launch_table_grad_fold(a.bricks, d_planar, dims, a.param, ctx->compute_units, ctx->stream));
        std::vector<double> sums;
        try { sums.resize(3 * plane); } catch (const std::bad_alloc &) { return fail(ctx, MRL_ERR_OOM, "gradient buffer"); }
        MRL_HIP(ctx, hipMemcpyAsync(sums.data(), d_planar, 3 * plane * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
        MRL_HIP(ctx, hipStreamSynchronize(ctx->stream));
        for (size_t t = 0; t < 3 * plane; ++t)
            if (sums[t] != 0.0) grad_planar[t] += sums[t];
        return MRL_OK;
    };
    const int rc = run();
    if (rc != MRL_OK) (void)hipStreamSynchronize(ctx->stream);
    (void)hipFree(d_planar);
    return rc;
}

} // extern "C"
