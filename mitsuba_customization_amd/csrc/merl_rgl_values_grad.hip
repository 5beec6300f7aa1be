// merl_rgl_values_grad.hip — G += (d eval / d R)^T g, the adjoint of eval in the measured values of RGB RGL materials, onto up to 16
// target materials in one launch, with a material id per unit or over a wavefront queue; and new values for a resident RGL material
// in place (include/merl_hip_fit_rgl.h).  The RGL twin of merl_table_grad.hip: eval gathers, this scatters.
//   k_rgl_values_bricks<MULTI, INDEXED, MASK>  one lane = one unit: rgl::values_grad_unit (merl_rgl_values_grad.hpp) — eval's own
//                       lookup, the clamp mask from the value cell, the three factors of the unit's terms; the wave then transposes
//                       through LDS so that one wave-instruction carries whole gradient bricks (16 S doubles: four units for S = 1,
//                       two for S = 2, one for S = 4) as f64 atomic adds.  Lanes of a wave that share a brick are summed first when
//                       at least kMergeMin share the first live lane's (§5g's wave-uniform rule; wave_merge_rule / wave_scatter of
//                       merl_grad_scatter.hpp, which every adjoint's kernel runs).
//   k_rgl_values_fold   per planar texel: the sum of the brick slots that map to it (rgl::fold_sources, a fixed order), added into
//                       the caller's array when it is not zero
//   k_rgl_values_plain<MULTI, INDEXED>  the measured baseline: each lane adds its 12 S terms straight into the planar array
//   k_rgl_values_write  the update: one thread per float4 of the bracket-major value bricks reads its four nodes from the planar array
// !MULTI: the launch's one material, its descriptor by value in the kernel arguments and the kernel compiled for its bracket shape
// (MASK 1 / 3 / 5 / 15).  MULTI: a unit's id is compared with the (id, workspace base) pairs of the kernel arguments and the RglDev is
// read whole from behind the target's image, as rgl_walk_ids of merl_rgl.hip reads it; MASK 0, the shape tested at run time, one
// brick per wave-instruction.  Which instantiation a call launches is route_values_grad below; launch_values_grad names what it can
// reach and nothing else.
#include "merl_ctx.hpp"
#include "../../include/merl_hip_fit_rgl.h"
#include "merl_rgl_values_grad.hpp"
#include "merl_grad_scatter.hpp"

namespace mrl {

namespace {

constexpr int kVgBlock = 256;
constexpr int kVgMaxTargets = MRL_RGL_GRAD_MAX_TARGETS;

// One target of a launch: by value in the kernel arguments (a queue call copies nothing from host memory at call time).  40 B
struct ValuesTarget {
    int id;                              // the material id a unit must carry
    int slices;                          // S of its brackets
    int record_base;                     // bricks of the targets before it: what two lanes compare before they are summed together
    const RglDev *dev;                   // the descriptor stored behind the material's image
    unsigned long long brick_base;       // its first brick in the workspace, in doubles
    unsigned long long planar_base;      // its slice of the caller's array, in doubles
};

struct ValuesGradArgs {
    const float *wi, *wo, *g;
    size_t n;                            // units; of a queue launch the queue's capacity
    const int32_t *mat;                  // MULTI: a unit's material id
    const uint32_t *idx, *idx_count;     // INDEXED: the units idx[0 .. min(*idx_count, n))
    double *bricks, *planar;
    int merge;                           // 0: wave-uniform choice, 1: never, 2: always
    int n_targets;
    ValuesTarget targets[kVgMaxTargets]; // !MULTI: targets[0] is the launch's material
};

// unit i of the launch: its target (by value) and its factors; a unit out of range, of another material or dead is !live
template <bool MULTI, int MASK>
__device__ __forceinline__ rgl::ValuesGradUnit vg_unit(const ValuesGradArgs &a, const RglDev &r, size_t i, bool in_range, ValuesTarget &t)
{
    float wix = 0.0f, wiy = 0.0f, wiz = 0.0f, wox = 0.0f, woy = 0.0f, woz = 0.0f, g32[3] = { 0.0f, 0.0f, 0.0f };
    if (in_range) {
        load3(a.wi, i, wix, wiy, wiz);
        load3(a.wo, i, wox, woy, woz);
        load3(a.g, i, g32[0], g32[1], g32[2]);
    }
    t = a.targets[0];
    if constexpr (MULTI) {
        const int id = in_range ? a.mat[i] : -1;
        bool known = false;
        for (int k = 0; k < a.n_targets; ++k) {                  // a wave-uniform trip count, scalar loads
            const ValuesTarget &c = a.targets[k];
            const bool hit = in_range && c.id == id;
            t.slices = hit ? c.slices : t.slices; t.record_base = hit ? c.record_base : t.record_base; t.dev = hit ? c.dev : t.dev;
            t.brick_base = hit ? c.brick_base : t.brick_base; t.planar_base = hit ? c.planar_base : t.planar_base;
            known = known || hit;
        }
        if (!known) return rgl::ValuesGradUnit{};
        // the unit's descriptor into registers, whole: through a reference every table read would be two dependent loads
        const RglDev rm = *t.dev;
        return rgl::values_grad_unit<0>(rm, rgl::GridMem{ rm.phi, rm.theta, rm.wavelengths }, wix, wiy, wiz, wox, woy, woz, g32);
    } else {
        if (!in_range) return rgl::ValuesGradUnit{};
        return rgl::values_grad_unit<MASK>(r, rgl::GridMem{ r.phi, r.theta, r.wavelengths }, wix, wiy, wiz, wox, woy, woz, g32);
    }
}

constexpr int mask_slices(int mask) { return (mask & 1) + ((mask >> 1) & 1) + ((mask >> 2) & 1) + ((mask >> 3) & 1); }

template <bool MULTI, bool INDEXED, int MASK>
__global__ __launch_bounds__(kVgBlock, 2) void k_rgl_values_bricks(ValuesGradArgs a, RglDev r)
{
#pragma clang fp contract(off)
    // what the lanes of a wave hand to each other, factor-major: 64 lanes write 64 consecutive words, and a transposed read takes one
    // unit's factors for all slots in one instruction — the rows are padded by one element so that those land on different LDS banks
    __shared__ int s_key[kVgBlock];
    __shared__ int s_slices[kVgBlock];
    __shared__ unsigned long long s_off[kVgBlock];
    __shared__ double s_f[11][kVgBlock + 1];                    // a[3], ws[4], wc[4]
    // lanes per brick: the launch's own shape, or 64 where shapes mix
    constexpr unsigned L = MULTI ? 64u : 16u * (unsigned)mask_slices(MASK);
    const unsigned t = threadIdx.x, lane = t & 63u, wbase = t & ~63u;
    const unsigned slot = lane % L;
    const size_t stride = (size_t)gridDim.x * kVgBlock;
    const size_t n_items = grad_items<INDEXED>(a.n, a.idx_count);
    const size_t rounds = (n_items + stride - 1) / stride;       // the same trip count for every thread: barriers inside
    for (size_t rd = 0; rd < rounds; ++rd) {
        const size_t j0 = rd * stride + (size_t)blockIdx.x * kVgBlock + t;
        const bool in_range = j0 < n_items;
        size_t i = j0;
        if constexpr (INDEXED) i = in_range ? (size_t)a.idx[j0] : 0;
        ValuesTarget tg;
        const rgl::ValuesGradUnit u = vg_unit<MULTI, MASK>(a, r, i, in_range, tg);
        const int key = u.live ? tg.record_base + (int)u.record : -1;
        s_key[t] = key;
        s_slices[t] = u.live ? u.slices : 1;
        s_off[t] = tg.brick_base + (unsigned long long)u.record * (unsigned long long)(16 * u.slices);
#pragma unroll
        for (int q = 0; q < 3; ++q) s_f[q][t] = u.a[q];
#pragma unroll
        for (int q = 0; q < 4; ++q) { s_f[3 + q][t] = u.ws[q]; s_f[7 + q][t] = u.wc[q]; }
        __syncthreads();
        // slot -> (channel, slice, corner) of unit m's brick, and the product of its factors
        auto term = [&](unsigned m, int S) {
            const int lg = S >> 1;                               // log2 of 1 / 2 / 4
            const int jj = (int)(slot & 3u), kk = (int)(slot >> 2) & (S - 1), cc = (int)(slot >> 2) >> lg;
            return s_f[cc][m] * s_f[3 + kk][m] * s_f[7 + jj][m];
        };
        const uint64_t live = __ballot(key >= 0);
        // lanes of a wave that share a brick are summed first when many do: a brick's S is that of any of its units
        wave_scatter<L>(live, wave_merge_rule(a.merge, key, s_key, wbase, live), key, s_key, wbase, lane,
            [&](unsigned ref) { return slot < 12u * (unsigned)s_slices[ref]; },
            [&](unsigned m, unsigned ref) { return term(m, s_slices[ref]); },
            [&](double acc, unsigned m, unsigned ref) { return acc + term(m, s_slices[ref]); },
            [&](unsigned ref) { return a.bricks + s_off[ref] + slot; });
        __syncthreads();
    }
}

template <bool MULTI, bool INDEXED>
__global__ __launch_bounds__(kVgBlock, 2) void k_rgl_values_plain(ValuesGradArgs a, RglDev r)
{
#pragma clang fp contract(off)
    const size_t stride = (size_t)gridDim.x * kVgBlock;
    const size_t n_items = grad_items<INDEXED>(a.n, a.idx_count);
    for (size_t j0 = (size_t)blockIdx.x * kVgBlock + threadIdx.x; j0 < n_items; j0 += stride) {
        const size_t i = INDEXED ? (size_t)a.idx[j0] : j0;
        ValuesTarget tg;
        const rgl::ValuesGradUnit u = vg_unit<MULTI, 0>(a, r, i, true, tg);
        if (!u.live) continue;
        RglDev shape = r;                                        // n_phi, n_theta, nx, ny of the unit's material
        if constexpr (MULTI) { const RglDev rm = *tg.dev; shape = rm; }
        double *planar = a.planar + tg.planar_base;
#pragma unroll
        for (int c = 0; c < 3; ++c)
#pragma unroll
            for (int k = 0; k < 4; ++k)
#pragma unroll
                for (int jj = 0; jj < 4; ++jj) {
                    const double v = u.a[c] * u.ws[k] * u.wc[jj];
                    if (k < u.slices && v != 0.0) add_f64(planar + rgl::values_texel(shape, u, c, k, jj), v);
                }
    }
}

__global__ __launch_bounds__(kVgBlock) void k_rgl_values_fold(const double *bricks, double *planar, int n_phi, int n_theta, int nx, int ny)
{
    const size_t texels = (size_t)n_phi * n_theta * 3 * (size_t)ny * (size_t)nx;
    const size_t stride = (size_t)gridDim.x * kVgBlock;
    for (size_t t = (size_t)blockIdx.x * kVgBlock + threadIdx.x; t < texels; t += stride) {
        const int x = (int)(t % (size_t)nx), y = (int)((t / (size_t)nx) % (size_t)ny), c = (int)((t / ((size_t)nx * ny)) % 3);
        const size_t slice = t / ((size_t)nx * ny * 3);
        const int it = (int)(slice % (size_t)n_theta), ip = (int)(slice / (size_t)n_theta);
        size_t src[16];
        const int n = rgl::fold_sources(n_phi, n_theta, nx, ny, ip, it, c, y, x, src);
        double acc = 0.0;
        for (int k = 0; k < n; ++k) acc += bricks[src[k]];
        // a texel nothing reached keeps its bits (x + 0 would turn -0 into +0)
        if (acc != 0.0) planar[t] += acc;
    }
}

// The device twin of the value branch of append_warp (merl_rgl.hip): float4 f of the value bricks [bracket][cell][channel][slice]
// is the four nodes (y, x) (y, x + 1) (y + 1, x) (y + 1, x + 1) of its slice and channel in src [n_phi][n_theta][3][ny][nx].  No arithmetic.
__global__ __launch_bounds__(kVgBlock) void k_rgl_values_write(const float *__restrict__ src, float4 *__restrict__ cells, int n_phi, int n_theta, int nx, int ny)
{
    const int tb = n_theta > 1 ? n_theta - 1 : 1, pb = n_phi > 1 ? n_phi - 1 : 1;
    const int S = (n_phi > 1 ? 2 : 1) * (n_theta > 1 ? 2 : 1);
    const size_t per_c = (size_t)(nx - 1) * (size_t)(ny - 1), total = (size_t)pb * tb * per_c * 3 * (size_t)S;
    const size_t stride = (size_t)gridDim.x * kVgBlock;
    for (size_t f = (size_t)blockIdx.x * kVgBlock + threadIdx.x; f < total; f += stride) {
        const int slot = (int)(f % (size_t)S), ch = (int)((f / (size_t)S) % 3);
        const size_t cell = (f / (size_t)(3 * S)) % per_c, br = f / ((size_t)(3 * S) * per_c);
        const int ipb = (int)(br / (size_t)tb), itb = (int)(br % (size_t)tb);
        const int dp = n_phi > 1 ? (slot & 1) : 0, dt = n_phi > 1 ? (slot >> 1) : slot;
        const size_t slice = (size_t)(ipb + dp) * n_theta + (size_t)(itb + dt);
        const size_t y = cell / (size_t)(nx - 1), x = cell % (size_t)(nx - 1);
        const float *p = src + ((slice * 3 + (size_t)ch) * (size_t)ny + y) * (size_t)nx + x;
        cells[f] = make_float4(p[0], p[1], p[nx], p[nx + 1]);
    }
}

// ---- which instantiation a launch takes: pure arithmetic (route_rgl's style), then the one place that names the kernels ----
struct ValuesGradChoice {
    bool plain;         // MRL_OPT_TABLE_GRAD_KERNEL = 1
    bool multi;         // a material id per unit
    bool indexed;       // over a queue
    int mask;           // the bracket shape the kernel is compiled for; 0: tested at run time (multi, and the plain form)
    int merge;          // bricks: 0 wave-uniform, 1 never, 2 always
};
ValuesGradChoice route_values_grad(int variant, bool multi, bool indexed, int n_phi, int n_theta)
{
    const bool plain = variant == 1;
    const int mask = multi || plain ? 0 : 1 | (n_phi > 1 ? 2 : 0) | (n_theta > 1 ? 4 : 0) | (n_phi > 1 && n_theta > 1 ? 8 : 0);
    return { plain, multi, indexed, mask, variant == 2 ? 1 : (variant == 3 ? 2 : 0) };
}

unsigned vg_grid(size_t n, int compute_units) { return grid_blocks(n, kVgBlock, (size_t)std::max(compute_units, 1) * 2); }

hipError_t launch_values_grad(const ValuesGradChoice &k, ValuesGradArgs a, const RglDev &r, int compute_units, hipStream_t stream)
{
    if (a.n == 0) return hipSuccess;
    const dim3 grid(vg_grid(a.n, compute_units)), block(kVgBlock);
    a.merge = k.merge;
    with_flags([&](auto ix) {
        if (k.plain) {
            if (k.multi) hipLaunchKernelGGL((k_rgl_values_plain<true, ix>), grid, block, 0, stream, a, r);
            else hipLaunchKernelGGL((k_rgl_values_plain<false, ix>), grid, block, 0, stream, a, r);
            return;
        }
        switch (k.mask) {
        case 0:  hipLaunchKernelGGL((k_rgl_values_bricks<true, ix, 0>), grid, block, 0, stream, a, r); break;
        case 1:  hipLaunchKernelGGL((k_rgl_values_bricks<false, ix, 1>), grid, block, 0, stream, a, r); break;
        case 3:  hipLaunchKernelGGL((k_rgl_values_bricks<false, ix, 3>), grid, block, 0, stream, a, r); break;
        case 5:  hipLaunchKernelGGL((k_rgl_values_bricks<false, ix, 5>), grid, block, 0, stream, a, r); break;
        default: hipLaunchKernelGGL((k_rgl_values_bricks<false, ix, 15>), grid, block, 0, stream, a, r); break;
        }
    }, k.indexed);
    return hipGetLastError();
}

hipError_t launch_values_fold(const double *bricks, double *planar, const int shape[5], int compute_units, hipStream_t stream)
{
    const size_t texels = (size_t)shape[0] * shape[1] * 3 * (size_t)shape[3] * (size_t)shape[4];
    hipLaunchKernelGGL(k_rgl_values_fold, dim3(grid_blocks(texels, kVgBlock, (size_t)std::max(compute_units, 1) * 8)), dim3(kVgBlock), 0, stream,
                       bricks, planar, shape[0], shape[1], shape[4], shape[3]);
    return hipGetLastError();
}

hipError_t launch_values_write(const float *src, float4 *cells, const RglDev &r, int compute_units, hipStream_t stream)
{
    const size_t total = rgl::values_records(r.n_phi, r.n_theta, r.nx, r.ny) * 3 * (size_t)r.slices();
    hipLaunchKernelGGL(k_rgl_values_write, dim3(grid_blocks(total, kVgBlock, (size_t)std::max(compute_units, 1) * 8)), dim3(kVgBlock), 0, stream,
                       src, cells, r.n_phi, r.n_theta, r.nx, r.ny);
    return hipGetLastError();
}

} // namespace

} // namespace mrl

using namespace mrlabi;

namespace {

bool live_id(const mrl_ctx *ctx, int id) { return id >= 0 && (size_t)id < ctx->materials.size() && !ctx->materials[(size_t)id].released; }

// the planar shape of a material's values: n_phi, n_theta, 3, ny, nx
void shape_of(const mrl::RglDev &r, int shape[5]) { shape[0] = r.n_phi; shape[1] = r.n_theta; shape[2] = 3; shape[3] = r.ny; shape[4] = r.nx; }

struct ValuesLayout { size_t records, brick_doubles; };       // over all targets
// per target: bricks before it (records), its first brick and its planar slice (doubles).  False: what the layout function refuses
bool values_layout(const int *shapes, int n_targets, size_t *planar_off, size_t *record_base, size_t *brick_base, ValuesLayout *all)
{
    if (!shapes || n_targets < 1 || n_targets > MRL_RGL_GRAD_MAX_TARGETS) return false;
    uint64_t records = 0, bricks = 0, planar = 0;
    for (int k = 0; k < n_targets; ++k) {
        const int *s = shapes + 5 * k;
        if (s[0] < 1 || s[1] < 1 || s[2] != 3 || s[3] < 2 || s[4] < 2) return false;
        // four ints multiply to at most 2^124: checked pair by pair; slices x per is then at most 16 records
        const uint64_t brackets = (uint64_t)(s[0] > 1 ? s[0] - 1 : 1) * (uint64_t)(s[1] > 1 ? s[1] - 1 : 1), cells = (uint64_t)(s[3] - 1) * (uint64_t)(s[4] - 1);
        if (brackets > (uint64_t)INT32_MAX || cells > (uint64_t)INT32_MAX) return false;
        const uint64_t rec = brackets * cells;
        if (rec > (uint64_t)INT32_MAX) return false;
        const uint64_t slices = (uint64_t)s[0] * (uint64_t)s[1], per = (uint64_t)s[3] * (uint64_t)s[4];
        const int S = (s[0] > 1 ? 2 : 1) * (s[1] > 1 ? 2 : 1);
        if (planar_off) planar_off[k] = (size_t)planar;
        if (record_base) record_base[k] = (size_t)records;
        if (brick_base) brick_base[k] = (size_t)bricks;
        records += rec;
        if (records > (uint64_t)INT32_MAX) return false;
        bricks += rec * (uint64_t)(16 * S);
        planar += 3 * slices * per;                              // at most 48 x 2^31 per target
    }
    if (planar_off) planar_off[n_targets] = (size_t)planar;
    if (all) { all->records = (size_t)records; all->brick_doubles = (size_t)bricks; }
    return true;
}

// mrl_rgl_values_grad_batch / mrl_rgl_values_grad_queue: the checks, the workspace and the host-array path are grad_scatter_call's
// (merl_grad_scatter.hip)
int rgl_values_grad(mrl_ctx *ctx, const GradScatterCall &c)
{
    if (!ctx) return MRL_ERR_INVALID;
    mrl::ValuesGradArgs a;
    std::memset(&a, 0, sizeof a);
    int shapes[MRL_RGL_GRAD_MAX_TARGETS][5];
    size_t planar_off[MRL_RGL_GRAD_MAX_TARGETS + 1], record_base[MRL_RGL_GRAD_MAX_TARGETS], brick_base[MRL_RGL_GRAD_MAX_TARGETS];
    mrl::RglDev single{};                                        // a call without ids: its one material, by value
    mrl::ValuesGradChoice choice{};
    return grad_scatter_call(ctx, c, {
        [&](int32_t id) {
            if (!live_id(ctx, id) || ctx->materials[(size_t)id].dev.kind != mrl::KIND_RGL)
                return fail(ctx, MRL_ERR_MATERIAL, "a target is not a live RGB RGL material (mrl_material_upload_rgl / mrl_material_load_rgl)");
            return (int)MRL_OK;
        },
        [&](GradScatterLayout &lay) -> int {
            for (int k = 0; k < c.n_targets; ++k) shape_of(ctx->materials[(size_t)c.target_ids[k]].rgl, shapes[k]);
            ValuesLayout all;
            if (!values_layout(&shapes[0][0], c.n_targets, planar_off, record_base, brick_base, &all))
                return fail(ctx, MRL_ERR_INVALID, "the targets have more than 2^31 - 1 workspace records in all");
            a.idx = c.queue; a.idx_count = c.queue_count;
            a.n_targets = c.n_targets;
            for (int k = 0; k < c.n_targets; ++k) {
                const MaterialHost &mh = ctx->materials[(size_t)c.target_ids[k]];
                a.targets[k] = { c.target_ids[k], mh.rgl.slices(), (int)record_base[k], (const mrl::RglDev *)mh.dev.rgl,
                                 (unsigned long long)brick_base[k], (unsigned long long)planar_off[k] };
            }
            // a call without ids: when its material is no target nothing is added
            if (!c.mat) {
                int at = -1;
                for (int k = 0; k < c.n_targets; ++k) if (c.target_ids[k] == c.single_id) at = k;
                lay.nothing_to_add = at < 0;
                if (at < 0) return MRL_OK;
                a.targets[0] = a.targets[at];
                a.n_targets = 1;
                single = ctx->materials[(size_t)c.single_id].rgl;
            }
            choice = mrl::route_values_grad(ctx->table_grad_kernel, c.mat != nullptr, c.queued, single.n_phi, single.n_theta);
            lay.brick_bytes = choice.plain ? 0 : all.brick_doubles * sizeof(double);
            lay.out_doubles = planar_off[c.n_targets];
            return MRL_OK;
        },
        false,
        [&](char *const *addr, size_t m, double *bricks, double *out) {
            a.wi = (const float *)addr[0]; a.wo = (const float *)addr[1]; a.g = (const float *)addr[2]; a.n = m;
            a.mat = c.mat ? (const int32_t *)addr[3] : nullptr;
            a.bricks = bricks; a.planar = out;
            return mrl::launch_values_grad(choice, a, single, ctx->compute_units, ctx->stream);
        },
        [&](const double *bricks, double *out) {
            hipError_t e = hipSuccess;
            for (int k = 0; k < c.n_targets && e == hipSuccess; ++k)
                e = mrl::launch_values_fold(bricks + brick_base[k], out + planar_off[k], shapes[k], ctx->compute_units, ctx->stream);
            return e;
        } });
}

} // namespace

extern "C" {

int mrl_rgl_values_grad_batch(mrl_ctx *ctx, const float *wi, const float *wo, const float *grad_rgb, const int32_t *mat, int32_t single_id, size_t n,
                              const int32_t *target_ids, int n_targets, double *grad_values)
{
    return rgl_values_grad(ctx, { wi, wo, grad_rgb, 12, "grad_rgb", mat, single_id, n, false, nullptr, nullptr, target_ids, n_targets,
                                  MRL_RGL_GRAD_MAX_TARGETS, grad_values });
}

int mrl_rgl_values_grad_queue(mrl_ctx *ctx, const float *wi, const float *wo, const float *grad_rgb, const int32_t *mat, int32_t single_id,
                              const uint32_t *queue, const uint32_t *queue_count, size_t capacity, const int32_t *target_ids, int n_targets,
                              double *grad_values)
{
    return rgl_values_grad(ctx, { wi, wo, grad_rgb, 12, "grad_rgb", mat, single_id, capacity, true, queue, queue_count, target_ids, n_targets,
                                  MRL_RGL_GRAD_MAX_TARGETS, grad_values });
}

int mrl_rgl_values_shape(const mrl_ctx *ctx, int id, int shape[5])
{
    if (!ctx || !shape) return MRL_ERR_INVALID;
    MRL_GUARD(ctx);
    if (!live_id(ctx, id) || ctx->materials[(size_t)id].dev.kind != mrl::KIND_RGL) return MRL_ERR_MATERIAL;
    shape_of(ctx->materials[(size_t)id].rgl, shape);
    return MRL_OK;
}

int mrl_rgl_values_grad_layout(const int *shapes, int n_targets, size_t *offsets_out)
{
    return values_layout(shapes, n_targets, offsets_out, nullptr, nullptr, nullptr) ? MRL_OK : MRL_ERR_INVALID;
}

int mrl_material_update_rgl_values(mrl_ctx *ctx, int id, const float *rgb, int flags)
{
    if (!ctx) return MRL_ERR_INVALID;
    MRL_GUARD(ctx);
    if (!rgb) return fail(ctx, MRL_ERR_INVALID, "null argument");
    if (flags != 0) return fail(ctx, MRL_ERR_INVALID, "unknown flag bits");
    if (!live_id(ctx, id)) return fail(ctx, MRL_ERR_MATERIAL, "unknown material id");
    MaterialHost &m = ctx->materials[(size_t)id];
    if (m.dev.kind != mrl::KIND_RGL) return fail(ctx, MRL_ERR_MATERIAL, "only RGB RGL materials are updated from an rgb array");
    MRL_HIP(ctx, hipSetDevice(ctx->device));
    const mrl::RglDev &r = m.rgl;
    const size_t floats = (size_t)r.n_phi * r.n_theta * 3 * (size_t)r.ny * (size_t)r.nx;
    const bool from_host = pointer_kind(rgb) == 0;
    const float *d_rgb = rgb;
    if (from_host) {
        for (size_t k = 0; k < floats; ++k)
            if (!std::isfinite(rgb[k])) return fail(ctx, MRL_ERR_INVALID, "non-finite table value");
        const int rc = ctx->buf[mrl_ctx::BUF_STAGE].reserve(ctx, floats * sizeof(float));
        if (rc != MRL_OK) return rc;
        d_rgb = (const float *)ctx->buf[mrl_ctx::BUF_STAGE].p;
    }
    const ScalarPause quiet(ctx);                                // a service instance may be reading the values
    hipStream_t stream = ctx->stream;
    if (from_host) MRL_HIP(ctx, hipMemcpyAsync((void *)d_rgb, rgb, floats * sizeof(float), hipMemcpyHostToDevice, stream));
    MRL_HIP(ctx, mrl::launch_values_write(d_rgb, const_cast<float4 *>(r.rgb_cells), r, ctx->compute_units, stream));
    // who must not run ahead of the new values: the caller's source buffer (host path) and the one-unit service, as in
    // mrl_material_update_table.  Not inside a stream capture (nothing runs there)
    if (from_host || quiet.svc) {
        hipStreamCaptureStatus capturing = hipStreamCaptureStatusNone;
        if (hipStreamIsCapturing(stream, &capturing) != hipSuccess) { (void)hipGetLastError(); capturing = hipStreamCaptureStatusNone; }
        if (capturing == hipStreamCaptureStatusNone) MRL_HIP(ctx, hipStreamSynchronize(stream));
    }
    return MRL_OK;
}

} // extern "C"
