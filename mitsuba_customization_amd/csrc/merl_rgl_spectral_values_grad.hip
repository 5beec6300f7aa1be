// merl_rgl_spectral_values_grad.hip — G += (d eval_spectral / d R)^T g, the adjoint of eval_spectral in the spectra of spectral RGL
// materials, onto up to 16 target materials in one launch, with a material id per unit or over a wavefront queue; and new spectra for
// a resident spectral RGL material in place (include/merl_hip_fit_rgl_spectral.h).  The spectral twin of
// merl_rgl_values_grad.hip: the same wave scatter (merl_grad_scatter.hpp), the RGB per-lane geometry, the spectral channel stage.
//   k_rgl_spectral_values_bricks<MULTI, INDEXED, MASK>  one lane = one unit.  The unit's geometry once (rgl::spectral_values_unit of
//                       merl_rgl_spectral_values_grad.hpp): its slice weights, corner weights and brick offset are parked in LDS.  Then
//                       a loop over the launch's W wavelengths; in each pass a lane reads its g and lambda (one dword each), finds
//                       eval's bracket, reads both nodes' corner vectors, forms the interpolated value with eval's own operations and
//                       parks (key, a) for the two nodes; the wave then adds node c0's and node c0 + 1's runs — 4 S contiguous doubles
//                       [slice][corner] of the unit's brick each — with wave_scatter<4 S>, 64 / (4 S) units per wave-instruction.
//                       Lanes that share a (record, node) are summed first by §5g's rule (wave_merge_rule).
//   k_rgl_spectral_values_fold   per planar texel: the sum of the brick slots that map to it (rgl::spectral_fold_sources, a fixed
//                       order), added into the caller's array when it is not zero
//   k_rgl_spectral_values_plain<MULTI, INDEXED>  the baseline: each lane adds its terms straight into the planar array
//   k_rgl_spectral_values_write  the update: k_rgl_values_write with the channel count as a parameter
// Barriers: the per-pass LDS arrays are guarded by two block barriers per pass, outside every divergent branch — the round count and W
// are launch-uniform, and a dead or out-of-range lane walks the whole loop with key -1.
// !MULTI: the launch's one material, its descriptor by value in the kernel arguments, the kernel compiled for its bracket shape (MASK
// 1 / 3 / 5 / 15) and the file's wavelength nodes in LDS (§5q).  MULTI: a unit's id is compared with the targets of the kernel
// arguments and the RglDev is read whole from behind the target's image; MASK 0, L = 16 with the absent slices masked; the nodes are
// read from memory (rgl::GridMem).
#include "merl_ctx.hpp"
#include "../../include/merl_hip_fit_rgl_spectral.h"
#include "merl_rgl_spectral_values_grad.hpp"
#include "merl_grad_scatter.hpp"

namespace mrl {

namespace {

constexpr int kSvBlock = 256;
constexpr int kSvMaxTargets = MRL_RGL_SPECTRAL_GRAD_MAX_TARGETS;
constexpr int kSvMaxNodes = 4096;                                // rgl_check_shapes' bound on a file's wavelength nodes

// One target of a launch: by value in the kernel arguments (a queue call copies nothing from host memory at call time).  40 B
struct SpectralTarget {
    int id;                              // the material id a unit must carry
    int slices;                          // S of its brackets
    int n_wl;                            // its wavelength nodes
    int key_base;                        // (record, node) pairs of the targets before it: what two lanes compare before they are summed
    const RglDev *dev;                   // the descriptor stored behind the material's image
    unsigned long long brick_base;       // its first brick in the workspace, in doubles
    unsigned long long planar_base;      // its slice of the caller's array, in doubles
};

struct SpectralValuesArgs {
    const float *wi, *wo, *g, *wl;       // g [n][W]; wl [n][W], or null: the file's own nodes (one material, W = its node count)
    int W;
    size_t n;                            // units; of a queue launch the queue's capacity
    const int32_t *mat;                  // MULTI: a unit's material id
    const uint32_t *idx, *idx_count;     // INDEXED: the units idx[0 .. min(*idx_count, n))
    double *bricks, *planar;
    int merge;                           // 0: wave-uniform choice, 1: never, 2: always
    int n_targets;
    SpectralTarget targets[kSvMaxTargets];   // !MULTI: targets[0] is the launch's material
};

// the parameter grids from the image, the wavelength nodes from the block's copy in LDS
struct GridNodesLds {
    const float *phi, *theta, *nodes;
    __device__ __forceinline__ float phi_at(int k) const { return phi[k]; }
    __device__ __forceinline__ float theta_at(int k) const { return theta[k]; }
    __device__ __forceinline__ float wavelength_at(int k) const { return nodes[k]; }
};

// unit i of the launch: its target (by value), its descriptor (MULTI: rm) and its geometry; out of range, of another material or dead: !live
template <bool MULTI, int MASK>
__device__ __forceinline__ rgl::SpectralValuesUnit sv_unit(const SpectralValuesArgs &a, const RglDev &r, size_t i, bool in_range, SpectralTarget &t, RglDev &rm)
{
    float wix = 0.0f, wiy = 0.0f, wiz = 0.0f, wox = 0.0f, woy = 0.0f, woz = 0.0f;
    if (in_range) {
        load3(a.wi, i, wix, wiy, wiz);
        load3(a.wo, i, wox, woy, woz);
    }
    t = a.targets[0];
    rgl::SpectralValuesUnit dead = rgl::SpectralValuesUnit{};
    dead.slices = 1;
    if constexpr (MULTI) {
        const int id = in_range ? a.mat[i] : -1;
        bool known = false;
        for (int k = 0; k < a.n_targets; ++k) {                  // a wave-uniform trip count, scalar loads
            const SpectralTarget &c = a.targets[k];
            const bool hit = in_range && c.id == id;
            t.slices = hit ? c.slices : t.slices; t.n_wl = hit ? c.n_wl : t.n_wl; t.key_base = hit ? c.key_base : t.key_base;
            t.dev = hit ? c.dev : t.dev; t.brick_base = hit ? c.brick_base : t.brick_base; t.planar_base = hit ? c.planar_base : t.planar_base;
            known = known || hit;
        }
        if (!known) return dead;
        // the unit's descriptor into registers, whole: through a reference every table read would be two dependent loads
        rm = *t.dev;
        return rgl::spectral_values_unit<0>(rm, rgl::GridMem{ rm.phi, rm.theta, rm.wavelengths }, wix, wiy, wiz, wox, woy, woz);
    } else {
        if (!in_range) return dead;
        return rgl::spectral_values_unit<MASK>(r, rgl::GridMem{ r.phi, r.theta, r.wavelengths }, wix, wiy, wiz, wox, woy, woz);
    }
}

constexpr int sv_mask_slices(int mask) { return (mask & 1) + ((mask >> 1) & 1) + ((mask >> 2) & 1) + ((mask >> 3) & 1); }

template <bool MULTI, bool INDEXED, int MASK>
__global__ __launch_bounds__(kSvBlock, 2) void k_rgl_spectral_values_bricks(SpectralValuesArgs a, RglDev r)
{
#pragma clang fp contract(off)
    // per unit, parked once per round: the slice and corner weights (factor-major, rows padded by one element: a transposed read lands
    // on different LDS banks), S and the brick's offset.  Per pass: the two nodes' keys and factors, and the first node
    __shared__ int s_slices[kSvBlock];
    __shared__ unsigned long long s_off[kSvBlock];
    __shared__ double s_f[8][kSvBlock + 1];                     // ws[4], wc[4]
    __shared__ int s_key[2][kSvBlock];
    __shared__ int s_c0[kSvBlock];
    __shared__ double s_a[2][kSvBlock];
    __shared__ float s_nodes[MULTI ? 1 : kSvMaxNodes];
    // lanes per (record, node) run: the launch's own shape, or 16 where shapes mix
    constexpr unsigned L = MULTI ? 16u : 4u * (unsigned)sv_mask_slices(MASK);
    const unsigned t = threadIdx.x, lane = t & 63u, wbase = t & ~63u;
    const unsigned slot = lane % L, corner = slot & 3u, slice = slot >> 2;
    if constexpr (!MULTI) {
        const int nodes = r.n_wl < kSvMaxNodes ? r.n_wl : kSvMaxNodes;
        for (int k = (int)t; k < nodes; k += kSvBlock) s_nodes[k] = r.wavelengths[k];
        __syncthreads();
    }
    const int W = a.W;
    const bool own_nodes = a.wl == nullptr;
    const size_t stride = (size_t)gridDim.x * kSvBlock;
    const size_t n_items = grad_items<INDEXED>(a.n, a.idx_count);
    const size_t rounds = (n_items + stride - 1) / stride;       // the same trip count for every thread: barriers inside
    for (size_t rd = 0; rd < rounds; ++rd) {
        const size_t j0 = rd * stride + (size_t)blockIdx.x * kSvBlock + t;
        const bool in_range = j0 < n_items;
        size_t i = j0;
        if constexpr (INDEXED) i = in_range ? (size_t)a.idx[j0] : 0;
        SpectralTarget tg;
        RglDev rm = r;
        const rgl::SpectralValuesUnit u = sv_unit<MULTI, MASK>(a, r, i, in_range, tg, rm);
        const int S = u.live ? u.slices : 1;
        // (the layout refuses more than 2^31 - 1 (record, node) pairs over all targets: the keys fit an int)
        const int key_unit = u.live ? tg.key_base + (int)u.record * tg.n_wl : -1;
        s_slices[t] = S;
        s_off[t] = tg.brick_base + (unsigned long long)u.record * (unsigned long long)(4 * S) * (unsigned long long)tg.n_wl;
#pragma unroll
        for (int q = 0; q < 4; ++q) { s_f[q][t] = u.ws[q]; s_f[4 + q][t] = u.wc[q]; }
        const size_t row = i * (size_t)W;
#pragma nounroll
        for (int k = 0; k < W; ++k) {
            rgl::SpectralValuesPass p = { 0, 0.0, 0.0 };
            if (u.live) {                                        // (no barrier in here)
                const float gk = a.g[row + (size_t)k];
                const float lambda = own_nodes ? 0.0f : a.wl[row + (size_t)k];
                if constexpr (MULTI) p = rgl::spectral_values_pass<0>(rm, rgl::GridMem{ rm.phi, rm.theta, rm.wavelengths }, u, gk, own_nodes, lambda, k);
                else p = rgl::spectral_values_pass<MASK>(r, GridNodesLds{ r.phi, r.theta, s_nodes }, u, gk, own_nodes, lambda, k);
            }
            // a zero factor parks key -1: nothing is added to that node
            s_key[0][t] = p.a0 != 0.0 ? key_unit + p.c0 : -1;
            s_key[1][t] = p.a1 != 0.0 ? key_unit + p.c0 + 1 : -1;
            s_c0[t] = p.c0;
            s_a[0][t] = p.a0; s_a[1][t] = p.a1;
            __syncthreads();
#pragma unroll
            for (int nd = 0; nd < 2; ++nd) {
                const int *keys = s_key[nd];
                const double *fa = s_a[nd];
                const int key = keys[t];
                const uint64_t live = __ballot(key >= 0);        // no lane of the wave has a term for this node: the pass is skipped, wave-uniformly
                wave_scatter<L>(live, wave_merge_rule(a.merge, key, keys, wbase, live), key, keys, wbase, lane,
                    [&](unsigned ref) { return MULTI ? slice < (unsigned)s_slices[ref] : true; },
                    [&](unsigned m, unsigned) { return fa[m] * s_f[slice][m] * s_f[4 + corner][m]; },
                    [&](double acc, unsigned m, unsigned) { return acc + fa[m] * s_f[slice][m] * s_f[4 + corner][m]; },
                    [&](unsigned ref) { return a.bricks + s_off[ref] + (size_t)(s_c0[ref] + nd) * (size_t)(4 * s_slices[ref]) + slot; });
            }
            __syncthreads();
        }
    }
}

template <bool MULTI, bool INDEXED>
__global__ __launch_bounds__(kSvBlock, 2) void k_rgl_spectral_values_plain(SpectralValuesArgs a, RglDev r)
{
#pragma clang fp contract(off)
    const int W = a.W;
    const bool own_nodes = a.wl == nullptr;
    const size_t stride = (size_t)gridDim.x * kSvBlock;
    const size_t n_items = grad_items<INDEXED>(a.n, a.idx_count);
    for (size_t j0 = (size_t)blockIdx.x * kSvBlock + threadIdx.x; j0 < n_items; j0 += stride) {
        const size_t i = INDEXED ? (size_t)a.idx[j0] : j0;
        SpectralTarget tg;
        RglDev rm = r;                                           // MULTI: the unit's material, whole
        const rgl::SpectralValuesUnit u = sv_unit<MULTI, 0>(a, r, i, true, tg, rm);
        if (!u.live) continue;
        double *planar = a.planar + tg.planar_base;
        const rgl::GridMem grids{ rm.phi, rm.theta, rm.wavelengths };
        const size_t row = i * (size_t)W;
#pragma nounroll
        for (int k = 0; k < W; ++k) {
            const float gk = a.g[row + (size_t)k];
            const float lambda = own_nodes ? 0.0f : a.wl[row + (size_t)k];
            const rgl::SpectralValuesPass p = rgl::spectral_values_pass<0>(rm, grids, u, gk, own_nodes, lambda, k);
#pragma unroll
            for (int nd = 0; nd < 2; ++nd) {
                const double an = nd ? p.a1 : p.a0;
                if (an == 0.0) continue;
#pragma unroll
                for (int s = 0; s < 4; ++s)
#pragma unroll
                    for (int jj = 0; jj < 4; ++jj) {
                        const double v = an * u.ws[s] * u.wc[jj];
                        if (s < u.slices && v != 0.0) add_f64(planar + rgl::spectral_values_texel(rm, u, p.c0 + nd, s, jj), v);
                    }
            }
        }
    }
}

__global__ __launch_bounds__(kSvBlock) void k_rgl_spectral_values_fold(const double *bricks, double *planar, int n_phi, int n_theta, int n_ch, int nx, int ny)
{
    const size_t texels = (size_t)n_phi * n_theta * (size_t)n_ch * (size_t)ny * (size_t)nx;
    const size_t stride = (size_t)gridDim.x * kSvBlock;
    for (size_t t = (size_t)blockIdx.x * kSvBlock + threadIdx.x; t < texels; t += stride) {
        const int x = (int)(t % (size_t)nx), y = (int)((t / (size_t)nx) % (size_t)ny), c = (int)((t / ((size_t)nx * ny)) % (size_t)n_ch);
        const size_t slice = t / ((size_t)nx * ny * (size_t)n_ch);
        const int it = (int)(slice % (size_t)n_theta), ip = (int)(slice / (size_t)n_theta);
        size_t src[16];
        const int n = rgl::spectral_fold_sources(n_phi, n_theta, nx, ny, n_ch, ip, it, c, y, x, src);
        double acc = 0.0;
        for (int k = 0; k < n; ++k) acc += bricks[src[k]];
        // a texel nothing reached keeps its bits (x + 0 would turn -0 into +0)
        if (acc != 0.0) planar[t] += acc;
    }
}

// The device twin of the value branch of append_warp (merl_rgl.hip) for n_ch channels: float4 f of the value bricks
// [bracket][cell][channel][slice] is the four nodes (y, x) (y, x + 1) (y + 1, x) (y + 1, x + 1) of its slice and channel in
// src [n_phi][n_theta][n_ch][ny][nx].  No arithmetic.
__global__ __launch_bounds__(kSvBlock) void k_rgl_spectral_values_write(const float *__restrict__ src, float4 *__restrict__ cells, int n_phi, int n_theta, int n_ch,
                                                                        int nx, int ny)
{
    const int tb = n_theta > 1 ? n_theta - 1 : 1, pb = n_phi > 1 ? n_phi - 1 : 1;
    const int S = (n_phi > 1 ? 2 : 1) * (n_theta > 1 ? 2 : 1);
    const size_t per_c = (size_t)(nx - 1) * (size_t)(ny - 1), per_cell = (size_t)n_ch * (size_t)S, total = (size_t)pb * tb * per_c * per_cell;
    const size_t stride = (size_t)gridDim.x * kSvBlock;
    for (size_t f = (size_t)blockIdx.x * kSvBlock + threadIdx.x; f < total; f += stride) {
        const int slot = (int)(f % (size_t)S), ch = (int)((f / (size_t)S) % (size_t)n_ch);
        const size_t cell = (f / per_cell) % per_c, br = f / (per_cell * per_c);
        const int ipb = (int)(br / (size_t)tb), itb = (int)(br % (size_t)tb);
        const int dp = n_phi > 1 ? (slot & 1) : 0, dt = n_phi > 1 ? (slot >> 1) : slot;
        const size_t slice = (size_t)(ipb + dp) * n_theta + (size_t)(itb + dt);
        const size_t y = cell / (size_t)(nx - 1), x = cell % (size_t)(nx - 1);
        const float *p = src + ((slice * (size_t)n_ch + (size_t)ch) * (size_t)ny + y) * (size_t)nx + x;
        cells[f] = make_float4(p[0], p[1], p[nx], p[nx + 1]);
    }
}

// ---- which instantiation a launch takes: pure arithmetic, then the one place that names the kernels ----
struct SpectralValuesChoice {
    bool plain;         // MRL_OPT_TABLE_GRAD_KERNEL = 1
    bool multi;         // a material id per unit
    bool indexed;       // over a queue
    int mask;           // the bracket shape the kernel is compiled for; 0: tested at run time (multi, and the plain form)
    int merge;          // bricks: 0 wave-uniform, 1 never, 2 always
};
SpectralValuesChoice route_spectral_values_grad(int variant, bool multi, bool indexed, int n_phi, int n_theta)
{
    const bool plain = variant == 1;
    const int mask = multi || plain ? 0 : 1 | (n_phi > 1 ? 2 : 0) | (n_theta > 1 ? 4 : 0) | (n_phi > 1 && n_theta > 1 ? 8 : 0);
    return { plain, multi, indexed, mask, variant == 2 ? 1 : (variant == 3 ? 2 : 0) };
}

hipError_t launch_spectral_values_grad(const SpectralValuesChoice &k, SpectralValuesArgs a, const RglDev &r, int compute_units, hipStream_t stream)
{
    if (a.n == 0) return hipSuccess;
    const dim3 grid(grid_blocks(a.n, kSvBlock, (size_t)std::max(compute_units, 1) * 2)), block(kSvBlock);
    a.merge = k.merge;
    with_flags([&](auto ix) {
        if (k.plain) {
            if (k.multi) hipLaunchKernelGGL((k_rgl_spectral_values_plain<true, ix>), grid, block, 0, stream, a, r);
            else hipLaunchKernelGGL((k_rgl_spectral_values_plain<false, ix>), grid, block, 0, stream, a, r);
            return;
        }
        switch (k.mask) {
        case 0:  hipLaunchKernelGGL((k_rgl_spectral_values_bricks<true, ix, 0>), grid, block, 0, stream, a, r); break;
        case 1:  hipLaunchKernelGGL((k_rgl_spectral_values_bricks<false, ix, 1>), grid, block, 0, stream, a, r); break;
        case 3:  hipLaunchKernelGGL((k_rgl_spectral_values_bricks<false, ix, 3>), grid, block, 0, stream, a, r); break;
        case 5:  hipLaunchKernelGGL((k_rgl_spectral_values_bricks<false, ix, 5>), grid, block, 0, stream, a, r); break;
        default: hipLaunchKernelGGL((k_rgl_spectral_values_bricks<false, ix, 15>), grid, block, 0, stream, a, r); break;
        }
    }, k.indexed);
    return hipGetLastError();
}

hipError_t launch_spectral_values_fold(const double *bricks, double *planar, const int shape[5], int compute_units, hipStream_t stream)
{
    const size_t texels = (size_t)shape[0] * shape[1] * (size_t)shape[2] * (size_t)shape[3] * (size_t)shape[4];
    hipLaunchKernelGGL(k_rgl_spectral_values_fold, dim3(grid_blocks(texels, kSvBlock, (size_t)std::max(compute_units, 1) * 8)), dim3(kSvBlock), 0, stream,
                       bricks, planar, shape[0], shape[1], shape[2], shape[4], shape[3]);
    return hipGetLastError();
}

hipError_t launch_spectral_values_write(const float *src, float4 *cells, const RglDev &r, int compute_units, hipStream_t stream)
{
    const size_t total = rgl::values_records(r.n_phi, r.n_theta, r.nx, r.ny) * (size_t)r.n_wl * (size_t)r.slices();
    hipLaunchKernelGGL(k_rgl_spectral_values_write, dim3(grid_blocks(total, kSvBlock, (size_t)std::max(compute_units, 1) * 8)), dim3(kSvBlock), 0, stream,
                       src, cells, r.n_phi, r.n_theta, r.n_wl, r.nx, r.ny);
    return hipGetLastError();
}

} // namespace

} // namespace mrl

using namespace mrlabi;

namespace {

bool live_spectral(const mrl_ctx *ctx, int id)
{
    return id >= 0 && (size_t)id < ctx->materials.size() && !ctx->materials[(size_t)id].released && ctx->materials[(size_t)id].dev.kind == mrl::KIND_RGL_SPECTRAL;
}

// the planar shape of a material's spectra: n_phi, n_theta, n_wl, ny, nx
void shape_of(const mrl::RglDev &r, int shape[5]) { shape[0] = r.n_phi; shape[1] = r.n_theta; shape[2] = r.n_wl; shape[3] = r.ny; shape[4] = r.nx; }

struct SpectralLayout { size_t pairs, brick_doubles; };       // over all targets
// per target: (record, node) pairs before it, its first brick and its planar slice (doubles).  False: what the layout function refuses
bool spectral_layout(const int *shapes, int n_targets, size_t *planar_off, size_t *key_base, size_t *brick_base, SpectralLayout *all)
{
    if (!shapes || n_targets < 1 || n_targets > MRL_RGL_SPECTRAL_GRAD_MAX_TARGETS) return false;
    uint64_t pairs = 0, bricks = 0, planar = 0;
    for (int k = 0; k < n_targets; ++k) {
        const int *s = shapes + 5 * k;
        if (s[0] < 1 || s[1] < 1 || s[2] < 1 || s[2] > 4096 || s[3] < 2 || s[4] < 2) return false;
        // checked pair by pair: no product leaves 64 bits
        const uint64_t brackets = (uint64_t)(s[0] > 1 ? s[0] - 1 : 1) * (uint64_t)(s[1] > 1 ? s[1] - 1 : 1), cells = (uint64_t)(s[3] - 1) * (uint64_t)(s[4] - 1);
        if (brackets > (uint64_t)INT32_MAX || cells > (uint64_t)INT32_MAX) return false;
        const uint64_t rec = brackets * cells;
        if (rec > (uint64_t)INT32_MAX) return false;
        const uint64_t rec_nodes = rec * (uint64_t)s[2];                 // at most 2^43
        const uint64_t slices = (uint64_t)s[0] * (uint64_t)s[1], per = (uint64_t)s[3] * (uint64_t)s[4];
        const int S = (s[0] > 1 ? 2 : 1) * (s[1] > 1 ? 2 : 1);
        if (planar_off) planar_off[k] = (size_t)planar;
        if (key_base) key_base[k] = (size_t)pairs;
        if (brick_base) brick_base[k] = (size_t)bricks;
        pairs += rec_nodes;
        if (pairs > (uint64_t)INT32_MAX) return false;
        bricks += rec_nodes * (uint64_t)(4 * S);
        planar += (uint64_t)s[2] * slices * per;
    }
    if (planar_off) planar_off[n_targets] = (size_t)planar;
    if (all) { all->pairs = (size_t)pairs; all->brick_doubles = (size_t)bricks; }
    return true;
}

// mrl_rgl_spectral_values_grad_batch / _queue: the checks on W and the wavelength array here (those of mrl_rgl_grad_dir_spectral_*),
// every other check, the workspace and the host-array path in grad_scatter_call (merl_grad_scatter.hip) with the one extra stream
int rgl_spectral_values_grad(mrl_ctx *ctx, GradScatterCall c, const float *wl, int W)
{
    if (!ctx) return MRL_ERR_INVALID;
    MRL_GUARD(ctx);
    if (c.n == 0) return MRL_OK;
    if (W < 1 || W > 4096) return fail(ctx, MRL_ERR_INVALID, "1..4096 wavelengths per unit");
    // the materials of one call may have different wavelength grids: "the file's own nodes" names no one set of wavelengths
    if (c.mat && !wl) return fail(ctx, MRL_ERR_INVALID, "a call with material ids needs per-unit wavelengths");
    if (!c.mat && !wl && live_spectral(ctx, c.single_id) && W != ctx->materials[(size_t)c.single_id].rgl.n_wl)
        return fail(ctx, MRL_ERR_INVALID, "without a wavelength array the values are those at the file's " +
                                              std::to_string(ctx->materials[(size_t)c.single_id].rgl.n_wl) + " wavelength nodes");
    c.g_bytes = 4 * (size_t)W;
    c.extra = wl; c.extra_bytes = 4 * (size_t)W; c.extra_name = "wavelengths";
    c.cap_bytes = (size_t)256 << 20;                             // host arrays: as the spectral eval calls stage them (W may be 4096)
    mrl::SpectralValuesArgs a;
    std::memset(&a, 0, sizeof a);
    a.W = W;
    int shapes[MRL_RGL_SPECTRAL_GRAD_MAX_TARGETS][5];
    size_t planar_off[MRL_RGL_SPECTRAL_GRAD_MAX_TARGETS + 1], key_base[MRL_RGL_SPECTRAL_GRAD_MAX_TARGETS], brick_base[MRL_RGL_SPECTRAL_GRAD_MAX_TARGETS];
    mrl::RglDev single{};                                        // a call without ids: its one material, by value
    mrl::SpectralValuesChoice choice{};
    return grad_scatter_call(ctx, c, {
        [&](int32_t id) {
            if (!live_spectral(ctx, id))
                return fail(ctx, MRL_ERR_MATERIAL, "a target is not a live spectral RGL material (mrl_material_upload_rgl_spectral)");
            return (int)MRL_OK;
        },
        [&](GradScatterLayout &lay) -> int {
            for (int k = 0; k < c.n_targets; ++k) shape_of(ctx->materials[(size_t)c.target_ids[k]].rgl, shapes[k]);
            SpectralLayout all;
            if (!spectral_layout(&shapes[0][0], c.n_targets, planar_off, key_base, brick_base, &all))
                return fail(ctx, MRL_ERR_INVALID, "the targets have more than 2^31 - 1 (workspace record, node) pairs in all");
            a.idx = c.queue; a.idx_count = c.queue_count;
            a.n_targets = c.n_targets;
            for (int k = 0; k < c.n_targets; ++k) {
                const MaterialHost &mh = ctx->materials[(size_t)c.target_ids[k]];
                a.targets[k] = { c.target_ids[k], mh.rgl.slices(), mh.rgl.n_wl, (int)key_base[k], (const mrl::RglDev *)mh.dev.rgl,
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
            choice = mrl::route_spectral_values_grad(ctx->table_grad_kernel, c.mat != nullptr, c.queued, single.n_phi, single.n_theta);
            lay.brick_bytes = choice.plain ? 0 : all.brick_doubles * sizeof(double);
            lay.out_doubles = planar_off[c.n_targets];
            return MRL_OK;
        },
        false,
        [&](char *const *addr, size_t m, double *bricks, double *out) {
            a.wi = (const float *)addr[0]; a.wo = (const float *)addr[1]; a.g = (const float *)addr[2]; a.n = m;
            a.mat = c.mat ? (const int32_t *)addr[3] : nullptr;
            a.wl = wl ? (const float *)addr[c.mat ? 4 : 3] : nullptr;
            a.bricks = bricks; a.planar = out;
            return mrl::launch_spectral_values_grad(choice, a, single, ctx->compute_units, ctx->stream);
        },
        [&](const double *bricks, double *out) {
            hipError_t e = hipSuccess;
            for (int k = 0; k < c.n_targets && e == hipSuccess; ++k)
                e = mrl::launch_spectral_values_fold(bricks + brick_base[k], out + planar_off[k], shapes[k], ctx->compute_units, ctx->stream);
            return e;
        } });
}

} // namespace

extern "C" {

int mrl_rgl_spectral_values_grad_batch(mrl_ctx *ctx, const float *wi, const float *wo, const float *wavelengths, int n_wavelengths, const float *grad_values,
                                       const int32_t *mat, int32_t single_id, size_t n, const int32_t *target_ids, int n_targets, double *grad_spectra)
{
    return rgl_spectral_values_grad(ctx, { wi, wo, grad_values, 4, "grad_values", mat, single_id, n, false, nullptr, nullptr, target_ids, n_targets,
                                           MRL_RGL_SPECTRAL_GRAD_MAX_TARGETS, grad_spectra }, wavelengths, n_wavelengths);
}

int mrl_rgl_spectral_values_grad_queue(mrl_ctx *ctx, const float *wi, const float *wo, const float *wavelengths, int n_wavelengths, const float *grad_values,
                                       const int32_t *mat, int32_t single_id, const uint32_t *queue, const uint32_t *queue_count, size_t capacity,
                                       const int32_t *target_ids, int n_targets, double *grad_spectra)
{
    return rgl_spectral_values_grad(ctx, { wi, wo, grad_values, 4, "grad_values", mat, single_id, capacity, true, queue, queue_count, target_ids, n_targets,
                                           MRL_RGL_SPECTRAL_GRAD_MAX_TARGETS, grad_spectra }, wavelengths, n_wavelengths);
}

int mrl_rgl_spectral_values_shape(const mrl_ctx *ctx, int id, int shape[5])
{
    if (!ctx || !shape) return MRL_ERR_INVALID;
    MRL_GUARD(ctx);
    if (!live_spectral(ctx, id)) return MRL_ERR_MATERIAL;
    shape_of(ctx->materials[(size_t)id].rgl, shape);
    return MRL_OK;
}

int mrl_rgl_spectral_values_grad_layout(const int *shapes, int n_targets, size_t *offsets_out)
{
    return spectral_layout(shapes, n_targets, offsets_out, nullptr, nullptr, nullptr) ? MRL_OK : MRL_ERR_INVALID;
}

int mrl_material_update_rgl_spectral_values(mrl_ctx *ctx, int id, const float *spectra, int flags)
{
    if (!ctx) return MRL_ERR_INVALID;
    MRL_GUARD(ctx);
    if (!spectra) return fail(ctx, MRL_ERR_INVALID, "null argument");
    if (flags != 0) return fail(ctx, MRL_ERR_INVALID, "unknown flag bits");
    if (id < 0 || (size_t)id >= ctx->materials.size() || ctx->materials[(size_t)id].released) return fail(ctx, MRL_ERR_MATERIAL, "unknown material id");
    if (!live_spectral(ctx, id)) return fail(ctx, MRL_ERR_MATERIAL, "only spectral RGL materials are updated from a spectra array");
    MaterialHost &m = ctx->materials[(size_t)id];
    MRL_HIP(ctx, hipSetDevice(ctx->device));
    const mrl::RglDev &r = m.rgl;
    const size_t floats = (size_t)r.n_phi * r.n_theta * (size_t)r.n_wl * (size_t)r.ny * (size_t)r.nx;
    const bool from_host = pointer_kind(spectra) == 0;
    const float *d_src = spectra;
    if (from_host) {
        for (size_t k = 0; k < floats; ++k)
            if (!std::isfinite(spectra[k])) return fail(ctx, MRL_ERR_INVALID, "non-finite table value");
        const int rc = ctx->buf[mrl_ctx::BUF_STAGE].reserve(ctx, floats * sizeof(float));
        if (rc != MRL_OK) return rc;
        d_src = (const float *)ctx->buf[mrl_ctx::BUF_STAGE].p;
    }
    const ScalarPause quiet(ctx);                                // a service instance may be reading the values
    hipStream_t stream = ctx->stream;
    if (from_host) MRL_HIP(ctx, hipMemcpyAsync((void *)d_src, spectra, floats * sizeof(float), hipMemcpyHostToDevice, stream));
    MRL_HIP(ctx, mrl::launch_spectral_values_write(d_src, const_cast<float4 *>(r.rgb_cells), r, ctx->compute_units, stream));
    // who must not run ahead of the new values: the caller's source buffer (host path) and the one-unit service, as in
    // mrl_material_update_rgl_values.  Not inside a stream capture (nothing runs there)
    if (from_host || quiet.svc) {
        hipStreamCaptureStatus capturing = hipStreamCaptureStatusNone;
        if (hipStreamIsCapturing(stream, &capturing) != hipSuccess) { (void)hipGetLastError(); capturing = hipStreamCaptureStatusNone; }
        if (capturing == hipStreamCaptureStatusNone) MRL_HIP(ctx, hipStreamSynchronize(stream));
    }
    return MRL_OK;
}

} // extern "C"
