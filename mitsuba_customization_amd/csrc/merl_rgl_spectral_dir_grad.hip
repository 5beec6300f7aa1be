// merl_rgl_spectral_dir_grad.hip — the gradient of eval in the directions and in the wavelengths on spectral RGL materials
// (include/merl_hip_diff_rgl_spectral.h, mrl_rgl_grad_dir_spectral_batch and mrl_rgl_grad_dir_spectral_queue):
// grad_wi[u] = sum_k g_uk d E_k / d wi_u, the same in wo_u, and grad_wavelengths[u][k] = g_uk d E_k / d lambda_uk — per-unit outputs
// like the RGB RGL gradient's (merl_rgl_dir_grad.hip): no workspace, no second kernel, nothing to order.
//   k_rgl_spectral_dir_grad<INDEXED, MULTI, MASK>   persistent grid, grid-stride loop (dir_grad_loop), one lane = one unit:
//                                    rgl::eval_dir_grad_spectral of merl_rgl_spectral_dir_grad.hpp.  Reads 24 + 4 W B of streams per unit
//                                    (+ 4 W with wavelengths, + 4 with material ids, + 4 with a queue), stage 1 of the RGB kernel, and
//                                    per wavelength the corner vectors of its two nodes; writes 12 or 24 B and / or 4 W B.
//   The W loop is a run-time loop: g and lambda are read and grad_wavelengths is written one dword per wavelength and lane (rows are
//   4-byte aligned only), nothing of it is indexed in registers, so it stays out of scratch.
//   !MULTI: the launch's one material; its descriptor arrives by value (SGPRs), parameter grids and integrals are read from the image
//   in memory as the RGB kernel reads them, and the WAVELENGTH grid — searched once per wavelength and unit, a chain of dependent reads —
//   from a copy in LDS (at most 4096 floats; MRL_RGL_SPECTRAL_WL_LDS = 0 reads it from memory: the A/B of DESIGN.md §5q).
//   MULTI: the descriptor is read whole from behind the material a.mat[i] names; a unit whose id names no live spectral RGL material
//   gets zeros in every output; the grids come from memory (rgl::GridMem).  INDEXED: walks a queue.
//   MASK: the bracket shape the kernel is compiled for (1, 3, 5, 15: every single-material launch; 0, tested at run time: ids).
// A unit's bits depend on its inputs and its material alone: every instantiation inlines the same contraction-free function.
#include "merl_ctx.hpp"
#include "../../include/merl_hip_diff_rgl_spectral.h"
#include "merl_rgl_spectral_dir_grad.hpp"
#include "merl_dir_grad.hpp"

namespace mrl {

namespace {

// Launch shape from the compiled register count (DESIGN.md §5q has the compiler's report), by the rule of merl_rgl_dir_grad.hip: the
// largest number of 256-thread blocks per compute unit at which the kernel has no scratch.  Two nodes' corner vectors and their
// five terms each are held per wavelength where the RGB kernel holds three channels' vectors.
constexpr int kRglSpectralDirBlock = 256;
#ifndef MRL_RGL_SPECTRAL_DIR_BLOCKS_PER_CU
#define MRL_RGL_SPECTRAL_DIR_BLOCKS_PER_CU 2
#endif
#ifndef MRL_RGL_SPECTRAL_DIR_BLOCKS_PER_CU_15
#define MRL_RGL_SPECTRAL_DIR_BLOCKS_PER_CU_15 1
#endif
#ifndef MRL_RGL_SPECTRAL_WL_LDS
#define MRL_RGL_SPECTRAL_WL_LDS 1
#endif
constexpr int rgl_spectral_dir_blocks_per_cu(int mask) { return mask == 15 || mask == 0 ? MRL_RGL_SPECTRAL_DIR_BLOCKS_PER_CU_15 : MRL_RGL_SPECTRAL_DIR_BLOCKS_PER_CU; }

struct SpectralRows { const float *wl; float *grad_wl; int W; };    // wavelengths [n][W] or null, grad_wavelengths [n][W] or null

constexpr int kMaxWlNodes = 4096;                                    // rgl_check_shapes' bound on a file's wavelength nodes
__shared__ float rgl_wl_nodes[kMaxWlNodes];
// the parameter grids from the image, the wavelength grid from the block's copy
struct GridWlLds {
    const float *phi, *theta;
    __device__ __forceinline__ float phi_at(int k) const { return phi[k]; }
    __device__ __forceinline__ float theta_at(int k) const { return theta[k]; }
    __device__ __forceinline__ float wavelength_at(int k) const { return rgl_wl_nodes[k]; }
};

template <bool INDEXED, bool MULTI, int MASK>
__global__ __launch_bounds__(kRglSpectralDirBlock, rgl_spectral_dir_blocks_per_cu(MASK)) void k_rgl_spectral_dir_grad(BatchArgs a, DirGradOut o, RglDev r, SpectralRows s)
{
#pragma clang fp contract(off)
    constexpr bool kWlLds = !MULTI && MRL_RGL_SPECTRAL_WL_LDS != 0;
    if constexpr (kWlLds) {
        const int nodes = r.n_wl < kMaxWlNodes ? r.n_wl : kMaxWlNodes;
        for (int k = threadIdx.x; k < nodes; k += kRglSpectralDirBlock) rgl_wl_nodes[k] = r.wavelengths[k];
        __syncthreads();
    }
    dir_grad_loop<kRglSpectralDirBlock, INDEXED>(a, o, [&](size_t i, float (&r_wi)[3], float (&r_wo)[3]) {
        float wix, wiy, wiz, wox, woy, woz;
        load3s<true>(a.wi, i, wix, wiy, wiz);
        load3s<true>(a.wo, i, wox, woy, woz);
        const size_t row = i * (size_t)s.W;
        const float *g_row = o.g + row, *wl_row = s.wl ? s.wl + row : nullptr;
        float *gw_row = s.grad_wl ? s.grad_wl + row : nullptr;
        rgl::RglDirGrad d;
        if constexpr (MULTI) {
            for (int c = 0; c < 3; ++c) r_wi[c] = r_wo[c] = 0.0f;
            const int id = a.mat[i];
            if (id < 0 || id >= a.n_materials || a.materials[id].kind != KIND_RGL_SPECTRAL) {
                if (gw_row) for (int k = 0; k < s.W; ++k) gw_row[k] = 0.0f;
                return false;
            }
            // the unit's descriptor into registers, whole: through a reference every table read would be two dependent loads
            const RglDev rm = *(const RglDev *)a.materials[id].rgl;
            d = rgl::eval_dir_grad_spectral(rm, rgl::GridMem{ rm.phi, rm.theta, rm.wavelengths }, wix, wiy, wiz, wox, woy, woz, g_row, wl_row, s.W, gw_row);
        } else if constexpr (kWlLds) {
            d = rgl::eval_dir_grad_spectral<MASK>(r, GridWlLds{ r.phi, r.theta }, wix, wiy, wiz, wox, woy, woz, g_row, wl_row, s.W, gw_row);
        } else {
            d = rgl::eval_dir_grad_spectral<MASK>(r, rgl::GridMem{ r.phi, r.theta, r.wavelengths }, wix, wiy, wiz, wox, woy, woz, g_row, wl_row, s.W, gw_row);
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) { r_wi[c] = d.wi[c]; r_wo[c] = d.wo[c]; }
        return true;
    });
}

// a.mat: a material id per unit; a.idx: a queue (a.n: its capacity); r: the material of a launch without ids (unused with)
hipError_t launch_rgl_spectral_dir_grad(const BatchArgs &a, const DirGradOut &o, const RglDev &r, const SpectralRows &s, int compute_units, hipStream_t stream)
{
    // the bracket shape of the launch's one file (find_slices' mask); files of any shape meet behind material ids
    const int mask = a.mat ? 0 : 1 | (r.n_phi > 1 ? 2 : 0) | (r.n_theta > 1 ? 4 : 0) | (r.n_phi > 1 && r.n_theta > 1 ? 8 : 0);
    const dim3 grid(grid_blocks(a.n, kRglSpectralDirBlock, (size_t)std::max(compute_units, 1) * rgl_spectral_dir_blocks_per_cu(mask))), block(kRglSpectralDirBlock);
    with_flags([&](auto indexed) {
        switch (mask) {
        case 0:  hipLaunchKernelGGL((k_rgl_spectral_dir_grad<indexed, true, 0>), grid, block, 0, stream, a, o, r, s); break;
        case 1:  hipLaunchKernelGGL((k_rgl_spectral_dir_grad<indexed, false, 1>), grid, block, 0, stream, a, o, r, s); break;
        case 3:  hipLaunchKernelGGL((k_rgl_spectral_dir_grad<indexed, false, 3>), grid, block, 0, stream, a, o, r, s); break;
        case 5:  hipLaunchKernelGGL((k_rgl_spectral_dir_grad<indexed, false, 5>), grid, block, 0, stream, a, o, r, s); break;
        default: hipLaunchKernelGGL((k_rgl_spectral_dir_grad<indexed, false, 15>), grid, block, 0, stream, a, o, r, s); break;
        }
    }, a.idx != nullptr);
    return hipGetLastError();
}

} // namespace

} // namespace mrl

using namespace mrlabi;

namespace {

// both calls: the checks on W and the wavelength arrays here (those of mrl_eval_spectral_*), every other check, the staging of host
// arrays and the launch in grad_dir_call (merl_calls.hip) with the two extra streams
int rgl_grad_dir_spectral(mrl_ctx *ctx, DirGradCall c, const float *wl, int W, float *grad_wl)
{
    if (!ctx) return MRL_ERR_INVALID;
    MRL_GUARD(ctx);
    if (c.n == 0) return MRL_OK;
    if (W < 1 || W > 4096) return fail(ctx, MRL_ERR_INVALID, "1..4096 wavelengths per unit");
    // the materials of one call may have different wavelength grids: "the file's own nodes" names no one set of wavelengths
    if (c.mat && !wl) return fail(ctx, MRL_ERR_INVALID, "a call with material ids needs per-unit wavelengths");
    if (!wl && grad_wl) return fail(ctx, MRL_ERR_INVALID, "grad_wavelengths needs per-unit wavelengths: the file's own nodes are no input of the call");
    if (!c.mat && !wl && c.single_id >= 0 && (size_t)c.single_id < ctx->materials.size()) {
        const MaterialHost &m = ctx->materials[(size_t)c.single_id];
        if (!m.released && m.dev.kind == mrl::KIND_RGL_SPECTRAL && W != m.rgl.n_wl)
            return fail(ctx, MRL_ERR_INVALID, "without a wavelength array the values are those at the file's " + std::to_string(m.rgl.n_wl) + " wavelength nodes");
    }
    const size_t row = 4 * (size_t)W;
    c.extra = { { (void *)wl, row, false, "wavelengths", c.mat != nullptr }, { (void *)grad_wl, row, true, "grad_wavelengths", false } };
    DirGradFamily f = { row, "grad_values",
        [](const MaterialHost &m) { return m.dev.kind == mrl::KIND_RGL_SPECTRAL; },
        "the spectral RGL direction gradient is defined for spectral RGL materials (mrl_material_upload_rgl_spectral)", false,
        [&] { return tombstone_dev(ctx); },
        [&](const mrl::BatchArgs &a, const float *g, float *grad_wi, float *grad_wo, void *const *extra) {
            const mrl::RglDev r = a.mat ? mrl::RglDev{} : ctx->materials[(size_t)c.single_id].rgl;
            return mrl::launch_rgl_spectral_dir_grad(a, { g, grad_wi, grad_wo }, r, { (const float *)extra[0], (float *)extra[1], W }, ctx->compute_units, ctx->stream);
        } };
    // host arrays: chunks of at most 256 MiB of slot, as the spectral eval calls stage them (W may be 4096)
    f.cap_bytes = (size_t)256 << 20;
    return grad_dir_call(ctx, c, f);
}

} // namespace

extern "C" {

int mrl_rgl_grad_dir_spectral_batch(mrl_ctx *ctx, const float *wi, const float *wo, const float *wavelengths, int n_wavelengths, const float *grad_values,
                                    const int32_t *mat, int32_t single_id, size_t n, float *grad_wi, float *grad_wo, float *grad_wavelengths)
{
    return rgl_grad_dir_spectral(ctx, { wi, wo, grad_values, mat, single_id, n, false, nullptr, nullptr, grad_wi, grad_wo }, wavelengths, n_wavelengths, grad_wavelengths);
}

int mrl_rgl_grad_dir_spectral_queue(mrl_ctx *ctx, const float *wi, const float *wo, const float *wavelengths, int n_wavelengths, const float *grad_values,
                                    const int32_t *mat, int32_t single_id, const uint32_t *queue, const uint32_t *queue_count, size_t capacity,
                                    float *grad_wi, float *grad_wo, float *grad_wavelengths)
{
    return rgl_grad_dir_spectral(ctx, { wi, wo, grad_values, mat, single_id, capacity, true, queue, queue_count, grad_wi, grad_wo }, wavelengths, n_wavelengths,
                                 grad_wavelengths);
}

} // extern "C"
