// merl_rgl_dir_grad.hip — the gradient of eval in the directions on RGB RGL materials (include/merl_hip_diff_rgl.h,
// mrl_rgl_grad_dir_batch and mrl_rgl_grad_dir_queue): grad_wi[u] = sum_c g_uc d eval_c / d wi_u and the same in wo_u,
// a per-unit output like the table direction gradient's (merl_table_dir_grad.hip): no workspace, no second kernel, nothing to order.
//   k_rgl_dir_grad<INDEXED, MULTI, MASK>   persistent grid, grid-stride loop (dir_grad_loop), one lane = one unit: rgl::eval_dir_grad of
//                                    merl_rgl_dir_grad.hpp.  Reads 36 B of streams per unit (+ 4 with material ids, + 4 with a queue),
//                                    one vndf record with its marginal, the ndf and the sigma cell (stage 1, issued together) and the
//                                    three channels' corner vectors (stage 2), writes 12 or 24 B.
//   !MULTI: the launch's one material; its descriptor arrives by value (SGPRs), grids and integrals are read from the image in memory
//   (rgl::GridMem, rgl::SearchMem) — eval of this model makes no search, so a copy in LDS has nothing to serve.
//   MULTI: the descriptor is read whole from behind the material a.mat[i] names (as rgl_walk_ids of merl_rgl.hip reads it); a unit
//   whose id names no live RGB RGL material gets zeros.  INDEXED: walks a queue.
//   MASK: the bracket shape the kernel is compiled for (1, 3, 5, 15: every single-material launch; 0, tested at run time: material
//   ids).  Not a speed-up that was measured: with the shape tested at run time the single-material kernels spill (580 - 668 B of
//   scratch per lane at two waves per SIMD), compiled for a shape the reads and sums are straight-line code and 1, 3 and 5 do not.
// A unit's bits depend on its inputs and its material alone: every instantiation inlines the same contraction-free function.
#include "merl_ctx.hpp"
#include "../../include/merl_hip_diff_rgl.h"
#include "merl_rgl_dir_grad.hpp"
#include "merl_dir_grad.hpp"

namespace mrl {

namespace {

// Launch shape from the compiled register count (DESIGN.md §5p has the compiler's report).  The per-lane math is f64 throughout —
// about 190 registers of state before a table value arrives — on top of up to 24 float4 held between a stage's reads and its sums.
// A bracket of one or two slices (MASK 1, 3, 5) fits 256 VGPRs: two 256-thread blocks per compute unit, two waves per SIMD.  The
// anisotropic shape (15) and the run-time shape (0: material ids) do not: bounded to 256 they spill 312 and 572 B per lane, so
// they get one block per compute unit and the whole register file (256 VGPRs + the accumulation registers, no scratch).
constexpr int kRglDirBlock = 256;
#ifndef MRL_RGL_DIR_BLOCKS_PER_CU
#define MRL_RGL_DIR_BLOCKS_PER_CU 2
#endif
#ifndef MRL_RGL_DIR_BLOCKS_PER_CU_15
#define MRL_RGL_DIR_BLOCKS_PER_CU_15 1
#endif
constexpr int rgl_dir_blocks_per_cu(int mask) { return mask == 15 || mask == 0 ? MRL_RGL_DIR_BLOCKS_PER_CU_15 : MRL_RGL_DIR_BLOCKS_PER_CU; }

template <bool INDEXED, bool MULTI, int MASK>
__global__ __launch_bounds__(kRglDirBlock, rgl_dir_blocks_per_cu(MASK)) void k_rgl_dir_grad(BatchArgs a, DirGradOut o, RglDev r)
{
#pragma clang fp contract(off)
    dir_grad_loop<kRglDirBlock, INDEXED>(a, o, [&](size_t i, float (&r_wi)[3], float (&r_wo)[3]) {
        float wix, wiy, wiz, wox, woy, woz, g32[3];
        load3s<true>(a.wi, i, wix, wiy, wiz);
        load3s<true>(a.wo, i, wox, woy, woz);
        load3s<true>(o.g, i, g32[0], g32[1], g32[2]);
        rgl::RglDirGrad d;
        if constexpr (MULTI) {
            for (int c = 0; c < 3; ++c) r_wi[c] = r_wo[c] = 0.0f;
            const int id = a.mat[i];
            if (id < 0 || id >= a.n_materials || a.materials[id].kind != KIND_RGL) return false;
            // the unit's descriptor into registers, whole: through a reference every table read would be two dependent loads
            const RglDev rm = *(const RglDev *)a.materials[id].rgl;
            d = rgl::eval_dir_grad(rm, rgl::GridMem{ rm.phi, rm.theta, rm.wavelengths }, wix, wiy, wiz, wox, woy, woz, g32);
        } else {
            d = rgl::eval_dir_grad<MASK>(r, rgl::GridMem{ r.phi, r.theta, r.wavelengths }, wix, wiy, wiz, wox, woy, woz, g32);
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) { r_wi[c] = d.wi[c]; r_wo[c] = d.wo[c]; }
        return true;
    });
}

// a.mat: a material id per unit; a.idx: a queue (a.n: its capacity); r: the material of a launch without ids (unused with)
hipError_t launch_rgl_dir_grad(const BatchArgs &a, const DirGradOut &o, const RglDev &r, int compute_units, hipStream_t stream)
{
    // the bracket shape of the launch's one file (find_slices' mask); files of any shape meet behind material ids
    const int mask = a.mat ? 0 : 1 | (r.n_phi > 1 ? 2 : 0) | (r.n_theta > 1 ? 4 : 0) | (r.n_phi > 1 && r.n_theta > 1 ? 8 : 0);
    const dim3 grid(grid_blocks(a.n, kRglDirBlock, (size_t)std::max(compute_units, 1) * rgl_dir_blocks_per_cu(mask))), block(kRglDirBlock);
    with_flags([&](auto indexed) {
        switch (mask) {
        case 0:  hipLaunchKernelGGL((k_rgl_dir_grad<indexed, true, 0>), grid, block, 0, stream, a, o, r); break;
        case 1:  hipLaunchKernelGGL((k_rgl_dir_grad<indexed, false, 1>), grid, block, 0, stream, a, o, r); break;
        case 3:  hipLaunchKernelGGL((k_rgl_dir_grad<indexed, false, 3>), grid, block, 0, stream, a, o, r); break;
        case 5:  hipLaunchKernelGGL((k_rgl_dir_grad<indexed, false, 5>), grid, block, 0, stream, a, o, r); break;
        default: hipLaunchKernelGGL((k_rgl_dir_grad<indexed, false, 15>), grid, block, 0, stream, a, o, r); break;
        }
    }, a.idx != nullptr);
    return hipGetLastError();
}

} // namespace

} // namespace mrl

using namespace mrlabi;

namespace {

// both calls: the checks, the staging of host arrays and the launch are grad_dir_call's (merl_calls.hip)
int rgl_grad_dir(mrl_ctx *ctx, const DirGradCall &c)
{
    if (!ctx) return MRL_ERR_INVALID;
    return grad_dir_call(ctx, c, { 12, "grad_rgb",
        [](const MaterialHost &m) { return m.dev.kind == mrl::KIND_RGL; },
        "the RGL direction gradient is defined for RGB RGL materials (mrl_material_upload_rgl / mrl_material_load_rgl)", false,
        [&] { return tombstone_dev(ctx); },
        [&](const mrl::BatchArgs &a, const float *g, float *grad_wi, float *grad_wo, void *const *) {
            const mrl::RglDev r = a.mat ? mrl::RglDev{} : ctx->materials[(size_t)c.single_id].rgl;
            return mrl::launch_rgl_dir_grad(a, { g, grad_wi, grad_wo }, r, ctx->compute_units, ctx->stream);
        } });
}

} // namespace

extern "C" {

int mrl_rgl_grad_dir_batch(mrl_ctx *ctx, const float *wi, const float *wo, const float *grad_rgb, const int32_t *mat, int32_t single_id, size_t n,
                           float *grad_wi, float *grad_wo)
{
    return rgl_grad_dir(ctx, { wi, wo, grad_rgb, mat, single_id, n, false, nullptr, nullptr, grad_wi, grad_wo });
}

int mrl_rgl_grad_dir_queue(mrl_ctx *ctx, const float *wi, const float *wo, const float *grad_rgb, const int32_t *mat, int32_t single_id,
                           const uint32_t *queue, const uint32_t *queue_count, size_t capacity, float *grad_wi, float *grad_wo)
{
    return rgl_grad_dir(ctx, { wi, wo, grad_rgb, mat, single_id, capacity, true, queue, queue_count, grad_wi, grad_wo });
}

} // extern "C"
