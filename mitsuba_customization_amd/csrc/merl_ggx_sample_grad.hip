// merl_ggx_sample_grad.hip — the gradients of pdf and of sample on GGX conductors (include/merl_hip_diff_sample.h, mrl_ggx_pdf_grad_batch /
// _queue and mrl_ggx_sample_grad_batch / _queue): what an MIS weight and an attached sampler hand back to the shading
// frame and to the roughness.  Per-unit OUTPUTS like the direction gradient of eval (merl_ggx_dir_grad.hip), the parameter gradients
// included: nothing is summed over units, so there is no workspace, no second kernel and nothing to order — the caller sums.
//   k_ggx_pdf_grad<PER_LANE, INDEXED>      one lane = one unit: fast::ggx_pdf_grad of merl_ggx_fast.hpp; reads 28 B per unit (+ 4 with
//                                          material ids, + 4 with a queue), writes up to 28
//   k_ggx_sample_grad<PER_LANE, INDEXED, PARAMS>   one lane = one unit: fast::ggx_sample_grad, the forward chain recomputed and one
//                                          reverse sweep; reads 48 B per unit, writes 12, and 28 more with grad_params (PARAMS)
//   both: persistent grid, grid-stride loop.  PER_LANE: the material comes from mat[i], its constants are built per lane from the
//   context's material array (an id that names no live GGX material: a constant material, outputs forced to zero); otherwise they are
//   wave-uniform.  INDEXED: walks a queue.
// A unit's bits depend on its inputs and its material alone: all instantiations inline the same contraction-free function, and a
// NULL output drops its stores, never a part of the function.
#include "merl_ctx.hpp"
#include "../../include/merl_hip_diff_sample.h"
#include "merl_ggx_fast.hpp"
#include "merl_unit.hpp"

namespace mrl {

namespace {

// Launch shapes from the compiled register counts (granules of 8 out of 512 per SIMD lane; a 256-thread block is one wave per SIMD):
//   k_ggx_pdf_grad      at most 64 VGPRs under the bound below in all four instantiations: eight waves per SIMD, eight blocks per
//                       compute unit
//   k_ggx_sample_grad   the forward chain and the reverse sweep keep some ninety f64 values alive.  With grad_params: 194 to 216
//                       VGPRs, two waves per SIMD, two blocks per compute unit (at three the compiler spills 92 to 172 B, at four 260
//                       to 356 B).  Without (PARAMS = false, the Fresnel parameter terms fall away): 132 to 150 VGPRs, three waves,
//                       three blocks — hence the template; the per-lane function is the same one, so the bits of grad_wi are too
// no scratch, no LDS (tests/test_ggx_sample_grad_cpu.py reads both off the ISA).  That is the grid, so every block of the persistent
// grid is resident at once and the loop strides over the rest.
constexpr int kSampleGradBlock = 256;
constexpr int kPdfGradBlocksPerCu = 8;
constexpr int kSampleGradBlocksPerCu = 2;
constexpr int kSampleGradWiBlocksPerCu = 3;

struct PdfGradOut { const float *g; float *grad_wi, *grad_wo, *grad_alpha; };          // g: [n]
struct SampleGradOut { const float *g; float *grad_wi, *grad_params; };                // g: [n][7]; grad_params: [n][7]

// the material of unit i: its parameters into (alpha, eta, k); false: its id names no live GGX material (a.single, the constant
// material of a launch with ids, is evaluated and the outputs are forced to zero)
template <bool PER_LANE>
__device__ __forceinline__ bool ggx_params(const BatchArgs &a, size_t i, double &alpha, double eta[3], double k[3])
{
    bool known = true;
    alpha = a.single.alpha;
#pragma unroll
    for (int c = 0; c < 3; ++c) { eta[c] = a.single.eta[c]; k[c] = a.single.k[c]; }
    if constexpr (PER_LANE) {
        const LaneMaterial lane = lane_material(a, i);
        const MaterialDev &m = lane.m;
        known = lane.in_range && m.kind == KIND_GGX;
        alpha = known ? m.alpha : alpha;
#pragma unroll
        for (int c = 0; c < 3; ++c) { eta[c] = known ? m.eta[c] : eta[c]; k[c] = known ? m.k[c] : k[c]; }
    }
    return known;
}

template <bool PER_LANE, bool INDEXED>
__global__ __launch_bounds__(kSampleGradBlock, kPdfGradBlocksPerCu) void k_ggx_pdf_grad(BatchArgs a, PdfGradOut o)
{
#pragma clang fp contract(off)
    const size_t stride = (size_t)gridDim.x * kSampleGradBlock;
    const size_t n_items = item_count<INDEXED>(a);
    for (size_t j = (size_t)blockIdx.x * kSampleGradBlock + threadIdx.x; j < n_items; j += stride) {
        const size_t i = INDEXED ? (size_t)a.idx[j] : j;
        double alpha, eta[3], k[3];
        const bool known = ggx_params<PER_LANE>(a, i, alpha, eta, k);
        const fast::GgxConsts g = fast::ggx_consts_exact(alpha, eta, k);
        float wix, wiy, wiz, wox, woy, woz;
        load3s<true>(a.wi, i, wix, wiy, wiz);
        load3s<true>(a.wo, i, wox, woy, woz);
        const fast::GgxPdfGrad r = fast::ggx_pdf_grad(g, wix, wiy, wiz, wox, woy, woz, ldf<true>(o.g + i));
        if (o.grad_wi) {
            const float v[3] = { known ? r.wi[0] : 0.0f, known ? r.wi[1] : 0.0f, known ? r.wi[2] : 0.0f };
            store3s<true>(o.grad_wi, i, v);
        }
        if (o.grad_wo) {
            const float v[3] = { known ? r.wo[0] : 0.0f, known ? r.wo[1] : 0.0f, known ? r.wo[2] : 0.0f };
            store3s<true>(o.grad_wo, i, v);
        }
        if (o.grad_alpha) stf<true>(o.grad_alpha + i, known ? r.alpha : 0.0f);
    }
}

// PARAMS: grad_params is wanted (false: o.grad_params is NULL)
template <bool PER_LANE, bool INDEXED, bool PARAMS>
__global__ __launch_bounds__(kSampleGradBlock, PARAMS ? kSampleGradBlocksPerCu : kSampleGradWiBlocksPerCu) void k_ggx_sample_grad(BatchArgs a, SampleGradOut o)
{
#pragma clang fp contract(off)
    const size_t stride = (size_t)gridDim.x * kSampleGradBlock;
    const size_t n_items = item_count<INDEXED>(a);
    for (size_t j = (size_t)blockIdx.x * kSampleGradBlock + threadIdx.x; j < n_items; j += stride) {
        const size_t i = INDEXED ? (size_t)a.idx[j] : j;
        double alpha, eta[3], k[3];
        const bool known = ggx_params<PER_LANE>(a, i, alpha, eta, k);
        const fast::GgxConsts g = fast::ggx_consts_exact(alpha, eta, k);
        float wix, wiy, wiz, go[7];
        load3s<true>(a.wi, i, wix, wiy, wiz);
        const float u0 = ldf<true>(a.u + 2 * i), u1 = ldf<true>(a.u + 2 * i + 1);
#pragma unroll
        for (int c = 0; c < 7; ++c) go[c] = ldf<true>(o.g + 7 * i + c);
        const fast::GgxSampleGrad r = fast::ggx_sample_grad(g, eta, k, wix, wiy, wiz, u0, u1, go);
        if (o.grad_wi) {
            const float v[3] = { known ? r.wi[0] : 0.0f, known ? r.wi[1] : 0.0f, known ? r.wi[2] : 0.0f };
            store3s<true>(o.grad_wi, i, v);
        }
        if constexpr (PARAMS) {
#pragma unroll
            for (int c = 0; c < 7; ++c) stf<true>(o.grad_params + 7 * i + c, known ? r.params[c] : 0.0f);
        }
    }
}

// a.mat: a material id per unit; a.idx: a queue (a.n: its capacity); a.single: the material of a launch without ids
hipError_t launch_ggx_pdf_grad(const BatchArgs &a, const PdfGradOut &o, int compute_units, hipStream_t stream)
{
    const dim3 grid(grid_blocks(a.n, kSampleGradBlock, (size_t)std::max(compute_units, 1) * kPdfGradBlocksPerCu)), block(kSampleGradBlock);
    with_flags([&](auto per_lane, auto indexed) { hipLaunchKernelGGL((k_ggx_pdf_grad<per_lane, indexed>), grid, block, 0, stream, a, o); },
               a.mat != nullptr, a.idx != nullptr);
    return hipGetLastError();
}

hipError_t launch_ggx_sample_grad(const BatchArgs &a, const SampleGradOut &o, int compute_units, hipStream_t stream)
{
    const int per_cu = o.grad_params ? kSampleGradBlocksPerCu : kSampleGradWiBlocksPerCu;
    const dim3 grid(grid_blocks(a.n, kSampleGradBlock, (size_t)std::max(compute_units, 1) * per_cu)), block(kSampleGradBlock);
    with_flags([&](auto per_lane, auto indexed, auto params) {
                   hipLaunchKernelGGL((k_ggx_sample_grad<per_lane, indexed, params>), grid, block, 0, stream, a, o);
               }, a.mat != nullptr, a.idx != nullptr, o.grad_params != nullptr);
    return hipGetLastError();
}

} // namespace

} // namespace mrl

using namespace mrlabi;

namespace {

// what a unit with an id that names no live GGX material evaluates (its outputs are forced to zero)
mrl::MaterialDev constant_ggx()
{
    mrl::MaterialDev m;
    std::memset(&m, 0, sizeof m);
    m.kind = mrl::KIND_GGX;
    m.alpha = 0.5;
    for (int c = 0; c < 3; ++c) { m.eta[c] = 1.5; m.k[c] = 1.0; }
    return m;
}

bool is_ggx(const MaterialHost &m) { return m.dev.kind == mrl::KIND_GGX; }

// all four calls: the checks, the staging of host arrays and the launch are grad_dir_call's (merl_calls.hip).  grad_alpha and
// grad_params travel as `out` extras; the sample gradient's second input is u (8 B a unit) and it has no grad_wo.
int ggx_pdf_grad(mrl_ctx *ctx, DirGradCall c, float *grad_alpha)
{
    if (!ctx) return MRL_ERR_INVALID;
    c.extra = { { grad_alpha, 4, true, "grad_alpha", false } };
    return grad_dir_call(ctx, c, { 4, "grad_pdf", is_ggx, "the pdf gradient is defined for GGX conductor materials", false, constant_ggx,
        [&](const mrl::BatchArgs &a, const float *g, float *grad_wi, float *grad_wo, void *const *extra) {
            return mrl::launch_ggx_pdf_grad(a, { g, grad_wi, grad_wo, (float *)extra[0] }, ctx->compute_units, ctx->stream);
        } });
}

int ggx_sample_grad(mrl_ctx *ctx, DirGradCall c, float *grad_params)
{
    if (!ctx) return MRL_ERR_INVALID;
    c.extra = { { grad_params, 28, true, "grad_params", false } };
    DirGradFamily f = { 28, "grad_out", is_ggx, "the sample gradient is defined for GGX conductor materials", false, constant_ggx,
        [&](const mrl::BatchArgs &a, const float *g, float *grad_wi, float *, void *const *extra) {
            mrl::BatchArgs b = a;
            b.u = a.wo; b.wo = nullptr;                               // the family's second input
            return mrl::launch_ggx_sample_grad(b, { g, grad_wi, (float *)extra[0] }, ctx->compute_units, ctx->stream);
        } };
    f.second_bytes = 8;
    f.second_name = "u";
    return grad_dir_call(ctx, c, f);
}

} // namespace

extern "C" {

int mrl_ggx_pdf_grad_batch(mrl_ctx *ctx, const float *wi, const float *wo, const float *grad_pdf, const int32_t *mat, int32_t single_id, size_t n,
                           float *grad_wi, float *grad_wo, float *grad_alpha)
{
    return ggx_pdf_grad(ctx, { wi, wo, grad_pdf, mat, single_id, n, false, nullptr, nullptr, grad_wi, grad_wo }, grad_alpha);
}

int mrl_ggx_pdf_grad_queue(mrl_ctx *ctx, const float *wi, const float *wo, const float *grad_pdf, const int32_t *mat, int32_t single_id,
                           const uint32_t *queue, const uint32_t *queue_count, size_t capacity, float *grad_wi, float *grad_wo, float *grad_alpha)
{
    return ggx_pdf_grad(ctx, { wi, wo, grad_pdf, mat, single_id, capacity, true, queue, queue_count, grad_wi, grad_wo }, grad_alpha);
}

int mrl_ggx_sample_grad_batch(mrl_ctx *ctx, const float *wi, const float *u, const float *grad_out, const int32_t *mat, int32_t single_id, size_t n,
                              float *grad_wi, float *grad_params)
{
    return ggx_sample_grad(ctx, { wi, u, grad_out, mat, single_id, n, false, nullptr, nullptr, grad_wi, nullptr }, grad_params);
}

int mrl_ggx_sample_grad_queue(mrl_ctx *ctx, const float *wi, const float *u, const float *grad_out, const int32_t *mat, int32_t single_id,
                              const uint32_t *queue, const uint32_t *queue_count, size_t capacity, float *grad_wi, float *grad_params)
{
    return ggx_sample_grad(ctx, { wi, u, grad_out, mat, single_id, capacity, true, queue, queue_count, grad_wi, nullptr }, grad_params);
}

} // extern "C"
