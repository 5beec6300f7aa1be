// merl_ggx_grad.hip — the parameter gradient of eval on one GGX conductor (include/merl_hip_fit.h, mrl_ggx_grad_batch):
// grad_params += sum_u sum_c g_uc J_uc and normal += sum_u sum_c h_uc J_uc J_uc^T with J_uc = d eval_c(wi_u, wo_u) / d (alpha, eta, k).
// The opposite shape of the table adjoint (merl_table_grad.hip): f64 math per unit, reduced to 7 (+ 16) numbers, nothing scattered.
//   k_ggx_grad<NORMAL>   persistent grid, one lane = one unit per round: the forward-mode twins of merl_ggx_fast.hpp, f64 accumulators
//                        in registers across the grid-stride loop, then wave (cross-lane moves) -> block (LDS) -> one row of the
//                        workspace [grid][kRow] per block, written with plain stores
//   k_ggx_grad_sum       one block: the rows summed in a fixed order and added to the caller's outputs
// No atomics and nothing to clear: every row is written before it is read, and grid and order depend on (n, compute units) alone,
// so two calls on the same inputs return the same bits.
#include "merl_ctx.hpp"
#include "../../include/merl_hip_fit.h"
#include "merl_ggx_fast.hpp"
#include "merl_ggx_grad.hpp"

namespace mrl {

namespace {

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / 64;
constexpr int kBlocksPerCu = 3;           // the gradient + normal kernel holds 162 VGPRs: three waves per SIMD are resident.  One grid for both
                                         // kernels: grad_params must not depend on whether `normal` is asked for
constexpr int kSumBlock = 1024;          // kParams, kNormalTerms, kRow, normal_entry, wave_sum: merl_ggx_grad.hpp
constexpr int kSumGroups = kSumBlock / kRow;

struct GgxGradArgs {
    const float *wi, *wo, *g, *h;        // h: nullptr = 1
    size_t n;
    MaterialDev m;
    double *partials;                    // [grid][kRow]
};

template <bool NORMAL>
__global__ __launch_bounds__(kBlock) void k_ggx_grad(GgxGradArgs a)
{
#pragma clang fp contract(off)
    constexpr int K = kParams + (NORMAL ? kNormalTerms : 0);
    __shared__ double s_part[kWaves][kRow];
    const fast::GgxConsts g(a.m);
    double acc[K];
#pragma unroll
    for (int k = 0; k < K; ++k) acc[k] = 0.0;
    const bool has_h = a.h != nullptr;
    const size_t stride = (size_t)gridDim.x * kBlock;
    for (size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x; i < a.n; i += stride) {
        float wix, wiy, wiz, wox, woy, woz, g32[3], h32[3] = { 1.0f, 1.0f, 1.0f };
        load3(a.wi, i, wix, wiy, wiz);
        load3(a.wo, i, wox, woy, woz);
        load3(a.g, i, g32[0], g32[1], g32[2]);
        if (NORMAL && has_h) load3(a.h, i, h32[0], h32[1], h32[2]);
        const fast::GgxJacobian j = fast::ggx_eval_jacobian(g, a.m.eta, a.m.k, fast::normalize_f32(wix, wiy, wiz), fast::normalize_f32(wox, woy, woz));
        // what eval masks, and where its D / G1 selects return 0: removed by selects — the Jacobian of such a unit is garbage and
        // its g and h may be NaN
        const float poison = fast::cos_or_nan32((wix + wiy + wiz), wox, woy, woz, true);
        const bool live = (wiz > 0.0f) && (woz > 0.0f) && (poison == poison) && j.live;
        double sum_a = 0.0, sum_aa = 0.0;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const double gc = live ? (double)g32[c] : 0.0;
            const double ja = live ? j.d_alpha[c] : 0.0, je = live ? j.d_eta[c] : 0.0, jk = live ? j.d_k[c] : 0.0;
            sum_a = __builtin_fma(gc, ja, sum_a);
            acc[1 + c] = __builtin_fma(gc, je, acc[1 + c]);
            acc[4 + c] = __builtin_fma(gc, jk, acc[4 + c]);
            if constexpr (NORMAL) {
                const double hc = live ? (double)h32[c] : 0.0;
                const double ha = hc * ja, he = hc * je, hk = hc * jk;
                sum_aa = __builtin_fma(ha, ja, sum_aa);
                acc[kParams + 1 + c] = __builtin_fma(ha, je, acc[kParams + 1 + c]);
                acc[kParams + 4 + c] = __builtin_fma(ha, jk, acc[kParams + 4 + c]);
                acc[kParams + 7 + c] = __builtin_fma(he, je, acc[kParams + 7 + c]);
                acc[kParams + 10 + c] = __builtin_fma(he, jk, acc[kParams + 10 + c]);
                acc[kParams + 13 + c] = __builtin_fma(hk, jk, acc[kParams + 13 + c]);
            }
        }
        acc[0] += sum_a;
        if constexpr (NORMAL) acc[kParams] += sum_aa;
    }
    const unsigned t = threadIdx.x, lane = t & 63u, wave = t >> 6;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const double s = wave_sum(acc[k]);
        if (lane == 0) s_part[wave][k] = s;
    }
    __syncthreads();
    if (t < (unsigned)K) {
        double s = s_part[0][t];
#pragma unroll
        for (int w = 1; w < kWaves; ++w) s += s_part[w][t];
        a.partials[(size_t)blockIdx.x * kRow + t] = s;
    }
}

// terms: kParams, or kParams + kNormalTerms (then `normal` is written, both triangles).  Thread (group, column) sums the rows
// group, group + kSumGroups, ... of its column; the groups are then summed in order.
__global__ __launch_bounds__(kSumBlock) void k_ggx_grad_sum(const double *partials, unsigned rows, int terms, double *grad, double *normal)
{
    __shared__ double s_sum[kSumGroups][kRow + 1];
    const unsigned t = threadIdx.x, col = t % kRow, group = t / kRow;
    double acc = 0.0;
    if (col < (unsigned)terms)
        for (unsigned r = group; r < rows; r += kSumGroups) acc += partials[(size_t)r * kRow + col];
    s_sum[group][col] = acc;
    __syncthreads();
    if (t < (unsigned)terms) {
        double total = s_sum[0][t];
        for (int q = 1; q < kSumGroups; ++q) total += s_sum[q][t];
        if (t < (unsigned)kParams) {
            grad[t] += total;
        } else {
            int ea, eb;
            normal_entry((int)t - kParams, ea, eb);
            normal[ea * kParams + eb] += total;
            if (ea != eb) normal[eb * kParams + ea] += total;
        }
    }
}

size_t ggx_grad_max_rows(int compute_units) { return (size_t)std::max(compute_units, 1) * kBlocksPerCu; }
unsigned ggx_grad_grid(size_t n, int compute_units) { return grid_blocks(n, kBlock, ggx_grad_max_rows(compute_units)); }

// the rows the largest grid writes, and behind them the sums of a host-array call: grad[kParams] | normal[kParams][kParams]
size_t ggx_grad_workspace_bytes(int compute_units)
{
    return (ggx_grad_max_rows(compute_units) * kRow + kParams + kParams * kParams) * sizeof(double);
}

// grad (+ normal, unless nullptr) += the sums over a's units; grad and normal are device pointers
hipError_t launch_ggx_grad(const GgxGradArgs &a, double *grad, double *normal, int compute_units, hipStream_t stream)
{
    const unsigned grid = ggx_grad_grid(a.n, compute_units);
    if (normal) hipLaunchKernelGGL(k_ggx_grad<true>, dim3(grid), dim3(kBlock), 0, stream, a);
    else hipLaunchKernelGGL(k_ggx_grad<false>, dim3(grid), dim3(kBlock), 0, stream, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_ggx_grad_sum, dim3(1), dim3(kSumBlock), 0, stream, (const double *)a.partials, grid,
                       kParams + (normal ? kNormalTerms : 0), grad, normal);
    return hipGetLastError();
}

} // namespace

} // namespace mrl

using namespace mrlabi;

extern "C" {

int mrl_ggx_grad_batch(mrl_ctx *ctx, const float *wi, const float *wo, const float *grad_rgb, const float *curv_rgb, int32_t id, size_t n,
                       double grad_params[7], double *normal)
{
    if (!ctx) return MRL_ERR_INVALID;
    MRL_GUARD(ctx);
    if (n == 0) return MRL_OK;
    StreamList streams = { { (void *)wi, 12, false, "wi" }, { (void *)wo, 12, false, "wo" }, { (void *)grad_rgb, 12, false, "grad_rgb" } };
    if (first_null(streams) || !grad_params) return fail(ctx, MRL_ERR_INVALID, "null array argument");
    if (curv_rgb) streams.push_back({ (void *)curv_rgb, 12, false, "curv_rgb" });
    if (id < 0 || (size_t)id >= ctx->materials.size() || ctx->materials[(size_t)id].released) return fail(ctx, MRL_ERR_MATERIAL, "unknown material id");
    const MaterialHost &mh = ctx->materials[(size_t)id];
    if (mh.dev.kind != mrl::KIND_GGX) return fail(ctx, MRL_ERR_MATERIAL, "the parameter gradient is defined for GGX conductor materials");
    MRL_HIP(ctx, hipSetDevice(ctx->device));
    const int kind = common_kind({ grad_params, normal }, streams);
    if (kind < 0) return fail(ctx, MRL_ERR_POINTER_MIX, "host and device pointers mixed in one call");

    DeviceBuf &work = ctx->buf[mrl_ctx::BUF_GGX_GRAD];
    const int rc = work.reserve(ctx, mrl::ggx_grad_workspace_bytes(ctx->compute_units));
    if (rc != MRL_OK) return rc;
    mrl::GgxGradArgs a;
    std::memset(&a, 0, sizeof a);
    a.m = mh.dev;
    a.partials = (double *)work.p;
    if (kind == 1) {
        a.wi = wi; a.wo = wo; a.g = grad_rgb; a.h = curv_rgb; a.n = n;
        MRL_HIP(ctx, mrl::launch_ggx_grad(a, grad_params, normal, ctx->compute_units, ctx->stream));
        return MRL_OK;
    }
    // host arrays: the inputs are staged chunk by chunk, every chunk adds to one small device array, and that is added to the
    // caller's on the host
    constexpr int kSums = mrl::kParams + mrl::kParams * mrl::kParams;
    double *d_sums = a.partials + mrl::ggx_grad_max_rows(ctx->compute_units) * mrl::kRow;
    static const double zeros[kSums] = {};
    double sums[kSums];
    MRL_HIP(ctx, hipMemcpyAsync(d_sums, zeros, sizeof zeros, hipMemcpyHostToDevice, ctx->stream));
    const int rs = run_host_staged(ctx, streams, n, 0, [&](char *const *addr, size_t m) -> int {
        a.wi = (const float *)addr[0]; a.wo = (const float *)addr[1]; a.g = (const float *)addr[2];
        a.h = curv_rgb ? (const float *)addr[3] : nullptr; a.n = m;
        MRL_HIP(ctx, mrl::launch_ggx_grad(a, d_sums, normal ? d_sums + mrl::kParams : nullptr, ctx->compute_units, ctx->stream));
        return MRL_OK;
    });
    if (rs != MRL_OK) { (void)hipStreamSynchronize(ctx->stream); return rs; }
    MRL_HIP(ctx, hipMemcpyAsync(sums, d_sums, sizeof sums, hipMemcpyDeviceToHost, ctx->stream));
    MRL_HIP(ctx, hipStreamSynchronize(ctx->stream));
    for (int k = 0; k < mrl::kParams; ++k) grad_params[k] += sums[k];
    if (normal)
        for (int j = 0; j < mrl::kNormalTerms; ++j) {
            int ea, eb;
            mrl::normal_entry(j, ea, eb);
            normal[ea * mrl::kParams + eb] += sums[mrl::kParams + ea * mrl::kParams + eb];
            if (ea != eb) normal[eb * mrl::kParams + ea] += sums[mrl::kParams + eb * mrl::kParams + ea];
        }
    return MRL_OK;
}

} // extern "C"
