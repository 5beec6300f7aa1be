// merl_ggx_grad_mat.hip — the parameter gradient of eval on GGX conductors with a material id per unit and over wavefront queues,
// onto up to 16 target materials in one launch (include/merl_hip_fit_ggx.h, mrl_ggx_grad_batch_mat / mrl_ggx_grad_queue; DESIGN.md
// §5m).  The per-unit math is that of merl_ggx_grad.hip (fast::ggx_eval_jacobian, the same selects and FMA chains, contraction off);
// what differs is the reduction: one lane's units belong to different targets, so the sum is a segmented one.
//   k_ggx_grad_mat<NORMAL, PER_LANE, INDEXED>   persistent grid, one lane = one unit per round.  A wave holds register accumulators
//                        for ONE wave-uniform "current" target and a private block of LDS rows [targets][kRow].  The targets present
//                        in a round are taken in ascending order; a round whose only target is the current one just accumulates
//                        (a queue partitioned by material runs at the single-material rate); any other target first flushes the
//                        registers — a reduce-scatter over the wave, one add into the current target's LDS row — and becomes the
//                        current one.  At the
//                        end the four waves' rows are added in wave order and written with plain stores: one row per block and target
//   k_ggx_grad_mat_sum   one block per target: its rows summed in a fixed order and added to that target's outputs, unless no unit
//                        named the target (column kNamedCol of the rows counts the waves that met it)
// No atomics and nothing to clear in memory: every row is written before it is read.
#include "merl_ctx.hpp"
#include "../../include/merl_hip_fit_ggx.h"
#include "merl_ggx_fast.hpp"
#include "merl_ggx_grad.hpp"
#include "merl_unit.hpp"

namespace mrl {

namespace {

constexpr int kMatBlock = 256;
constexpr int kMatWaves = kMatBlock / 64;
// One grid for all instantiations: grad_params must not depend on whether `normal` is asked for.  The gradient + normal kernels
// stay below 168 VGPRs (launch bounds below): three waves per SIMD are resident, as in merl_ggx_grad.hip; 3 x 16 KB of LDS per CU.
constexpr int kMatBlocksPerCu = 3;
constexpr int kMaxTargets = MRL_GGX_GRAD_MAX_TARGETS;
constexpr int kNamedCol = kRow - 1;      // of a row: how many waves met a unit that names the target (0: the outputs are left alone)
constexpr int kMatSumBlock = 1024;
constexpr int kMatSumGroups = kMatSumBlock / kRow;

struct GgxGradMatOut {
    const float *g, *h;                  // [n][3]; h: nullptr = 1
    int n_targets;
    int single_slot;                     // a launch without ids: the target its one material is, or -1
    int32_t ids[kMaxTargets];            // the targets, by value: a queue call reads nothing from host memory
    double *partials;                    // [grid][n_targets][kRow]
};

template <bool NORMAL, bool PER_LANE, bool INDEXED>
__global__ __launch_bounds__(kMatBlock, kMatBlocksPerCu) void k_ggx_grad_mat(BatchArgs a, GgxGradMatOut o)
{
#pragma clang fp contract(off)
    constexpr int K = kParams + (NORMAL ? kNormalTerms : 0);
    __shared__ double s_rows[kMatWaves][kMaxTargets * kRow];
    const unsigned t = threadIdx.x, lane = t & 63u, wave = t >> 6;
    double *row = s_rows[wave];
    const int n_rows = o.n_targets * kRow;
    for (int e = (int)lane; e < n_rows; e += 64) row[e] = 0.0;
    __syncthreads();

    double acc[K];
#pragma unroll
    for (int k = 0; k < K; ++k) acc[k] = 0.0;
    int cur = -1;                        // wave-uniform: the target the registers hold
    unsigned named = 0;                  // wave-uniform: the targets some unit of this wave named
    // The registers into the current target's row, as a reduce-scatter: the K terms are padded to P = 8 or 32; at every step a lane
    // keeps one half of the terms it still holds, hands the other half to its xor partner and adds what the partner hands over,
    // so the data moved halves with the lanes summed — 32 (10) cross-lane moves of an f64 where K butterflies take 138 (42).
    // Once one term is left (summed over 2 P lanes) a butterfly finishes it: term t ends in the lanes t * (64 / P) ..., and the
    // first of them adds it into the row.  The order of every sum depends on nothing
    auto flush = [&]() {
        constexpr int P = NORMAL ? 32 : 8;
#pragma unroll
        for (int step = 0; (P >> 1 >> step) >= 1; ++step) {
            const int len = P >> 1 >> step;
            const unsigned off = 32u >> step;
            const bool up = (lane & off) != 0u;
#pragma unroll
            for (int i = 0; i < len; ++i) {
                const double lo = acc[i], hi = i + len < K ? acc[i + len < K ? i + len : 0] : 0.0;
                const double send = up ? lo : hi, keep = up ? hi : lo;
                acc[i] = keep + __shfl_xor(send, (int)off, 64);
            }
        }
#pragma unroll
        for (int off = 64 / P / 2; off >= 1; off >>= 1) acc[0] += __shfl_xor(acc[0], off, 64);
        const unsigned term = lane / (64u / P);
        if (lane % (64u / P) == 0u && term < (unsigned)K) row[cur * kRow + (int)term] += acc[0];
#pragma unroll
        for (int k = 0; k < K; ++k) acc[k] = 0.0;
    };

    const bool has_h = o.h != nullptr;
    const size_t stride = (size_t)gridDim.x * kMatBlock;
    const size_t n_items = item_count<INDEXED>(a);
    for (size_t base = (size_t)blockIdx.x * kMatBlock; base < n_items; base += stride) {
        const size_t j = base + t;
        const bool active = j < n_items;
        size_t i = 0;
        int slot = -1;
        // the lane's material; a lane without a target evaluates a constant one and adds nothing.  Selected per lane in the
        // single-material launch as well: constants derived once per launch would be held in registers across the loop, and the
        // kernel would no longer fit the registers of three waves per SIMD
        MaterialDev m;
        m.alpha = 0.5;
#pragma unroll
        for (int c = 0; c < 3; ++c) { m.eta[c] = 1.5; m.k[c] = 1.0; }
        if (active) {
            i = INDEXED ? (size_t)a.idx[j] : j;
            if constexpr (PER_LANE) {
                const int id = a.mat[i];
#pragma unroll
                for (int q = 0; q < kMaxTargets; ++q)
                    if (q < o.n_targets && id == o.ids[q]) slot = q;
                // a target is a live GGX material (checked by the host): its record is in range
                const MaterialDev &rec = id_material(a, slot >= 0 ? id : 0).m;
                if (slot >= 0) {
                    m.alpha = rec.alpha;
#pragma unroll
                    for (int c = 0; c < 3; ++c) { m.eta[c] = rec.eta[c]; m.k[c] = rec.k[c]; }
                }
            } else {
                slot = o.single_slot;
                if (slot >= 0) {
                    m.alpha = a.single.alpha;
#pragma unroll
                    for (int c = 0; c < 3; ++c) { m.eta[c] = a.single.eta[c]; m.k[c] = a.single.k[c]; }
                }
            }
        }
        // the targets present in this wave's round, a wave-uniform mask
        unsigned todo = 0;
        if constexpr (PER_LANE) {
#pragma unroll
            for (int q = 0; q < kMaxTargets; ++q)
                if (q < o.n_targets && __ballot(slot == q) != 0ull) todo |= 1u << q;
        } else {
            if (o.single_slot >= 0 && __ballot(slot >= 0) != 0ull) todo = 1u << o.single_slot;
        }
        if (todo == 0) continue;
        named |= todo;

        float wix = 0.0f, wiy = 0.0f, wiz = 0.0f, wox = 0.0f, woy = 0.0f, woz = 0.0f, g32[3] = { 0.0f, 0.0f, 0.0f }, h32[3] = { 1.0f, 1.0f, 1.0f };
        if (slot >= 0) {
            load3(a.wi, i, wix, wiy, wiz);
            load3(a.wo, i, wox, woy, woz);
            load3(o.g, i, g32[0], g32[1], g32[2]);
            if (NORMAL && has_h) load3(o.h, i, h32[0], h32[1], h32[2]);
        }
        const fast::GgxConsts g(m);
        // The half vector of fast::unit_sum is a sum of two products (component x length^-1 of either direction) that sits outside
        // any contraction pragma: one product of each component is fused into the sum, and WHICH one depends on the code around
        // it.  In k_ggx_grad it is the incident one for x and y and the outgoing one for z; here, left alone, the outgoing one for
        // all three — an ulp in the half vector, 1e-10 of the scale of the sums of a smooth material.  The three products that
        // k_ggx_grad rounds are therefore made opaque, so that a unit's terms have the same bits in both kernels
        fast::Vec3 in = fast::normalize_f32(wix, wiy, wiz), out = fast::normalize_f32(wox, woy, woz);
        asm volatile("" : "+v"(in.z), "+v"(out.x), "+v"(out.y));
        const fast::GgxJacobian jac = fast::ggx_eval_jacobian(g, m.eta, m.k, in, out);
        // what eval masks, and where its D / G1 selects return 0: removed by selects — the Jacobian of such a unit is garbage and
        // its g and h may be NaN
        const float poison = fast::cos_or_nan32((wix + wiy + wiz), wox, woy, woz, true);
        const bool live = (wiz > 0.0f) && (woz > 0.0f) && (poison == poison) && jac.live;

        // ascending over the targets present; the chain below is k_ggx_grad's, `on` in the place of its `live`
        for (;;) {
            const int s = __builtin_ctz(todo);
            todo &= todo - 1;
            if (s != cur) {
                if (cur >= 0) flush();
                cur = s;
            }
            const bool on = live && slot == s;
            double sum_a = 0.0, sum_aa = 0.0;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const double gc = on ? (double)g32[c] : 0.0;
                const double ja = on ? jac.d_alpha[c] : 0.0, je = on ? jac.d_eta[c] : 0.0, jk = on ? jac.d_k[c] : 0.0;
                sum_a = __builtin_fma(gc, ja, sum_a);
                acc[1 + c] = __builtin_fma(gc, je, acc[1 + c]);
                acc[4 + c] = __builtin_fma(gc, jk, acc[4 + c]);
                if constexpr (NORMAL) {
                    const double hc = on ? (double)h32[c] : 0.0;
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
            if (todo == 0) break;
        }
    }
    if (cur >= 0) flush();
    if (lane < (unsigned)o.n_targets) row[(int)lane * kRow + kNamedCol] = (named >> lane) & 1u ? 1.0 : 0.0;
    __syncthreads();
    double *out = o.partials + (size_t)blockIdx.x * (size_t)n_rows;
    for (int e = (int)t; e < n_rows; e += kMatBlock) {
        double s = s_rows[0][e];
#pragma unroll
        for (int w = 1; w < kMatWaves; ++w) s += s_rows[w][e];
        out[e] = s;
    }
}

// block = target.  terms: kParams, or kParams + kNormalTerms (then `normal` is written, both triangles).  Thread (group, column)
// sums the rows group, group + kMatSumGroups, ... of its column of this target; the groups are then summed in order.  A target no
// unit named is left alone.  named (may be null): [n_targets], += the target's count of kNamedCol — the host-array path's record
__global__ __launch_bounds__(kMatSumBlock) void k_ggx_grad_mat_sum(const double *partials, unsigned rows, int n_targets, int terms, double *grad,
                                                                   double *normal, double *named)
{
    __shared__ double s_sum[kMatSumGroups][kRow + 1];
    __shared__ double s_total[kRow];
    const unsigned t = threadIdx.x, col = t % kRow, group = t / kRow, target = blockIdx.x;
    double acc = 0.0;
    if (col < (unsigned)terms || col == (unsigned)kNamedCol)
        for (unsigned r = group; r < rows; r += kMatSumGroups) acc += partials[((size_t)r * n_targets + target) * kRow + col];
    s_sum[group][col] = acc;
    __syncthreads();
    if (t < (unsigned)kRow) {
        double total = s_sum[0][t];
        for (int q = 1; q < kMatSumGroups; ++q) total += s_sum[q][t];
        s_total[t] = total;
    }
    __syncthreads();
    if (s_total[kNamedCol] == 0.0) return;
    if (t < (unsigned)terms) {
        const double total = s_total[t];
        if (t < (unsigned)kParams) {
            grad[target * kParams + t] += total;
        } else {
            int ea, eb;
            normal_entry((int)t - kParams, ea, eb);
            double *nm = normal + (size_t)target * kParams * kParams;
            nm[ea * kParams + eb] += total;
            if (ea != eb) nm[eb * kParams + ea] += total;
        }
    }
    if (named && t == (unsigned)kNamedCol) named[target] += s_total[kNamedCol];
}

size_t ggx_grad_mat_max_blocks(int compute_units) { return (size_t)std::max(compute_units, 1) * kMatBlocksPerCu; }

// per target of a host-array call: grad[kParams] | normal[kParams][kParams]; behind all targets: named[kMaxTargets]
constexpr int kSumsPerTarget = kParams + kParams * kParams;
constexpr int kHostSums = kMaxTargets * kSumsPerTarget + kMaxTargets;

// the rows the largest grid writes at the most targets, and behind them the sums of a host-array call.  One size whatever the call:
// the buffer never moves once it is there, so that pointers captured in a graph stay valid
size_t ggx_grad_mat_workspace_bytes(int compute_units)
{
    return (ggx_grad_mat_max_blocks(compute_units) * kMaxTargets * kRow + kHostSums) * sizeof(double);
}

// grad (+ normal, unless nullptr) += the targets' sums over a's units; device pointers.  a.mat: an id per unit; a.idx: a queue
hipError_t launch_ggx_grad_mat(const BatchArgs &a, const GgxGradMatOut &o, double *grad, double *normal, double *named, int compute_units,
                               hipStream_t stream)
{
    const dim3 grid(grid_blocks(a.n, kMatBlock, ggx_grad_mat_max_blocks(compute_units))), block(kMatBlock);
    with_flags([&](auto with_normal, auto per_lane, auto indexed) {
        hipLaunchKernelGGL((k_ggx_grad_mat<with_normal, per_lane, indexed>), grid, block, 0, stream, a, o);
    }, normal != nullptr, a.mat != nullptr, a.idx != nullptr);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_ggx_grad_mat_sum, dim3((unsigned)o.n_targets), dim3(kMatSumBlock), 0, stream, (const double *)o.partials, grid.x,
                       o.n_targets, kParams + (normal ? kNormalTerms : 0), grad, normal, named);
    return hipGetLastError();
}

} // namespace

} // namespace mrl

using namespace mrlabi;

namespace {

// mrl_ggx_grad_batch_mat / mrl_ggx_grad_queue (include/merl_hip_fit_ggx.h); queued: over queue[0 .. min(*queue_count, n)), n its capacity
int ggx_grad_targets(mrl_ctx *ctx, const float *wi, const float *wo, const float *grad_rgb, const float *curv_rgb, const int32_t *mat,
                     int32_t single_id, size_t n, bool queued, const uint32_t *queue, const uint32_t *queue_count, const int32_t *target_ids,
                     int n_targets, double *grad_params, double *normal)
{
    if (!ctx) return MRL_ERR_INVALID;
    MRL_GUARD(ctx);
    if (n == 0) return MRL_OK;
    StreamList streams = { { (void *)wi, 12, false, "wi" }, { (void *)wo, 12, false, "wo" }, { (void *)grad_rgb, 12, false, "grad_rgb" } };
    if (first_null(streams) || !grad_params || !target_ids || (queued && (!queue || !queue_count))) return fail(ctx, MRL_ERR_INVALID, "null array argument");
    int at_h = -1, at_mat = -1;
    if (curv_rgb) { at_h = (int)streams.size(); streams.push_back({ (void *)curv_rgb, 12, false, "curv_rgb" }); }
    if (mat) { at_mat = (int)streams.size(); streams.push_back({ (void *)mat, 4, false, "mat" }); }
    if (n_targets < 1 || n_targets > MRL_GGX_GRAD_MAX_TARGETS)
        return fail(ctx, MRL_ERR_INVALID, "n_targets must be 1.." + std::to_string(MRL_GGX_GRAD_MAX_TARGETS));
    mrl::GgxGradMatOut o;
    std::memset(&o, 0, sizeof o);
    o.n_targets = n_targets;
    o.single_slot = -1;
    for (int k = 0; k < mrl::kMaxTargets; ++k) o.ids[k] = -1;
    for (int k = 0; k < n_targets; ++k) {
        const int32_t id = target_ids[k];
        if (id < 0 || (size_t)id >= ctx->materials.size() || ctx->materials[(size_t)id].released) return fail(ctx, MRL_ERR_MATERIAL, "unknown material id");
        if (ctx->materials[(size_t)id].dev.kind != mrl::KIND_GGX)
            return fail(ctx, MRL_ERR_MATERIAL, "the parameter gradient is defined for GGX conductor materials");
        for (int j = 0; j < k; ++j)
            if (target_ids[j] == id) return fail(ctx, MRL_ERR_INVALID, "a material is listed twice among the targets");
        o.ids[k] = id;
        if (!mat && id == single_id) o.single_slot = k;
    }
    if (queued && n > ((size_t)1 << 32)) return fail(ctx, MRL_ERR_INVALID, "queue capacity exceeds 2^32 (indices are uint32)");
    MRL_HIP(ctx, hipSetDevice(ctx->device));
    const int kind = queued ? common_kind({ grad_params, normal, queue, queue_count }, streams) : common_kind({ grad_params, normal }, streams);
    if (queued && kind != 1) return fail(ctx, MRL_ERR_POINTER_MIX, "queue calls take device pointers only");
    if (kind < 0) return fail(ctx, MRL_ERR_POINTER_MIX, "host and device pointers mixed in one call");

    DeviceBuf &work = ctx->buf[mrl_ctx::BUF_GGX_GRAD_MAT];
    const int rc = work.reserve(ctx, mrl::ggx_grad_mat_workspace_bytes(ctx->compute_units));
    if (rc != MRL_OK) return rc;
    o.partials = (double *)work.p;
    mrl::BatchArgs a;
    std::memset(&a, 0, sizeof a);
    a.materials = ctx->d_materials;
    a.n_materials = (int)ctx->materials.size();
    a.safe = tombstone_dev(ctx);
    if (!mat && o.single_slot >= 0) a.single = ctx->materials[(size_t)single_id].dev;        // else unused: no lane reads it
    a.opts = ctx->opts;
    a.idx = queue; a.idx_count = queue_count;
    if (kind == 1) {
        a.wi = wi; a.wo = wo; a.mat = mat; a.n = n;
        o.g = grad_rgb; o.h = curv_rgb;
        MRL_HIP(ctx, mrl::launch_ggx_grad_mat(a, o, grad_params, normal, nullptr, ctx->compute_units, ctx->stream));
        return MRL_OK;
    }
    // host arrays: the inputs are staged chunk by chunk, every chunk adds to one small device array, and that is added to the
    // caller's on the host
    double *d_sums = o.partials + mrl::ggx_grad_mat_max_blocks(ctx->compute_units) * mrl::kMaxTargets * mrl::kRow;
    double *d_normal = d_sums + mrl::kMaxTargets * mrl::kParams, *d_named = d_sums + mrl::kMaxTargets * mrl::kSumsPerTarget;
    std::vector<double> sums((size_t)mrl::kHostSums);
    MRL_HIP(ctx, hipMemsetAsync(d_sums, 0, sums.size() * sizeof(double), ctx->stream));
    const int rs = run_host_staged(ctx, streams, n, 0, [&](char *const *addr, size_t m) -> int {
        a.wi = (const float *)addr[0]; a.wo = (const float *)addr[1]; a.n = m;
        o.g = (const float *)addr[2];
        o.h = at_h >= 0 ? (const float *)addr[at_h] : nullptr;
        a.mat = at_mat >= 0 ? (const int32_t *)addr[at_mat] : nullptr;
        MRL_HIP(ctx, mrl::launch_ggx_grad_mat(a, o, d_sums, normal ? d_normal : nullptr, d_named, ctx->compute_units, ctx->stream));
        return MRL_OK;
    });
    if (rs != MRL_OK) { (void)hipStreamSynchronize(ctx->stream); return rs; }
    MRL_HIP(ctx, hipMemcpyAsync(sums.data(), d_sums, sums.size() * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    MRL_HIP(ctx, hipStreamSynchronize(ctx->stream));
    for (int t = 0; t < n_targets; ++t) {
        if (sums[(size_t)(mrl::kMaxTargets * mrl::kSumsPerTarget + t)] == 0.0) continue;      // no unit named it: its rows keep their bits
        for (int k = 0; k < mrl::kParams; ++k) grad_params[t * mrl::kParams + k] += sums[(size_t)(t * mrl::kParams + k)];
        if (!normal) continue;
        const double *src = sums.data() + mrl::kMaxTargets * mrl::kParams + (size_t)t * mrl::kParams * mrl::kParams;
        double *dst = normal + (size_t)t * mrl::kParams * mrl::kParams;
        for (int j = 0; j < mrl::kNormalTerms; ++j) {
            int ea, eb;
            mrl::normal_entry(j, ea, eb);
            dst[ea * mrl::kParams + eb] += src[ea * mrl::kParams + eb];
            if (ea != eb) dst[eb * mrl::kParams + ea] += src[eb * mrl::kParams + ea];
        }
    }
    return MRL_OK;
}

} // namespace

extern "C" {

int mrl_ggx_grad_batch_mat(mrl_ctx *ctx, const float *wi, const float *wo, const float *grad_rgb, const float *curv_rgb, const int32_t *mat,
                           int32_t single_id, size_t n, const int32_t *target_ids, int n_targets, double *grad_params, double *normal)
{
    return ggx_grad_targets(ctx, wi, wo, grad_rgb, curv_rgb, mat, single_id, n, false, nullptr, nullptr, target_ids, n_targets, grad_params, normal);
}

int mrl_ggx_grad_queue(mrl_ctx *ctx, const float *wi, const float *wo, const float *grad_rgb, const float *curv_rgb, const int32_t *mat,
                       int32_t single_id, const uint32_t *queue, const uint32_t *queue_count, size_t capacity, const int32_t *target_ids,
                       int n_targets, double *grad_params, double *normal)
{
    return ggx_grad_targets(ctx, wi, wo, grad_rgb, curv_rgb, mat, single_id, capacity, true, queue, queue_count, target_ids, n_targets,
                            grad_params, normal);
}

} // extern "C"
