// merl_update.hip — new values for a resident material, in place (include/merl_hip_update.h): a table's image is
// rewritten from a planar array by the upload's own build kernels, its row marginal rebuilt on the device (k_marginal_partial +
// k_marginal_finish below; an upload sums it on the host), its conditional rows by the upload's kernels; a GGX conductor's
// parameters are written into its entry of the device array by a one-thread kernel.  Nothing is allocated per call: the per-material
// workspace (MaterialHost::update_ws) is sized by the material's first update and stays where it is.
#include "merl_ctx.hpp"
#include "../../include/merl_hip_update.h"

namespace {

constexpr int kUpdBlock = 256;                // 4 waves
// cells of one row that one block sums.  FIXED: which cells meet in which partial sum, and in which order the partial sums of a
// row are combined, depends on the table's dims alone — never on the grid a launch got or on the device's CU count
constexpr int kUpdSegment = 1024;

struct ChannelScales { double s[mrl::kMaxChannels]; };       // by value in the kernel arguments (256 B): uniform reads

// wave sum without an LDS round trip: five DPP / swizzle steps and one cross-half step, a fixed tree (lane 0 holds the sum)
__device__ __forceinline__ double wave_sum(double v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off);
    return v;
}

// the 4 wave sums of a block, combined in a fixed order; thread 0 holds the result.  (One 32-B exchange through LDS: waves share
// nothing else.)  Every thread of the block calls it; `part` is free for reuse after the second barrier.
__device__ __forceinline__ double block_sum(double v, double *part)
{
    v = wave_sum(v);
    const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
    __syncthreads();                                                       // earlier readers of part[] are done
    if (lane == 0) part[wave] = v;
    __syncthreads();
    return (part[0] + part[1]) + (part[2] + part[3]);
}

// Pass 1, one block per (row, segment): sum over the segment's cells k and the channels of w_ch max(v scale_ch, 0) — build_sampling /
// build_sampling_nch of merl_materials.hip, in another order.  Thread t takes cells t, t + 256, ...: consecutive lanes read
// consecutive doubles of a plane (phi_d runs fastest), n_ch coalesced streams.
template <bool LUMINANCE>
__global__ __launch_bounds__(kUpdBlock) void k_marginal_partial(const double *__restrict__ planar, int n_ch, size_t row_len, size_t plane,
                                                               unsigned n_seg, ChannelScales sc, double *__restrict__ partial)
{
    __shared__ double part[4];
    const size_t row = blockIdx.x / n_seg, seg = blockIdx.x % n_seg;
    const size_t k0 = seg * (size_t)kUpdSegment, k1 = min(k0 + (size_t)kUpdSegment, row_len);
    const double *p = planar + row * row_len;
    double acc = 0.0;
    for (size_t k = k0 + threadIdx.x; k < k1; k += kUpdBlock) {
        if (LUMINANCE) {
            const double r = p[k] * sc.s[0], g = p[k + plane] * sc.s[1], b = p[k + 2 * plane] * sc.s[2];
            acc += 0.2126 * (r > 0.0 ? r : 0.0) + 0.7152 * (g > 0.0 ? g : 0.0) + 0.0722 * (b > 0.0 ? b : 0.0);
        } else {
            double sum = 0.0;
            for (int ch = 0; ch < n_ch; ++ch) {
                const double v = p[k + (size_t)ch * plane] * sc.s[ch];
                sum += v > 0.0 ? v : 0.0;
            }
            acc += sum / (double)n_ch;
        }
    }
    const double total = block_sum(acc, part);
    if (threadIdx.x == 0) partial[blockIdx.x] = total;
}

// Pass 2, one block: per row the segments' sums in ascending order -> D; the mean; the 1 % floor, the flat lobe of the
// parameterisations whose rows are not theta_h and the all-zero case; Z and the running integral (per-thread serial chunks, a
// Hillis-Steele scan of the 256 chunk sums, as k_sampling2d_scan does) -> cdf and c.  s = sampling[0 .. n] is read, not written.
__global__ __launch_bounds__(kUpdBlock) void k_marginal_finish(const double *__restrict__ partial, unsigned n_seg, int n, double cells_per_row,
                                                              int flat, double *__restrict__ D, double *sampling)
{
    __shared__ double part[kUpdBlock];
    const int tid = (int)threadIdx.x;
    const double *s = sampling;
    double *cdf = sampling + (n + 1), *c = cdf + (n + 1);
    const int per = (n + kUpdBlock - 1) / kUpdBlock, lo = min(tid * per, n), hi = min(lo + per, n);
    double sum = 0.0;
    for (int j = lo; j < hi; ++j) {
        double acc = 0.0;
        for (unsigned g = 0; g < n_seg; ++g) acc += partial[(size_t)j * n_seg + g];
        const double d = acc / cells_per_row;
        D[j] = d;                                   // read back by this thread only
        sum += d;
    }
    double mean = block_sum(sum, part) / (double)n;
    if (flat) mean = 0.0;
    auto density = [&](int j) { return mean > 0.0 ? D[j] + 0.01 * mean : 1.0; };
    sum = 0.0;
    for (int j = lo; j < hi; ++j) sum += density(j) * (s[j + 1] - s[j]);
    __syncthreads();
    part[tid] = sum;
    __syncthreads();
    for (int off = 1; off < kUpdBlock; off <<= 1) {
        const double add = tid >= off ? part[tid - off] : 0.0;
        __syncthreads();
        part[tid] += add;
        __syncthreads();
    }
    const double Z = part[kUpdBlock - 1];
    double run = tid ? part[tid - 1] : 0.0;
    for (int j = lo; j < hi; ++j) {
        const double d = density(j);
        cdf[j] = run / Z;
        run += d * (s[j + 1] - s[j]);
        c[j] = d / (mrl::kPi * Z);
    }
    if (tid == 0) cdf[n] = 1.0;
}

__global__ void k_update_ggx(mrl::MaterialDev *m, double alpha, double e0, double e1, double e2, double k0, double k1, double k2)
{
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        m->alpha = alpha;
        m->eta[0] = e0; m->eta[1] = e1; m->eta[2] = e2;
        m->k[0] = k0; m->k[1] = k1; m->k[2] = k2;
    }
}

// the per-material workspace, in doubles: [n_th x n_seg] segment sums | [n_th] D | [n_ti x n_th] work array of the conditional rows
// (RGB tables) | [n_ch] channel scales (n-channel tables: their build kernel reads them from device memory)
struct UpdateLayout {
    unsigned n_seg;
    size_t partial, density, work2d, scales, doubles;
};
UpdateLayout update_layout(const MaterialHost &m)
{
    UpdateLayout l;
    const size_t n_th = (size_t)m.dev.n_th, row_len = (size_t)m.dev.n_td * (size_t)m.dev.n_pd;
    l.n_seg = (unsigned)((row_len + kUpdSegment - 1) / kUpdSegment);
    l.partial = 0;
    l.density = l.partial + n_th * l.n_seg;
    l.work2d = l.density + n_th;
    l.scales = l.work2d + (m.d_sampling2d ? (size_t)m.dev.n_ti * n_th : 0);
    l.doubles = l.scales + (m.dev.kind == mrl::KIND_TABLE_NCH ? (size_t)m.dev.n_ch : 0);
    return l;
}

bool live(const mrl_ctx *ctx, int id) { return id >= 0 && (size_t)id < ctx->materials.size() && !ctx->materials[(size_t)id].released; }

} // namespace

using namespace mrlabi;

extern "C" {

int mrl_material_update_table(mrl_ctx *ctx, int id, const double *planar, int flags)
{
    if (!ctx) return MRL_ERR_INVALID;
    MRL_GUARD(ctx);
    if (!planar) return fail(ctx, MRL_ERR_INVALID, "null argument");
    if (flags & ~MRL_UPDATE_KEEP_SAMPLING) return fail(ctx, MRL_ERR_INVALID, "unknown flag bits");
    if (!live(ctx, id)) return fail(ctx, MRL_ERR_MATERIAL, "unknown material id");
    MaterialHost &m = ctx->materials[(size_t)id];
    const bool rgb = m.dev.kind == mrl::KIND_MERL || m.dev.kind == mrl::KIND_TABLE, nch = m.dev.kind == mrl::KIND_TABLE_NCH;
    if (!rgb && !nch) return fail(ctx, MRL_ERR_MATERIAL, "only table materials (MERL, customized_measurement, n-channel) are updated from a planar array");
    if (rgb ? !m.has_scale : m.nch_scale.size() != (size_t)m.dev.n_ch)
        return fail(ctx, MRL_ERR_MATERIAL, "the table was restored from an image file and carries no channel scales: it cannot be rebuilt from a planar array");
    MRL_HIP(ctx, hipSetDevice(ctx->device));
    const int dims[3] = { m.dev.n_th, m.dev.n_td, m.dev.n_pd };
    const int n_ch = m.dev.n_ch;
    const size_t row_len = (size_t)dims[1] * (size_t)dims[2], plane = (size_t)dims[0] * row_len;
    const UpdateLayout l = update_layout(m);
    // the workspace: once per material (a captured update points at it afterwards)
    if (!m.update_ws.p) {
        int rc = m.update_ws.reserve(ctx, l.doubles * sizeof(double));
        if (rc != MRL_OK) return rc;
        if (nch) {
            const hipError_t e = hipMemcpy((double *)m.update_ws.p + l.scales, m.nch_scale.data(), (size_t)n_ch * sizeof(double), hipMemcpyHostToDevice);
            if (e != hipSuccess) {
                (void)hipGetLastError();
                (void)hipFree(m.update_ws.p); m.update_ws = DeviceBuf{};
                return fail(ctx, MRL_ERR_HIP, std::string("update workspace: ") + hipGetErrorString(e));
            }
        }
    }
    double *ws = (double *)m.update_ws.p;
    const bool from_host = pointer_kind(planar) == 0;
    const double *d_planar = planar;
    if (from_host) {
        const size_t bytes = (size_t)n_ch * plane * sizeof(double);
        int rc = ctx->buf[mrl_ctx::BUF_STAGE].reserve(ctx, bytes);
        if (rc != MRL_OK) return rc;
        d_planar = (const double *)ctx->buf[mrl_ctx::BUF_STAGE].p;
    }
    const ScalarPause quiet(ctx);                                // a service instance may be reading the table
    hipStream_t stream = ctx->stream;
    if (from_host) MRL_HIP(ctx, hipMemcpyAsync((void *)d_planar, planar, (size_t)n_ch * plane * sizeof(double), hipMemcpyHostToDevice, stream));
    const int clamp = ctx->opts.negative == mrl::NEGATIVE_CLAMP;
    hipError_t e;
    if (rgb) e = mrl::launch_build_table(d_planar, dims, m.scale, m.dev.layout, m.dev.param, clamp, m.d_texels, ctx->compute_units, stream);
    else     e = mrl::launch_build_table_nch(d_planar, ws + l.scales, dims, n_ch, m.dev.param, clamp, m.d_texels, ctx->compute_units, stream);
    if (e == hipSuccess && !(flags & MRL_UPDATE_KEEP_SAMPLING)) {
        ChannelScales sc;
        std::memset(&sc, 0, sizeof sc);
        for (int ch = 0; ch < n_ch; ++ch) sc.s[ch] = rgb ? m.scale[ch] : m.nch_scale[(size_t)ch];
        const dim3 grid((unsigned)((size_t)dims[0] * l.n_seg)), block(kUpdBlock);
        if (rgb) hipLaunchKernelGGL((k_marginal_partial<true>), grid, block, 0, stream, d_planar, n_ch, row_len, plane, l.n_seg, sc, ws + l.partial);
        else     hipLaunchKernelGGL((k_marginal_partial<false>), grid, block, 0, stream, d_planar, n_ch, row_len, plane, l.n_seg, sc, ws + l.partial);
        hipLaunchKernelGGL(k_marginal_finish, dim3(1), block, 0, stream, (const double *)(ws + l.partial), l.n_seg, dims[0], (double)dims[1] * (double)dims[2],
                           (int)(m.dev.param != mrl::PARAM_HALF_DIFF), ws + l.density, m.d_sampling);
        e = hipGetLastError();
        if (e == hipSuccess && m.d_sampling2d) {
            e = mrl::launch_build_sampling2d(m.dev, ctx->opts, m.dev.n_ti, m.d_sampling2d, ws + l.work2d, stream);
            if (e == hipSuccess) { m.rows_lookup = ctx->opts.lookup; m.rows_node = ctx->opts.node; }
        }
    }
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return fail(ctx, MRL_ERR_HIP, std::string("table update: ") + hipGetErrorString(e));
    }
    // who must not run ahead of the new image: the caller's source buffer (host path), and the one-unit service, which runs on a
    // stream of its own and resumes when this call returns.  Not inside a stream capture (nothing runs there)
    if (from_host || quiet.svc) {
        hipStreamCaptureStatus capturing = hipStreamCaptureStatusNone;
        if (hipStreamIsCapturing(stream, &capturing) != hipSuccess) { (void)hipGetLastError(); capturing = hipStreamCaptureStatusNone; }
        if (capturing == hipStreamCaptureStatusNone) MRL_HIP(ctx, hipStreamSynchronize(stream));
    }
    return MRL_OK;
}

int mrl_material_update_ggx(mrl_ctx *ctx, int id, float alpha, const float eta[3], const float k[3])
{
    if (!ctx || !eta || !k) return MRL_ERR_INVALID;
    MRL_GUARD(ctx);
    if (!(alpha > 0.0f)) return fail(ctx, MRL_ERR_INVALID, "alpha must be positive");
    if (!live(ctx, id) || ctx->materials[(size_t)id].dev.kind != mrl::KIND_GGX) return fail(ctx, MRL_ERR_MATERIAL, "not a live GGX material");
    MRL_HIP(ctx, hipSetDevice(ctx->device));
    const ScalarPause quiet(ctx);                                // a service instance reads the device array
    mrl::MaterialDev &d = ctx->materials[(size_t)id].dev;
    d.alpha = (double)alpha;
    for (int c = 0; c < 3; ++c) { d.eta[c] = (double)eta[c]; d.k[c] = (double)k[c]; }
    hipLaunchKernelGGL(k_update_ggx, dim3(1), dim3(64), 0, ctx->stream, ctx->d_materials + id, d.alpha, d.eta[0], d.eta[1], d.eta[2], d.k[0], d.k[1], d.k[2]);
    MRL_HIP(ctx, hipGetLastError());
    if (quiet.svc) {
        hipStreamCaptureStatus capturing = hipStreamCaptureStatusNone;
        if (hipStreamIsCapturing(ctx->stream, &capturing) != hipSuccess) { (void)hipGetLastError(); capturing = hipStreamCaptureStatusNone; }
        if (capturing == hipStreamCaptureStatusNone) MRL_HIP(ctx, hipStreamSynchronize(ctx->stream));
    }
    return MRL_OK;
}

int mrl_material_sampling(mrl_ctx *ctx, int id, double *out, size_t max_doubles)
{
    if (!ctx) return MRL_ERR_INVALID;
    MRL_GUARD(ctx);
    if (!live(ctx, id)) return fail(ctx, MRL_ERR_MATERIAL, "unknown material id");
    const MaterialHost &m = ctx->materials[(size_t)id];
    const int kind = m.dev.kind;
    if ((kind != mrl::KIND_MERL && kind != mrl::KIND_TABLE && kind != mrl::KIND_TABLE_NCH) || !m.d_sampling)
        return fail(ctx, MRL_ERR_MATERIAL, "the material has no row marginal (table materials do)");
    if (!out) return MRL_OK;
    const size_t need = 3 * (size_t)m.dev.n_th + 2;
    if (max_doubles < need) return fail(ctx, MRL_ERR_INVALID, "buffer too small");
    MRL_HIP(ctx, hipSetDevice(ctx->device));
    MRL_HIP(ctx, hipStreamSynchronize(ctx->stream));             // an update may be rewriting it
    MRL_HIP(ctx, hipMemcpy(out, m.d_sampling, need * sizeof(double), hipMemcpyDeviceToHost));
    return MRL_OK;
}

} // extern "C"
