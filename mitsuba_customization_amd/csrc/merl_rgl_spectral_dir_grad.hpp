// merl_rgl_spectral_dir_grad.hpp — the per-lane gradient of eval in the directions AND in the wavelengths on a spectral RGL material
// (include/merl_hip_diff_rgl_spectral.h): the function k_rgl_spectral_dir_grad runs, __host__ __device__ and free of
// HIP calls so that a host harness can run it.
//
// E_k(wi, wo, lambda_k) of merl_rgl.hpp's eval_pdf_spectral_at / spectrum_at, as a real-valued function: everything up to the cell
// of (sx, sy) in the values table and the factor ndf / (4 sigma) is the RGB function's (dir_grad_core of merl_rgl_dir_grad.hpp:
// stages 1 - 3 and step 4); the channel stage is this file's.  Per wavelength k of the unit:
//   the node bracket [c0, c0 + 1] of lambda_k (eval's search, through Grids), t_k its clamped position, d t / d lambda = 1 / (l1 - l0)
//   or 0 while the clamp is active;
//   both nodes' corner vectors, read together; each node's (v, d / d fx, d / d fy, d / d tp, d / d tt) — node_terms, the RGB
//   channel's operations —, the five interpolated with t_k (eval's lerp: the value's bits are eval's, so is the clamp decision);
//   V_k = max(0, v): a clamped wavelength joins no sum and its grad_wavelengths is 0;
//   (W, W_fx, W_fy, W_tp, W_tt) += g_k (...), one ascending FMA chain each;
//   grad_wavelengths[k] = g_k scale (v1 - v0) d t / d lambda, v1 - v0 the bilinear value of the corner differences formed per slice
//   in f64 before any weight meets them (blend4_diff) — written inside the loop, no register array.
// wl == nullptr (the file's own nodes, channel k = node k): the per-channel operations are exactly eval_dir_grad's, so a 3-node file
// that holds an RGB file's arrays returns mrl_rgl_grad_dir_batch's bits.
// g and lambda are read per lane, one dword per wavelength (rows are 4-byte aligned only: W = 7).  Contraction is off and the FMAs
// are spelt out: a unit's bits do not depend on the kernel it is inlined into.
#pragma once
#include "merl_rgl_dir_grad.hpp"

namespace mrl {
namespace rgl {

// sum_s w_s (r1_s - r0_s), corner by corner: the difference of two stored Floats per slice in f64, then the slice weights
MRL_HD D4 blend4_diff(const Slices &s, const Raw4 &r0, const Raw4 &r1)
{
#pragma clang fp contract(off)
    auto d = [](float b, float a) { return (double)b - (double)a; };
    D4 v = { s.w[0] * d(r1.q0.x, r0.q0.x), s.w[0] * d(r1.q0.y, r0.q0.y), s.w[0] * d(r1.q0.z, r0.q0.z), s.w[0] * d(r1.q0.w, r0.q0.w) };
    auto add = [&](double w, const float4 &b, const float4 &a) {
        v.x = __builtin_fma(w, d(b.x, a.x), v.x); v.y = __builtin_fma(w, d(b.y, a.y), v.y);
        v.z = __builtin_fma(w, d(b.z, a.z), v.z); v.w = __builtin_fma(w, d(b.w, a.w), v.w);
    };
    if (s.mask & 2) add(s.w[1], r1.q1, r0.q1);
    if (s.mask & 4) add(s.w[2], r1.q2, r0.q2);
    if (s.mask & 8) add(s.w[3], r1.q3, r0.q3);
    return v;
}

// nothing is formed from r before x is complete (device code): the three uses of a wavelength's two nodes — their difference, the
// lower node's terms, the upper node's — follow one another, so that their f64 conversions are not all live at once (side by side
// they spilled 88 - 96 B per lane on the isotropic shapes at two waves per SIMD).  MASK: the slices a bracket of that shape has (0:
// not known, all four): an absent slice's zeros stay constants.  settled: the whole of a node's terms before the next stage starts.
MRL_HD void not_before(float4 &q, double &x)
{
#if defined(__HIP_DEVICE_COMPILE__)
    asm volatile("" : "+v"(q.x), "+v"(q.y), "+v"(q.z), "+v"(q.w), "+v"(x));
#else
    (void)q; (void)x;
#endif
}
MRL_HD void settled(NodeTerms &n)
{
#if defined(__HIP_DEVICE_COMPILE__)
    asm volatile("" : "+v"(n.v), "+v"(n.fx), "+v"(n.fy), "+v"(n.tp), "+v"(n.tt));
#else
    (void)n;
#endif
}
template <int MASK>
MRL_HD void not_before(Raw4 &r, double &x)
{
    not_before(r.q0, x);
    if constexpr (MASK == 0 || (MASK & 2)) not_before(r.q1, x);
    if constexpr (MASK == 0 || (MASK & 4)) not_before(r.q2, x);
    if constexpr (MASK == 0 || (MASK & 8)) not_before(r.q3, x);
}

// grad_wi = sum_k g_k dE_k / d wi, grad_wo, and grad_wl[k] = g_k dE_k / d lambda_k (grad_wl may be null) of ONE unit on the spectral
// RGL material b.  g_row, wl_row, grad_wl: the unit's rows of W values (wl_row == nullptr: the file's own nodes, W == b.n_wl, grad_wl
// null).  Dead units return +0.0f everywhere, their whole grad_wl row included, whatever g_row and wl_row hold.  MASK, Grids: as
// eval_dir_grad; Grids::wavelength_at serves the bracket search.
template <int MASK = 0, class Grids>
MRL_HD RglDirGrad eval_dir_grad_spectral(const RglDev &b, const Grids &g, float wix, float wiy, float wiz, float wox, float woy, float woz,
                                         const float *g_row, const float *wl_row, int W, float *grad_wl)
{
#pragma clang fp contract(off)
    RglDirGrad out;
    const bool alive = dir_grad_core<MASK>(b, g, wix, wiy, wiz, wox, woy, woz, out,
        [&](const WarpDev &wr, const Cell &c, const Slices &sv, const Slices &sp, const Slices &st, double scale, ChannelSums &a) {
            // two nodes per wavelength, or one: the file's own nodes (channel k IS node k), a file with one node
            const int n_wl = b.n_wl;
            const bool two = wl_row && n_wl > 1;
#pragma nounroll
            for (int k = 0; k < W; ++k) {
                const float gf = g_row[k];
                int c0 = wl_row ? 0 : k;
                double t = 0.0, dt = 0.0;
                if (two) {
                    // eval's bracket (bracket_by of merl_rgl.hpp), and the slope of t
                    const double lambda = (double)wl_row[k];
                    int hi = n_wl - 1;
                    while (hi - c0 > 1) { const int mid = (c0 + hi) >> 1; if ((double)g.wavelength_at(mid) <= lambda) c0 = mid; else hi = mid; }
                    bracket_slope(g.wavelength_at(c0), g.wavelength_at(c0 + 1), lambda, t, dt);
                    dt = t == t ? dt : 0.0;                         // a NaN wavelength: E_k is no number, its derivative is written as 0
                }
                Raw4 r0 = fetch_raw(sv, wr, c.index, c0), r1 = r0;
                if (two) r1 = fetch_raw(sv, wr, c.index, c0 + 1);
                not_before_here(r0);
                double dv = 0.0;
                if (two) {
                    not_before_here(r1);
                    dv = bilinear(blend4_diff(sv, r0, r1), c.fx, c.fy);
                    not_before<MASK>(r0, dv);
                }
                // one node: the RGB function's channel, operation by operation
                NodeTerms n = node_terms(sv, sp, st, c, r0);
                if (two) {
                    settled(n);
                    not_before<MASK>(r1, n.v);
                    const NodeTerms n1 = node_terms(sv, sp, st, c, r1);
                    n.v = lerp(t, n.v, n1.v); n.fx = lerp(t, n.fx, n1.fx); n.fy = lerp(t, n.fy, n1.fy);
                    n.tp = lerp(t, n.tp, n1.tp); n.tt = lerp(t, n.tt, n1.tt);
                }
                const bool clamped = n.v < 0.0;
                add_channel(a, clamped ? 0.0 : (double)gf, n);
                if (grad_wl) grad_wl[k] = (clamped || dt == 0.0) ? 0.0f : fast::finite_f32((double)gf * scale * dv * dt);
            }
        });
    if (!alive && grad_wl) for (int k = 0; k < W; ++k) grad_wl[k] = 0.0f;
    return out;
}

} // namespace rgl
} // namespace mrl
