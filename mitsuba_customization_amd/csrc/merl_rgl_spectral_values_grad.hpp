// merl_rgl_spectral_values_grad.hpp — what ONE unit adds to the gradient of eval_spectral in the spectra of a spectral RGL material
// (include/merl_hip_fit_rgl_spectral.h), and the record -> texel map of the fold: the functions the kernels of
// merl_rgl_spectral_values_grad.hip run, __host__ __device__ and free of HIP calls so that a host harness can run them.
//
// In two steps, as the kernel runs them.  spectral_values_unit: the unit's geometry, once — everything rgl::values_grad_unit
// (merl_rgl_values_grad.hpp) does up to the cell: the bracket and the slice weights (incident), the position in the values table
// (half_lookup), the cell and its fractions (locate), J (value_scale); the slice weights ws and the corner weights wc are the RGB
// function's, bit for bit.  spectral_values_pass: one wavelength k of the unit — eval's bracket [c0, c0 + 1] and t_k (bracket_by, as
// spectrum_at of merl_rgl.hpp calls it), both nodes' corner vectors (fetch_raw), the interpolated value with eval's own operations
// (cell_value, blend4, lerp: the clamp decision is eval's), and the two factors
//     a0 = g_k [v_k >= 0] J (1 - t_k)   for node c0          a1 = g_k [v_k >= 0] J t_k   for node c0 + 1
// A factor of exactly 0 means "nothing is added to that node"; t_k = 0 / 1 (a wavelength on a node or clamped to an end) zeroes the
// other node's factor whatever g_k holds, and a NaN wavelength both.  With the file's own nodes (no wavelength array) c0 = k, t_k = 0
// and a0 = g_k [v_k >= 0] J: on a 3-node file that holds an RGB file's arrays the three a0 are values_grad_unit's a[3].
// Gradient brick of (bracket, cell): slot (node S + k) 4 + j for slice k of the bracket's S = 1 / 2 / 4 (phi fastest, the order of the
// value bricks' float4s) and corner j = (v00, v10, v01, v11) — n_wl S 4 doubles, no padding; what one unit adds for one node is the
// 4 S contiguous doubles of that node.
#pragma once
#include "merl_rgl_values_grad.hpp"

namespace mrl {
namespace rgl {

struct SpectralValuesUnit {
    bool live;          // false: eval's guard masks the unit — nothing was read, every factor is 0
    int slices;         // S of the material's brackets
    unsigned record;    // bracket x cells + cell: the unit's gradient brick (and value brick)
    unsigned ip, it;    // the bracket's first parameter nodes (the plain form's slices)
    double scale;       // J
    double ws[4];       // the slice weights, compact: in the order of the brick's slices
    double wc[4];       // the corner weights of (v00, v10, v01, v11)
    Slices sv;          // the bracket as eval holds it, and the cell: what a pass reads its nodes with
    Cell c;
};

// MASK: the bracket shape when the caller knows it at compile time (1, 3, 5, 15), 0: tested at run time — the same operations
// either way.  A dead unit returns zeros.
template <int MASK = 0, class Grids>
MRL_HD SpectralValuesUnit spectral_values_unit(const RglDev &b, const Grids &g, float wix, float wiy, float wiz, float wox, float woy, float woz)
{
#pragma clang fp contract(off)
    SpectralValuesUnit u;
    u.live = false; u.slices = b.slices(); u.record = 0u; u.ip = u.it = 0u; u.scale = 0.0;
    for (int k = 0; k < 4; ++k) u.ws[k] = u.wc[k] = 0.0;
    u.sv = single_slice();
    u.c = Cell{ 0, 0, 0, 0.0, 0.0 };
    const float nf = ((wix - wix) + (wiy - wiy)) + ((wiz - wiz) + (wox - wox)) + ((woy - woy) + (woz - woz));      // 0, or NaN
    if (!(wiz > 0.0f) || !(woz > 0.0f) || !(nf == 0.0f)) return u;
    Incident in;
    if (!incident<true>(b, g, wix, wiy, wiz, in)) return u;
    if constexpr (MASK != 0) in.sv.mask = MASK;
    const Half h = half_lookup(b, SearchMem(b.vndf()), in, wox, woy, woz, nullptr);
    if (!h.ok) return u;
    const WarpDev wr = b.rgb();
    u.c = locate(wr, h.sx, h.sy);
    u.scale = value_scale(b, in, h);
    u.sv = in.sv;
    const Slices &s = in.sv;
    // the bracket's slices in the order the bricks hold them (fetch_raw's: an absent phi neighbour moves the theta neighbour up)
    u.ws[0] = s.w[0];
    u.ws[1] = (s.mask & 2) ? s.w[1] : ((s.mask & 4) ? s.w[2] : 0.0);
    u.ws[2] = (s.mask & 8) ? s.w[2] : 0.0;
    u.ws[3] = (s.mask & 8) ? s.w[3] : 0.0;
    // bilinear()'s weights of the four corners
    const Cell &c = u.c;
    u.wc[0] = (1.0 - c.fy) * (1.0 - c.fx); u.wc[1] = (1.0 - c.fy) * c.fx; u.wc[2] = c.fy * (1.0 - c.fx); u.wc[3] = c.fy * c.fx;
    const unsigned per_c = (unsigned)((wr.nx - 1) * (wr.ny - 1));
    const unsigned tbr = (unsigned)(b.n_theta > 1 ? b.n_theta - 1 : 1), ib = s.cell0 / per_c;
    u.ip = ib / tbr; u.it = ib - u.ip * tbr;
    u.record = s.cell0 + (unsigned)c.index;
    u.live = true;
    return u;
}

struct SpectralValuesPass { int c0; double a0, a1; };       // node c0 receives a0, node c0 + 1 a1; 0: nothing is added to that node

// one wavelength of a LIVE unit.  own_nodes: the call has no wavelength array — channel k is the file's node k; else lambda is the
// unit's k-th wavelength.  Grids::wavelength_at serves eval's bracket search.
template <int MASK = 0, class Grids>
MRL_HD SpectralValuesPass spectral_values_pass(const RglDev &b, const Grids &g, const SpectralValuesUnit &u, float gk, bool own_nodes, float lambda, int k)
{
#pragma clang fp contract(off)
    SpectralValuesPass p = { own_nodes ? k : 0, 0.0, 0.0 };
    const WarpDev wr = b.rgb();
    Slices sv = u.sv;
    if constexpr (MASK != 0) sv.mask = MASK;
    // spectrum_at's operations, one by one
    const bool two = !own_nodes && b.n_wl > 1;
    double t = 0.0;
    if (two) bracket_by([&g](int j) { return g.wavelength_at(j); }, b.n_wl, (double)lambda, p.c0, t);
    const Raw4 r0 = fetch_raw(sv, wr, u.c.index, p.c0), r1 = fetch_raw(sv, wr, u.c.index, two ? p.c0 + 1 : p.c0);
    double v = cell_value(wr, u.c, blend4(sv, r0));
    if (two) v = lerp(t, v, cell_value(wr, u.c, blend4(sv, r1)));
    // eval's clamp (v < 0 evaluates to 0); a NaN wavelength leaves t and v no numbers: nothing for this k
    if (v < 0.0 || !(t == t)) return p;
    // a wavelength exactly on the bracket's upper node (the file's last node): eval's quotient there is 1 or 1 - 2^-53, whichever
    // the reciprocal's last bit gives; the weights take 1 — the clamp decision above stays eval's
    if (two && lambda == g.wavelength_at(p.c0 + 1)) t = 1.0;
    const double a = (double)gk * u.scale;
    // the whole weight on one node where t sits at an end: the other node receives no term at all
    p.a0 = t == 1.0 ? 0.0 : a * (1.0 - t);
    p.a1 = t == 0.0 ? 0.0 : a * t;
    return p;
}

// slot -> its value: the product of the three factors, formed in f64
MRL_HD double spectral_values_slot_term(double a, const double ws[4], const double wc[4], int slot)
{
#pragma clang fp contract(off)
    return a * ws[slot >> 2] * wc[slot & 3];
}

// The brick slots of planar texel (ip, it, c, y, x) of [n_phi][n_theta][n_ch][ny][nx]: fold_sources of merl_rgl_values_grad.hpp with the
// channel count as a parameter and bricks of n_ch S 4 doubles (no padding) — append_warp's copy rule read backwards, in a FIXED order
// (dp, dt, dy, dx ascending).  Returns their number (at most 16); out[k]: offsets in doubles from the target's first brick.
MRL_HD int spectral_fold_sources(int n_phi, int n_theta, int nx, int ny, int n_ch, int ip, int it, int c, int y, int x, size_t out[16])
{
    const int tb = n_theta > 1 ? n_theta - 1 : 1, pb = n_phi > 1 ? n_phi - 1 : 1;
    const int S = (n_phi > 1 ? 2 : 1) * (n_theta > 1 ? 2 : 1);
    const size_t cells = (size_t)(nx - 1) * (size_t)(ny - 1), brick = (size_t)n_ch * (size_t)(4 * S);
    int n = 0;
    for (int dp = 0; dp < (n_phi > 1 ? 2 : 1); ++dp)
        for (int dt = 0; dt < (n_theta > 1 ? 2 : 1); ++dt) {
            const int ipb = ip - dp, itb = it - dt;
            if (ipb < 0 || ipb >= pb || itb < 0 || itb >= tb) continue;
            const int slice = n_phi > 1 ? dp + 2 * dt : dt;
            for (int dy = 0; dy < 2; ++dy)
                for (int dx = 0; dx < 2; ++dx) {
                    const int cy = y - dy, cx = x - dx;
                    if (cy < 0 || cy >= ny - 1 || cx < 0 || cx >= nx - 1) continue;
                    const size_t record = ((size_t)ipb * tb + itb) * cells + (size_t)cy * (size_t)(nx - 1) + (size_t)cx;
                    out[n++] = record * brick + (size_t)((c * S + slice) * 4 + 2 * dy + dx);
                }
        }
    return n;
}

// the planar texel of the plain form: (node, compact slice k, corner j) of a unit -> index into [n_phi][n_theta][n_wl][ny][nx]
MRL_HD size_t spectral_values_texel(const RglDev &b, const SpectralValuesUnit &u, int node, int k, int j)
{
    // compact slice k -> (dp, dt): phi fastest where the file has more than one phi node
    const int dp = b.n_phi > 1 ? (k & 1) : 0, dt = b.n_phi > 1 ? (k >> 1) : k;
    const size_t slice = (size_t)(u.ip + (unsigned)dp) * (size_t)b.n_theta + (size_t)(u.it + (unsigned)dt);
    return ((slice * (size_t)b.n_wl + (size_t)node) * (size_t)b.ny + (size_t)(u.c.oy + (j >> 1))) * (size_t)b.nx + (size_t)(u.c.ox + (j & 1));
}

} // namespace rgl
} // namespace mrl
