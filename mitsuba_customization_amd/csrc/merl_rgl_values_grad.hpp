// merl_rgl_values_grad.hpp — what ONE unit adds to the gradient of eval in the measured values of an RGB RGL material
// (include/merl_hip_fit_rgl.h), and the record -> texel map of the fold: the functions the kernels of
// merl_rgl_values_grad.hip run, __host__ __device__ and free of HIP calls so that a host harness can run them.
//
// eval rounds  V_c = sum_k ws_k sum_j wc_j R[slice_k][c][corner_j],  E_c = max(0, V_c) J  (merl_rgl.hpp, eval_pdf_at), so
//     d E_c / d R[slice_k][c][corner_j] = [V_c >= 0] J ws_k wc_j
// in the cell eval selects.  Nothing of that selection is restated: the bracket and the slice weights are find_slices' (through
// incident), the position in the values table is warp_invert's (through half_lookup), the cell and its fractions are locate's, the
// clamp mask is the sign of cell_value(blend4(fetch_raw)) per channel — the very value eval clamps — and J is value_scale.  The
// three factors stay apart (a_c = g_c [V_c >= 0] J, the slice weights, the corner weights): the lanes of the scatter kernel form the
// products a_c ws_k wc_j in f64, one per slot of the unit's gradient brick.
// Gradient brick of (bracket, cell): slot (c S + k) 4 + j for channel c, slice k of the bracket's S = 1 / 2 / 4 (phi fastest, the
// order of the value bricks' float4s) and corner j = (v00, v10, v01, v11) — 12 S doubles, padded to 16 S (128 / 256 / 512 B).
#pragma once
#include "merl_rgl.hpp"

namespace mrl {
namespace rgl {

// the brackets and cells of a file's values table: its gradient bricks
MRL_HD size_t values_records(int n_phi, int n_theta, int nx, int ny)
{
    const size_t tb = n_theta > 1 ? (size_t)(n_theta - 1) : 1, pb = n_phi > 1 ? (size_t)(n_phi - 1) : 1;
    return pb * tb * (size_t)(nx - 1) * (size_t)(ny - 1);
}

struct ValuesGradUnit {
    bool live;          // false: eval's guard masks the unit — nothing was read, every factor is 0
    int slices;         // S of the material's brackets
    unsigned record;    // bracket x cells + cell: the unit's gradient brick (and value brick)
    unsigned ip, it;    // the bracket's first parameter nodes (the plain form's slices)
    int ox, oy;         // the cell's first node column / row
    double a[3];        // g_c [V_c >= 0] J
    double ws[4];       // the slice weights, compact: in the order of the brick's slices
    double wc[4];       // the corner weights of (v00, v10, v01, v11)
};

// MASK: the bracket shape when the caller knows it at compile time (1, 3, 5, 15), 0: tested at run time — the same operations
// either way.  A dead unit — eval's guard: wi.z <= 0, wo.z <= 0, a NaN / inf component, a failed normalisation — returns zeros
// whatever g32 holds.
template <int MASK = 0, class Grids>
MRL_HD ValuesGradUnit values_grad_unit(const RglDev &b, const Grids &g, float wix, float wiy, float wiz, float wox, float woy, float woz, const float g32[3])
{
#pragma clang fp contract(off)
    ValuesGradUnit u;
    u.live = false; u.slices = b.slices(); u.record = 0u; u.ip = u.it = 0u; u.ox = u.oy = 0;
    for (int k = 0; k < 3; ++k) u.a[k] = 0.0;
    for (int k = 0; k < 4; ++k) u.ws[k] = u.wc[k] = 0.0;
    const float nf = ((wix - wix) + (wiy - wiy)) + ((wiz - wiz) + (wox - wox)) + ((woy - woy) + (woz - woz));      // 0, or NaN
    if (!(wiz > 0.0f) || !(woz > 0.0f) || !(nf == 0.0f)) return u;
    Incident in;
    if (!incident<true>(b, g, wix, wiy, wiz, in)) return u;
    if constexpr (MASK != 0) in.sv.mask = MASK;
    const Half h = half_lookup(b, SearchMem(b.vndf()), in, wox, woy, woz, nullptr);
    if (!h.ok) return u;
    const WarpDev wr = b.rgb();
    const Cell c = locate(wr, h.sx, h.sy);
    // the three channels' vectors go out together; the jacobian's two cells are read while they are in flight
    Raw4 raw[3];
    for (int k = 0; k < 3; ++k) raw[k] = fetch_raw(in.sv, wr, c.index, k);
    const double scale = value_scale(b, in, h);
    for (int k = 0; k < 3; ++k) {
        const double v = cell_value(wr, c, blend4(in.sv, raw[k]));
        u.a[k] = v < 0.0 ? 0.0 : (double)g32[k] * scale;
    }
    // the bracket's slices in the order the bricks hold them (fetch_raw's: an absent phi neighbour moves the theta neighbour up)
    const Slices &s = in.sv;
    // (selects, not an index that runs: the factors stay in registers where the shape is tested at run time)
    u.ws[0] = s.w[0];
    u.ws[1] = (s.mask & 2) ? s.w[1] : ((s.mask & 4) ? s.w[2] : 0.0);
    u.ws[2] = (s.mask & 8) ? s.w[2] : 0.0;
    u.ws[3] = (s.mask & 8) ? s.w[3] : 0.0;
    // bilinear()'s weights of the four corners
    u.wc[0] = (1.0 - c.fy) * (1.0 - c.fx); u.wc[1] = (1.0 - c.fy) * c.fx; u.wc[2] = c.fy * (1.0 - c.fx); u.wc[3] = c.fy * c.fx;
    const unsigned per_c = (unsigned)((wr.nx - 1) * (wr.ny - 1));
    const unsigned tbr = (unsigned)(b.n_theta > 1 ? b.n_theta - 1 : 1), ib = s.cell0 / per_c;
    u.ip = ib / tbr; u.it = ib - u.ip * tbr;
    u.record = s.cell0 + (unsigned)c.index;
    u.ox = c.ox; u.oy = c.oy;
    u.live = true;
    return u;
}

// slot -> its value: the product of the unit's three factors, formed in f64
MRL_HD double values_slot_term(const double a[3], const double ws[4], const double wc[4], int slices, int slot)
{
#pragma clang fp contract(off)
    const int j = slot & 3, k = (slot >> 2) % slices, c = (slot >> 2) / slices;
    return a[c] * ws[k] * wc[j];
}

// The planar texel a brick slot belongs to — append_warp's copy rule (merl_rgl.hip) read backwards.  Texel (ip, it, c, y, x) of
// [n_phi][n_theta][3][ny][nx] is corner (dy, dx) of cell (y - dy, x - dx) in every bracket (ip - dp, it - dt) it bounds, as the
// bracket's slice dp + 2 dt (dt when the file has one phi node).  fold_sources lists those slots in a FIXED order (dp, dt, dy, dx
// ascending): the fold is deterministic.  Returns their number (at most 16); out[k]: offsets in doubles from the target's first brick.
MRL_HD int fold_sources(int n_phi, int n_theta, int nx, int ny, int ip, int it, int c, int y, int x, size_t out[16])
{
    const int tb = n_theta > 1 ? n_theta - 1 : 1, pb = n_phi > 1 ? n_phi - 1 : 1;
    const int S = (n_phi > 1 ? 2 : 1) * (n_theta > 1 ? 2 : 1);
    const size_t cells = (size_t)(nx - 1) * (size_t)(ny - 1);
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
                    out[n++] = record * (size_t)(16 * S) + (size_t)((c * S + slice) * 4 + 2 * dy + dx);
                }
        }
    return n;
}

// the planar texel of the plain form: slot (c, compact slice k, corner j) of a unit -> index into [n_phi][n_theta][3][ny][nx]
MRL_HD size_t values_texel(const RglDev &b, const ValuesGradUnit &u, int c, int k, int j)
{
    // compact slice k -> (dp, dt): phi fastest where the file has more than one phi node
    const int dp = b.n_phi > 1 ? (k & 1) : 0, dt = b.n_phi > 1 ? (k >> 1) : k;
    const size_t slice = (size_t)(u.ip + (unsigned)dp) * (size_t)b.n_theta + (size_t)(u.it + (unsigned)dt);
    return ((slice * 3 + (size_t)c) * (size_t)b.ny + (size_t)(u.oy + (j >> 1))) * (size_t)b.nx + (size_t)(u.ox + (j & 1));
}

} // namespace rgl
} // namespace mrl
