// merl_rgl_dir_grad.hpp — the per-lane gradient of eval in the directions on an RGB RGL material (include/merl_hip_diff_rgl.h,
// DESIGN.md §5p): the function k_rgl_dir_grad runs, __host__ __device__ and free of HIP calls so that a host harness can run it.
//
// E_c(wi, wo) of merl_rgl.hpp's eval_pdf_at, as a real-valued function: m = (a + b) normalised, u_m its warp coordinates,
// (sx, sy) = vndf.invert(u_m; tp, tt), V_c = max(0, rgb_c(sx, sy; tp, tt)), E_c = V_c ndf(u_m) / (4 sigma(u_wi)).  warp_invert is a
// direct cell lookup — no search —, so every step has a closed-form derivative in the cell eval selects.  Reverse mode by hand, for
// the cotangent g of the three channels:
//   1. the scalar partials of L = sum_c g_c E_c in the rgb cell's fractions and in (tp, tt): bilinear forms of the cell's corners,
//      the in-cell differences taken per slice in f64 BEFORE the slice weights meet them (blend_of, pair_diff below), the parameter
//      derivatives the same blends (blend4 / blend_pairs / blend_quad of merl_rgl.hpp) with the derivative weights
//      (-(1 - tt), (1 - tt), -tt, tt) and (-(1 - tp), -tp, (1 - tp), tp) in Slices::w;
//   2. through the inverse warp: with x, y the cell fractions, d uy / dy = lerp(y, r0, r1) = tot, d sx / dx = lerp(x, c0, c1) / tot,
//      d sx / dy carries the y-derivatives of c0, c1, `left` and `tot`; tot == 0 gives zero terms, as it gives a zero value;
//   3. the jacobian's factor ndf(u_m) / (4 sigma(u_wi)): two plain bilinear cells;
//   4. the six scalars (u_m, tp, tt, u_wi) go back to the four angles (theta_m, phi_m, theta_i, phi_i), the angles to the unit
//      vectors m and a (atan2(y, x) has the derivative (x dy - y dx) / (x^2 + y^2): no polynomial, no libm), m to a + b, and a, b
//      through the two normalisations and the +-1 factors of a symmetry-reduced file.
// Reads come in the two steps of merl_rgl.hpp: stage 1 issues everything addressable from the directions alone (the vndf record, the
// marginal below the row, the ndf cell, the sigma cell) back to back, stage 2 the three channels' vectors at the cell of (sx, sy);
// nothing is summed before its stage's reads are out.  (sx, sy) are formed with warp_invert's own expressions, so the rgb cell is
// eval's to the bit.  Where a map has no derivative (m at the normal, wi at the normal) that angle's terms are dropped by a select
// BEFORE any product.  Contraction is off and the FMAs are spelt out: a unit's bits do not depend on the kernel it is inlined into.
// Everything but step 1's channels is dir_grad_core, which the spectral function shares (merl_rgl_spectral_dir_grad.hpp, DESIGN.md
// §5q): the channel stage is a callable that fills ChannelSums; eval_dir_grad passes the three RGB channels.
#pragma once
#include "merl_rgl.hpp"
#include "merl_table_dir_grad.hpp"      // through_normalisation, finite_f32, kSingular

namespace mrl {
namespace rgl {

struct RglDirGrad { float wi[3], wo[3]; };

// The compiler may not form anything from these four vectors before this point (device code; nothing on the host).  Every Float of
// a cell meets three sets of weights, so its conversion to f64 is shared — and hoisted to where the vector arrives: all three
// channels as doubles at once are 96 registers, and the kernel spills.  A channel's vectors are pinned until its turn.
MRL_HD void not_before_here(float4 &q)
{
#if defined(__HIP_DEVICE_COMPILE__)
    asm volatile("" : "+v"(q.x), "+v"(q.y), "+v"(q.z), "+v"(q.w));
#else
    (void)q;
#endif
}
MRL_HD void not_before_here(Raw4 &r) { not_before_here(r.q0); not_before_here(r.q1); not_before_here(r.q2); not_before_here(r.q3); }
MRL_HD void not_before_here(SearchMem::PairRaw &r) { not_before_here(r.a); not_before_here(r.b); }

// sum_k w_k f(q_k) over the bracket's slices, in slice order: f forms a difference of two stored Floats in f64 (exact)
template <class F>
MRL_HD double blend_of(const Slices &s, const Raw4 &r, F f)
{
#pragma clang fp contract(off)
    double v = s.w[0] * f(r.q0);
    if (s.mask & 2) v = __builtin_fma(s.w[1], f(r.q1), v);
    if (s.mask & 4) v = __builtin_fma(s.w[2], f(r.q2), v);
    if (s.mask & 8) v = __builtin_fma(s.w[3], f(r.q3), v);
    return v;
}
// node row (row + 1) minus node row (row) of a record's integrals, per slice in f64, then blended (the slices as blend_pairs has them)
MRL_HD double pair_diff(const Slices &s, const SearchMem::PairRaw &r)
{
#pragma clang fp contract(off)
    double v = s.w[0] * ((double)r.a.y - (double)r.a.x);
    if (s.mask & 2) v = __builtin_fma(s.w[1], (double)r.b.y - (double)r.b.x, v);
    if (s.mask & 4) v = __builtin_fma(s.w[2], (double)r.a.w - (double)r.a.z, v);
    if (s.mask & 8) v = __builtin_fma(s.w[3], (double)r.b.w - (double)r.b.z, v);
    return v;
}

// the four in-cell differences of a cell's corners (v00, v10, v01, v11), blended: along x in the lower / upper node row, along y
// in the left / right node column
struct CellDiff { double xl, xu, yl, yr; };
MRL_HD CellDiff cell_diff(const Slices &s, const Raw4 &r)
{
    return { blend_of(s, r, [](const float4 &q) { return (double)q.y - (double)q.x; }), blend_of(s, r, [](const float4 &q) { return (double)q.w - (double)q.z; }),
             blend_of(s, r, [](const float4 &q) { return (double)q.z - (double)q.x; }), blend_of(s, r, [](const float4 &q) { return (double)q.w - (double)q.y; }) };
}

// the same bracket with other weights: (d / d tp, d / d tt) of find_slices' products
MRL_HD Slices with_weights(const Slices &s, double w0, double w1, double w2, double w3)
{
    Slices o = s;
    o.w[0] = w0; o.w[1] = w1; o.w[2] = w2; o.w[3] = w3;
    return o;
}

// a parameter's position in its bracket as bracket_by forms it, and d t / d p: 1 / (p1 - p0), 0 while the clamp is active
MRL_HD void bracket_slope(float p0f, float p1f, double p, double &t, double &dt)
{
#pragma clang fp contract(off)
    const double p0 = p0f, p1 = p1f;
    const double r = fast::rcp_nr(p1 - p0);
    t = fast::div_fast(p - p0, p1 - p0);
    dt = (t < 0.0 || t > 1.0) ? 0.0 : r;
    t = t < 0.0 ? 0.0 : (t > 1.0 ? 1.0 : t);
}

// the sums of an inverse warp at cell fractions (x, y) under one set of slice weights: the numerator of sx, its denominator and sy,
// with the pieces they are made of — warp_invert's expressions, operation by operation.  With the derivative weights they are the
// parameter derivatives of the same three.  Filled quantity by quantity for the three sets of weights (eval_dir_grad), so that a
// raw vector is done with before the next is converted.
struct InvertSums { double c0, c1, left, r0, r1, sxn, tot, sy; };

// the cotangents (tb, pb) of theta = atan2(|v_xy|, v_z) and phi = atan2(v_y, v_x) of a unit vector v, taken to v; rho2 = v_x^2 + v_y^2;
// ok = false (v at the normal): zero
MRL_HD void pull_angles(const Vec3d &v, double rho2, bool ok, double tb, double pb, double out[3])
{
#pragma clang fp contract(off)
    const double irho = fast::rsqrt_pos(ok ? rho2 : 1.0), rho = rho2 * irho;
    const double c = ok ? tb * fast::rcp_nr(__builtin_fma(v.z, v.z, rho2)) : 0.0;
    const double hz = c * v.z * irho;
    const double pr = ok ? pb * (irho * irho) : 0.0;
    out[0] = __builtin_fma(-pr, v.y, hz * v.x); out[1] = __builtin_fma(pr, v.x, hz * v.y); out[2] = -(c * rho);
}

// the partials of W = sum_k g_k V_k the channel stage hands back: in the rgb cell's fractions and in (tp, tt)
struct ChannelSums { double W, W_fx, W_fy, W_tp, W_tt; };
// one channel (an RGB channel, a wavelength node) at the cell c under the three sets of weights: its value and its four partials
struct NodeTerms { double v, fx, fy, tp, tt; };
MRL_HD NodeTerms node_terms(const Slices &sv, const Slices &sp, const Slices &st, const Cell &c, const Raw4 &raw)
{
#pragma clang fp contract(off)
    NodeTerms n;
    n.v = bilinear(blend4(sv, raw), c.fx, c.fy);
    const CellDiff d = cell_diff(sv, raw);
    n.tp = bilinear(blend4(sp, raw), c.fx, c.fy); n.tt = bilinear(blend4(st, raw), c.fx, c.fy);
    n.fx = lerp(c.fy, d.xl, d.xu); n.fy = lerp(c.fx, d.yl, d.yr);
    return n;
}
// ... joins the sums with the cotangent gk (0 where the channel is clamped): one ascending FMA chain per sum
MRL_HD void add_channel(ChannelSums &a, double gk, const NodeTerms &n)
{
#pragma clang fp contract(off)
    a.W = __builtin_fma(gk, n.v, a.W);
    a.W_fx = __builtin_fma(gk, n.fx, a.W_fx);
    a.W_fy = __builtin_fma(gk, n.fy, a.W_fy);
    a.W_tp = __builtin_fma(gk, n.tp, a.W_tp);
    a.W_tt = __builtin_fma(gk, n.tt, a.W_tt);
}
// a channel whose value is one stored channel's: clamped below 0
MRL_HD void channel_term(ChannelSums &a, const Slices &sv, const Slices &sp, const Slices &st, const Cell &c, const Raw4 &raw, float g)
{
    const NodeTerms n = node_terms(sv, sp, st, c, raw);
    add_channel(a, n.v < 0.0 ? 0.0 : (double)g, n);
}

// The gradient of ONE unit on the RGL material b in everything but its channel stage — shared by the RGB function below and the
// spectral one (merl_rgl_spectral_dir_grad.hpp).  channels(wr, c, sv, sp, st, scale, sums): reads the measured values at the cell c
// of the values table wr under the weights sv (value), sp, st (d / d tp, d / d tt) and fills sums; scale: ndf / (4 sigma), or 1.
// false: a dead unit — eval's: wi.z <= 0, wo.z <= 0, a NaN / inf component, a failed normalisation —, out is +0.0f, nothing was read
// and channels was not called.  g: where the parameter grids are read.  MASK: the bracket shape when the caller knows it at compile
// time (1, 3, 5, 15: find_slices' mask; every test on it folds and the reads and sums are straight-line code), 0: tested at run time
// — the same operations in the same order either way.
template <int MASK, class Grids, class Channels>
MRL_HD bool dir_grad_core(const RglDev &b, const Grids &g, float wix, float wiy, float wiz, float wox, float woy, float woz, RglDirGrad &out, Channels &&channels)
{
#pragma clang fp contract(off)
    for (int k = 0; k < 3; ++k) out.wi[k] = out.wo[k] = 0.0f;
    const float nf = ((wix - wix) + (wiy - wiy)) + ((wiz - wiz) + (wox - wox)) + ((woy - woy) + (woz - woz));      // 0, or NaN
    if (!(wiz > 0.0f) || !(woz > 0.0f) || !(nf == 0.0f)) return false;
    Incident in;
    if (!incident<false>(b, g, wix, wiy, wiz, in)) return false;
    if constexpr (MASK != 0) in.sv.mask = MASK;
    const Vec3d &a = in.wi;
    Vec3d wo = { (double)(wox * in.fx), (double)(woy * in.fy), (double)woz };
    if (!unit3(wo)) return false;
    const Vec3d s = { a.x + wo.x, a.y + wo.y, a.z + wo.z };
    Vec3d m = s;
    if (!unit3(m)) return false;
    // half_lookup's coordinates
    const double theta_m = elevation(m), phi_m = azimuth(m.y, m.x);
    const double umx = theta2u(theta_m);
    double umy = phi2u(b.isotropic ? phi_m - in.phi_i : phi_m);
    umy -= floor(umy);
    const double uix = theta2u(in.theta_i), uiy = phi2u(in.phi_i);

    // the parameter bracket find_slices chose, from its offsets: the nodes around (phi_i, theta_i) and the slopes of (tp, tt)
    const WarpDev wv = b.vndf(), wr = b.rgb();
    const Slices &sv = in.sv;
    const unsigned tbr = (unsigned)(b.n_theta > 1 ? b.n_theta - 1 : 1);
    const unsigned ib = sv.quad / (unsigned)(wv.ny - 1), ip = ib / tbr, it = ib - ip * tbr;
    double tp = 0.0, tt = 0.0, dtp = 0.0, dtt = 0.0;
    if (b.n_phi > 1) bracket_slope(g.phi_at((int)ip), g.phi_at((int)ip + 1), in.phi_i, tp, dtp);
    if (b.n_theta > 1) bracket_slope(g.theta_at((int)it), g.theta_at((int)it + 1), in.theta_i, tt, dtt);
    const Slices sp = with_weights(sv, -(1.0 - tt), 1.0 - tt, -tt, tt), st = with_weights(sv, -(1.0 - tp), -tp, 1.0 - tp, tp);

    // ---- stage 1: every read the directions alone address ----
    const SearchMem tv(wv);
    const int nx = wv.nx, ny = wv.ny;
    const double px = umx * (double)(nx - 1), py = umy * (double)(ny - 1);
    const int col = clamp_cell(px, nx - 2), row = clamp_cell(py, ny - 2);
    const double x = px - (double)col, y = py - (double)row;
    Raw4 qr = fetch_raw(sv, wv, row * (nx - 1) + col);
    auto lr = tv.left_raw(sv, row * (nx - 1) + col);
    auto tr = tv.total_raw(sv, row);
    auto br = tv.marg_raw(sv, row > 0 ? row - 1 : 0);
    const Slices one = single_slice();
    const WarpDev wn = b.ndf(), ws = b.sigma();
    const Cell cn = locate(wn, umx, umy), cs = locate(ws, uix, uiy);
    Raw4 rn{}, rs{};
    if (b.jacobian) { rn = fetch_raw(one, wn, cn.index); rs = fetch_raw(one, ws, cs.index); }

    // the inverse warp: value and parameter derivatives of (sxn, tot, sy), quantity by quantity, the exact in-cell differences
    // beside each; then sx, sy as eval forms them
    InvertSums iv, ip_, it_;
    auto corners = [&](const Slices &w, InvertSums &o) { const D4 q = blend4(w, qr); o.c0 = lerp(y, q.x, q.z); o.c1 = lerp(y, q.y, q.w); };
    auto lefts = [&](const Slices &w, InvertSums &o) { const D2 l = tv.pair_blend(w, lr); o.left = lerp(y, l.x, l.y); };
    auto totals = [&](const Slices &w, InvertSums &o) { const D2 t = tv.pair_blend(w, tr); o.r0 = t.x; o.r1 = t.y; };
    auto finish = [&](const Slices &w, InvertSums &o) {
        const double bf = tv.marg_blend(w, br);
        o.sxn = __builtin_fma(x, __builtin_fma(0.5 * x, o.c1 - o.c0, o.c0), o.left);
        o.tot = lerp(y, o.r0, o.r1);
        o.sy = __builtin_fma(y, __builtin_fma(0.5 * y, o.r1 - o.r0, o.r0), row > 0 ? bf : 0.0);
    };
    not_before_here(qr);
    corners(sv, iv); corners(sp, ip_); corners(st, it_);
    const CellDiff dq = cell_diff(sv, qr);
    not_before_here(lr);
    lefts(sv, iv); lefts(sp, ip_); lefts(st, it_);
    const double dleft = pair_diff(sv, lr);
    not_before_here(tr);
    totals(sv, iv); totals(sp, ip_); totals(st, it_);
    const double dr = pair_diff(sv, tr);
    not_before_here(br);
    finish(sv, iv); finish(sp, ip_); finish(st, it_);
    const bool has_mass = iv.tot > 0.0;
    const double inv_tot = fast::rcp_nr(has_mass ? iv.tot : 1.0);
    const double sx = has_mass ? iv.sxn * inv_tot : 0.0, sy = iv.sy;

    const double k_tot = has_mass ? inv_tot : 0.0;                                   // tot == 0: zero terms
    const double dsx_dx = lerp(x, iv.c0, iv.c1) * k_tot;
    const double dA_dy = x * __builtin_fma(0.5 * x, dq.yr - dq.yl, dq.yl);
    const double dsx_dy = (dA_dy + dleft - sx * dr) * k_tot;
    const double dsx_dtp = (ip_.sxn - sx * ip_.tot) * k_tot, dsx_dtt = (it_.sxn - sx * it_.tot) * k_tot;

    // 3. the jacobian's factor ndf / (4 sigma) and the partials of its logarithm's pieces in u_m and u_wi (times W below)
    double scale = 1.0, n_x = 0.0, n_y = 0.0, s_x = 0.0, s_y = 0.0;
    if (b.jacobian) {
        const double nv = bilinear(blend4(one, rn), cn.fx, cn.fy), sg = bilinear(blend4(one, rs), cs.fx, cs.fy);
        const CellDiff dn = cell_diff(one, rn), ds = cell_diff(one, rs);
        const double inv4 = fast::rcp_nr(4.0 * sg);
        scale = nv * inv4;
        n_x = inv4 * lerp(cn.fy, dn.xl, dn.xu) * (double)(wn.nx - 1);               // d scale / d u_m
        n_y = inv4 * lerp(cn.fx, dn.yl, dn.yr) * (double)(wn.ny - 1);
        const double sg_b = -(scale * inv4 * 4.0);                                   // d scale / d sigma
        s_x = sg_b * lerp(cs.fy, ds.xl, ds.xu) * (double)(ws.nx - 1);                // d scale / d u_wi
        s_y = sg_b * lerp(cs.fx, ds.yl, ds.yr) * (double)(ws.ny - 1);
    }

    // ---- stage 2: the channels at the cell of (sx, sy) ----
    // 1. the partials of W = sum_k g_k V_k over the channels that are not clamped
    const Cell c = locate(wr, sx, sy);
    ChannelSums cs_ = { 0.0, 0.0, 0.0, 0.0, 0.0 };
    channels(wr, c, sv, sp, st, scale, cs_);
    const double W = cs_.W, W_fx = cs_.W_fx, W_fy = cs_.W_fy, W_tp = cs_.W_tp, W_tt = cs_.W_tt;
    double umx_b = W * n_x, umy_b = W * n_y;
    const double uix_b = W * s_x, uiy_b = W * s_y;

    // 2. back through the inverse warp
    const double sx_b = scale * W_fx * (double)(nx - 1), sy_b = scale * W_fy * (double)(ny - 1);
    const double x_b = sx_b * dsx_dx, y_b = __builtin_fma(sx_b, dsx_dy, sy_b * iv.tot);
    const double tp_b = __builtin_fma(scale, W_tp, __builtin_fma(sx_b, dsx_dtp, sy_b * ip_.sy));
    const double tt_b = __builtin_fma(scale, W_tt, __builtin_fma(sx_b, dsx_dtt, sy_b * it_.sy));
    umx_b = __builtin_fma(x_b, (double)(nx - 1), umx_b);
    umy_b = __builtin_fma(y_b, (double)(ny - 1), umy_b);

    // 4. to the angles: u = sqrt(2 theta / pi) has d u / d theta = 1 / (pi u); the azimuths map with 1 / 2 pi
    const double rho_m2 = __builtin_fma(m.x, m.x, m.y * m.y), rho_a2 = __builtin_fma(a.x, a.x, a.y * a.y);
    const bool ok_m = rho_m2 > fast::kSingular, ok_a = rho_a2 > fast::kSingular;
    constexpr double k_az = 0.5 / kPi, k_el = 1.0 / kPi;
    const double phi_m_b = ok_m ? umy_b * k_az : 0.0;
    const double theta_m_b = ok_m ? umx_b * k_el * fast::rcp_nr(umx) : 0.0;
    const double theta_i_b = ok_a ? __builtin_fma(uix_b * k_el, fast::rcp_nr(uix), tt_b * dtt) : 0.0;
    const double phi_i_b = ok_a ? __builtin_fma(tp_b, dtp, uiy_b * k_az) - (b.isotropic ? phi_m_b : 0.0) : 0.0;
    double m_b[3], a_b[3], s_b[3];
    pull_angles(m, rho_m2, ok_m, theta_m_b, phi_m_b, m_b);
    pull_angles(a, rho_a2, ok_a, theta_i_b, phi_i_b, a_b);
    // m = s / |s|, s = a + b; a = wi' / |wi'|, b = wo' / |wo'| with wi', wo' the directions in the stored part of the azimuth
    const double ins = fast::rsqrt_pos(__builtin_fma(s.x, s.x, __builtin_fma(s.y, s.y, s.z * s.z)));
    fast::through_normalisation(fast::Vec3{ m.x, m.y, m.z }, ins, m_b[0], m_b[1], m_b[2], 1.0, s_b);
    const double rs_i = fast::dir_f32(wix * in.fx, wiy * in.fy, wiz).rs, rs_o = fast::dir_f32(wox * in.fx, woy * in.fy, woz).rs;
    double gi[3], go[3];
    fast::through_normalisation(fast::Vec3{ a.x, a.y, a.z }, rs_i, a_b[0] + s_b[0], a_b[1] + s_b[1], a_b[2] + s_b[2], 1.0, gi);
    fast::through_normalisation(fast::Vec3{ wo.x, wo.y, wo.z }, rs_o, s_b[0], s_b[1], s_b[2], 1.0, go);
    const double fx = (double)in.fx, fy = (double)in.fy;
    out.wi[0] = fast::finite_f32(gi[0] * fx); out.wi[1] = fast::finite_f32(gi[1] * fy); out.wi[2] = fast::finite_f32(gi[2]);
    out.wo[0] = fast::finite_f32(go[0] * fx); out.wo[1] = fast::finite_f32(go[1] * fy); out.wo[2] = fast::finite_f32(go[2]);
    return true;
}

// grad_wi = sum_c g_c dE_c / d wi and grad_wo of ONE unit on the RGB RGL material b: dir_grad_core with the three channels' corner
// vectors read together and summed in channel order.  Dead units return +0.0f whatever g32 holds.
template <int MASK = 0, class Grids>
MRL_HD RglDirGrad eval_dir_grad(const RglDev &b, const Grids &g, float wix, float wiy, float wiz, float wox, float woy, float woz, const float g32[3])
{
    RglDirGrad out;
    dir_grad_core<MASK>(b, g, wix, wiy, wiz, wox, woy, woz, out,
        [&](const WarpDev &wr, const Cell &c, const Slices &sv, const Slices &sp, const Slices &st, double, ChannelSums &a) {
            Raw4 raw0 = fetch_raw(sv, wr, c.index, 0), raw1 = fetch_raw(sv, wr, c.index, 1), raw2 = fetch_raw(sv, wr, c.index, 2);
            not_before_here(raw0); channel_term(a, sv, sp, st, c, raw0, g32[0]);
            not_before_here(raw1); channel_term(a, sv, sp, st, c, raw1, g32[1]);
            not_before_here(raw2); channel_term(a, sv, sp, st, c, raw2, g32[2]);
        });
    return out;
}

} // namespace rgl
} // namespace mrl
