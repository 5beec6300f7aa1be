// merl_table_dir_grad.hpp — the per-lane gradient of eval in the directions on an RGB table material (include/merl_hip_diff_table.h,
// DESIGN.md §5j): the function k_table_grad_dir runs, __host__ __device__ and free of HIP calls so that a host harness can run it.
//
// E_c(wi, wo) = T_c(x(a, b)) kappa with a = wi / |wi|, b = wo / |wo|, x the table coordinates of merl_table_fast.hpp, T_c the exact
// trilinear interpolant of the stored Float texels in the cell eval selects, kappa the Float wo.z (or 1).  Reverse mode, for the
// cotangent g of the three channels:
//   1. per channel the cell's texels are first taken relative to corner 0, u_k[c] = f[k][c] - f[0][c]: differences of Floats, exact
//      in f64 (to 2^-53 of themselves when the exponents lie more than 29 apart).  These are contracted with g corner by corner,
//      t_k = sum_c g_c u_k[c], t_0 = 0.  V = sum_c g_c T_c is sum_c g_c f[0][c] plus the trilinear form of the t_k, and
//      D_axis = sum_c g_c dT_c / df_axis the bilinear form of the differences of the t_k along the axis, all with f64 weights: nothing
//      of the Float corner weights or the packed Float blend of eval enters.  A t_k carries three f64 roundings of
//      sum_c |g_c| |f[k][c] - f[0][c]|, so the error of a D_axis is 2^-51 of sum_c |g_c| times the VARIATION of channel c inside the
//      cell — never of a channel's magnitude: a large flat channel next to a small smooth one contributes exact zeros.  Equal texels
//      give exactly 0.  (Contracting the raw texels first is no cheaper and wrong by 2^-53 of the largest |g_c f_c|; taking
//      all twelve edge differences per channel first is the same as this to 1e-15 of the cell's variation and compiles to 166 VGPRs
//      against 136 to 142: still three waves per SIMD, but under that bound of 168 the material-id kernels spill 12 B per lane);
//   2. the three D_axis are pulled back through the coordinate map onto the unit vectors a and b.  atan2(y, x) has the derivative
//      (x dy - y dx) / (x^2 + y^2), d xh / d theta_h = k_th / (2 xh): no polynomial, no libm, reciprocals and square roots from the
//      library's seeds + Newton steps;
//   3. through the two normalisations, (v - w (w . v) / |w|^2) / |w|, and the cosine: grad_wo.z += V.
// A clamped fraction has derivative 0 while its clamp is active; the padded upper end has it through its equal texels.  Where a
// coordinate map has no derivative (h == n, retro-reflection, px == py == 0; a direction at the normal in the standard forms) that
// coordinate's term is dropped by a select BEFORE any product, so no 0 * inf is formed.  A nearest lookup (MRL_OPT_LOOKUP = 0) is
// the same code with the nearest cell, zero fractions and zero masks: V is then the texel itself and every D_axis is 0.
// Contraction is off and the FMAs are spelt out: a unit's bits do not depend on the kernel the function is inlined into.
#pragma once
#include "merl_table_fast.hpp"

namespace mrl {
namespace fast {

struct TableDirGrad { float wi[3], wo[3]; };

// below this a singular measure (rho^2, |e|^2, px^2 + py^2, ...) counts as zero: its reciprocal stays finite
constexpr double kSingular = 1e-280;

// (1 - t) u + t v
MRL_HD double lerp_fma(double s, double t, double u, double v)
{
#pragma clang fp contract(off)
    return __builtin_fma(t, v, s * u);
}

// what the pull-backs return: the cotangents of the unit vectors a and b
struct UnitAdjoint { double ax, ay, az, bx, by, bz; };

// half / difference angles: x = (sqrt(theta_h k_th), theta_d k_td, phi_d k_pd) of s = a + b, e = a - b (coords() above).
// Xh, Xd, Xp: the cotangents of the three coordinates; xh: the first coordinate itself
MRL_HD UnitAdjoint pull_half_diff(const Vec3 &a, const Vec3 &b, double k_th, double k_td, double k_pd, double xh, double Xh, double Xd, double Xp)
{
#pragma clang fp contract(off)
    const double sx = a.x + b.x, sy = a.y + b.y, sz = a.z + b.z;
    const double ex = a.x - b.x, ey = a.y - b.y, ez = a.z - b.z;
    const double rho2 = __builtin_fma(sx, sx, sy * sy);
    const double s2 = __builtin_fma(sz, sz, rho2);
    const double e2 = __builtin_fma(ex, ex, __builtin_fma(ey, ey, ez * ez));
    const bool ok_h = rho2 > kSingular, ok_e = e2 > kSingular;
    const double irho = rsqrt_pos(ok_h ? rho2 : 1.0), rho = rho2 * irho;
    const double ins = rsqrt_pos(s2), ns = s2 * ins;                // |s| > 0 on every live unit (s_z > 0)
    const double ine = rsqrt_pos(ok_e ? e2 : 1.0), ne = e2 * ine;
    // theta_h = atan2(rho, s_z), xh = sqrt(theta_h k_th): d xh / d theta_h = k_th / (2 xh)
    const double th_bar = ok_h ? Xh * (0.5 * k_th) * rcp_nr(xh) : 0.0;
    const double c_h = th_bar * (ins * ins);
    const double hz = c_h * sz * irho;
    double s_x = hz * sx, s_y = hz * sy, s_z = -(c_h * rho);
    // theta_d = atan2(|e|, |s|)
    const double q = ok_e ? Xd * k_td * rcp_nr(e2 + s2) : 0.0;
    double c_s = -(q * ne * ins);                                   // times s
    const double c_e = q * ns * ine;                                // times e
    double e_x = c_e * ex, e_y = c_e * ey, e_z = c_e * ez;
    // phi_d = atan2(py, px) mod pi, py = e_y s_x - e_x s_y, px = -e_z |s|
    const double py = __builtin_fma(ey, sx, -(ex * sy)), px = -ez * ns;
    const double pp = __builtin_fma(px, px, py * py);
    const bool ok_p = ok_h && pp > kSingular;
    const double r = ok_p ? Xp * k_pd * rcp_nr(ok_p ? pp : 1.0) : 0.0;
    const double py_bar = r * px, px_bar = -(r * py);
    s_x = __builtin_fma(py_bar, ey, s_x); s_y = __builtin_fma(-py_bar, ex, s_y);
    e_y = __builtin_fma(py_bar, sx, e_y); e_x = __builtin_fma(-py_bar, sy, e_x);
    e_z = __builtin_fma(-px_bar, ns, e_z);
    c_s = __builtin_fma(-px_bar, ez * ins, c_s);
    s_x = __builtin_fma(c_s, sx, s_x); s_y = __builtin_fma(c_s, sy, s_y); s_z = __builtin_fma(c_s, sz, s_z);
    return { s_x + e_x, s_y + e_y, s_z + e_z, s_x - e_x, s_y - e_y, s_z - e_z };
}

// the standard forms: x = (theta_i k_0, theta_o k_1, dphi k_2), theta = atan2(|v_xy|, v_z), dphi = atan2(cr, dt) — its magnitude in
// the mirrored form (sign(cr) is the derivative of the fold), itself in the full one (coords_standard() above)
MRL_HD UnitAdjoint pull_standard(const Vec3 &a, const Vec3 &b, bool full, double k_0, double k_1, double k_2, double Xh, double Xd, double Xp)
{
#pragma clang fp contract(off)
    const double ra2 = __builtin_fma(a.x, a.x, a.y * a.y), rb2 = __builtin_fma(b.x, b.x, b.y * b.y);
    const bool ok_a = ra2 > kSingular, ok_b = rb2 > kSingular;
    const double ira = rsqrt_pos(ok_a ? ra2 : 1.0), irb = rsqrt_pos(ok_b ? rb2 : 1.0);
    const double c_a = ok_a ? Xh * k_0 * rcp_nr(__builtin_fma(a.z, a.z, ra2)) : 0.0;
    const double c_b = ok_b ? Xd * k_1 * rcp_nr(__builtin_fma(b.z, b.z, rb2)) : 0.0;
    const double az = c_a * a.z * ira, bz = c_b * b.z * irb;
    UnitAdjoint u = { az * a.x, az * a.y, -(c_a * (ra2 * ira)), bz * b.x, bz * b.y, -(c_b * (rb2 * irb)) };
    const double cr = __builtin_fma(a.x, b.y, -(a.y * b.x)), dt = __builtin_fma(a.x, b.x, a.y * b.y);
    const double cc = __builtin_fma(cr, cr, dt * dt);
    const bool ok_c = cc > kSingular;
    const double xp = (!full && cr < 0.0) ? -Xp : Xp;
    const double r = ok_c ? xp * k_2 * rcp_nr(ok_c ? cc : 1.0) : 0.0;
    const double cr_bar = r * dt, dt_bar = -(r * cr);
    u.ax = __builtin_fma(cr_bar, b.y, __builtin_fma(dt_bar, b.x, u.ax));
    u.ay = __builtin_fma(-cr_bar, b.x, __builtin_fma(dt_bar, b.y, u.ay));
    u.bx = __builtin_fma(-cr_bar, a.y, __builtin_fma(dt_bar, a.x, u.bx));
    u.by = __builtin_fma(cr_bar, a.x, __builtin_fma(dt_bar, a.y, u.by));
    return u;
}

// a cotangent of the unit vector u = w / |w| taken back to w: (v - u (u . v)) / |w|, times the factor k, as Float
MRL_HD void through_normalisation(const Vec3 &u, double rs, double vx, double vy, double vz, double k, double out[3])
{
#pragma clang fp contract(off)
    const double d = __builtin_fma(u.x, vx, __builtin_fma(u.y, vy, u.z * vz));
    const double s = rs * k;
    out[0] = __builtin_fma(-u.x, d, vx) * s; out[1] = __builtin_fma(-u.y, d, vy) * s; out[2] = __builtin_fma(-u.z, d, vz) * s;
}

// into the Float range; a NaN (a live unit whose cotangent overflows: inf - inf in the projections) becomes 0, not a number
MRL_HD float finite_f32(double x)
{
    const double c = __builtin_fmin(__builtin_fmax(x, -3.4028234663852886e38), 3.4028234663852886e38);
    return x == x ? (float)c : 0.0f;
}

// table_eval_dir_grad below in three parts, so that the n-channel function (merl_nch_dir_grad.hpp) runs the second and the third on
// its own t_k: the operations and their order are those of the one function this was.
// Part 1, cell selection: the unit vectors, eval's own coordinates, the cell (h0, d0, p0) eval selects and its fractions
struct DirCell {
    Dir in_dir, out_dir;
    Vec3 a, b;
    double c_xh;                 // the unshifted first coordinate (the sqrt warp's derivative needs it)
    bool mh, md, mp;             // df / dx is 1: trilinear, and no lower clamp active on the shifted coordinate (the azimuth: or periodic)
    TableCell cell;              // the cell eval selects and its fractions (a dead unit's: some cell inside the table)
    double k_th, k_td, k_pd;
    bool trilinear, periodic;
    float kappa;                 // eval_tail's Float wo.z (or 1; NaN when an input is not finite)
    bool live;                   // not one of eval's dead units
};

MRL_HD DirCell dir_cell(const MaterialDev &m, const Options &o, float wix, float wiy, float wiz, float wox, float woy, float woz)
{
#pragma clang fp contract(off)
    DirCell s;
    const TableMaps maps(m);
    s.in_dir = dir_f32(wix, wiy, wiz); s.out_dir = dir_f32(wox, woy, woz);
    s.a = unit(s.in_dir); s.b = unit(s.out_dir);
    const Coords c = maps(normalize_f32(wix, wiy, wiz), s.out_dir);         // eval's own coordinates: they select the cell
    s.trilinear = o.lookup != 0; s.periodic = param_phi_periodic(m.param);
    const int node = s.trilinear && o.node;
    const double shift = node ? 0.5 : 0.0;
    s.c_xh = c.xh;
    s.mh = s.trilinear && c.xh - shift >= 0.0; s.md = s.trilinear && c.xd - shift >= 0.0; s.mp = s.trilinear && (s.periodic || c.xp - shift >= 0.0);
    s.k_th = maps.k_th; s.k_td = maps.k_td; s.k_pd = maps.k_pd;
    // eval's cell under either lookup, selected (the option is wave-uniform; a nearest lookup has no fractions).  A dead unit's
    // coordinates are garbage: whatever they are, the trilinear cell stays inside the table (nearest_cell's already does)
    TableCell tri = trilinear_cell(c, m.n_th, m.n_td, m.n_pd, node, m.param);
    tri.h0 = clampi(tri.h0, 0, m.n_th - 1); tri.d0 = clampi(tri.d0, 0, m.n_td - 1); tri.p0 = clampi(tri.p0, 0, m.n_pd - 1);
    s.cell = s.trilinear ? tri : nearest_cell(c, m.n_th, m.n_td, m.n_pd);
    s.kappa = cos_or_nan32((wix + wiy + wiz), wox, woy, woz, o.cosine != 0);
    s.live = (wiz > 0.0f) && (woz > 0.0f) && (s.kappa == s.kappa);
    return s;
}

// Part 2, the forms of the t_k (t[0] == 0): V = base + the trilinear form, and the three bilinear forms of the differences along the
// axes, masked: df / dx is 1 inside the cell; 0 under an active lower clamp (the upper end has equal texels: its D is 0) and for nearest
struct DirForms { double V, Xh, Xd, Xp; };

MRL_HD DirForms dir_forms(const DirCell &s, const double t[8], double base)
{
#pragma clang fp contract(off)
    const double fh = s.cell.fh, fd = s.cell.fd, fp = s.cell.fp;
    const double gh = 1.0 - fh, gd = 1.0 - fd, gp = 1.0 - fp;
    DirForms r;
    r.V = base + lerp_fma(gh, fh, lerp_fma(gd, fd, fp * t[1], lerp_fma(gp, fp, t[2], t[3])),
                          lerp_fma(gd, fd, lerp_fma(gp, fp, t[4], t[5]), lerp_fma(gp, fp, t[6], t[7])));
    // corners (k, k + 1) along the azimuth, (k, k + 2) along axis 1, (k, k + 4) along axis 0
    const double Dp = lerp_fma(gh, fh, lerp_fma(gd, fd, t[1], t[3] - t[2]), lerp_fma(gd, fd, t[5] - t[4], t[7] - t[6]));
    const double Dd = lerp_fma(gh, fh, lerp_fma(gp, fp, t[2], t[3] - t[1]), lerp_fma(gp, fp, t[6] - t[4], t[7] - t[5]));
    const double Dh = lerp_fma(gd, fd, lerp_fma(gp, fp, t[4], t[5] - t[1]), lerp_fma(gp, fp, t[6] - t[2], t[7] - t[3]));
    r.Xh = s.mh ? Dh : 0.0;
    r.Xd = s.md ? Dd : 0.0;
    r.Xp = s.mp ? Dp : 0.0;
    return r;
}

// Part 3, pull-back and tail: through the coordinate map (a wave-uniform branch for a single-material launch), the normalisations
// and the cosine factor, and the dead-unit select
MRL_HD TableDirGrad dir_tail(int param, const Options &o, const DirCell &s, const DirForms &F)
{
#pragma clang fp contract(off)
    const UnitAdjoint u = param == PARAM_HALF_DIFF ? pull_half_diff(s.a, s.b, s.k_th, s.k_td, s.k_pd, s.c_xh, F.Xh, F.Xd, F.Xp)
                                                   : pull_standard(s.a, s.b, param == PARAM_STANDARD_FULL, s.k_th, s.k_td, s.k_pd, F.Xh, F.Xd, F.Xp);
    const bool no_cosine = o.cosine != 0;
    const bool live = s.live;
    double gi[3], go[3];
    through_normalisation(s.a, s.in_dir.rs, u.ax, u.ay, u.az, (double)s.kappa, gi);
    through_normalisation(s.b, s.out_dir.rs, u.bx, u.by, u.bz, (double)s.kappa, go);
    go[2] += no_cosine ? 0.0 : F.V;
    TableDirGrad r;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        r.wi[k] = live ? finite_f32(gi[k]) : 0.0f;
        r.wo[k] = live ? finite_f32(go[k]) : 0.0f;
    }
    return r;
}

// grad_wi = sum_c g_c dE_c / d wi and grad_wo of ONE unit on the RGB table m (kind MERL / TABLE, its texels in layout LAYOUT) under the
// options o (lookup, node, cosine; negative is a property of the stored texels here).  Dead units — eval's: wi.z <= 0, wo.z <= 0, a
// NaN / inf component — get +0.0f from a select at the very end, whatever g holds.
template <int LAYOUT>
MRL_HD TableDirGrad table_eval_dir_grad(const MaterialDev &m, const Options &o, float wix, float wiy, float wiz, float wox, float woy, float woz,
                                        const float g32[3])
{
#pragma clang fp contract(off)
    const DirCell s = dir_cell(m, o, wix, wiy, wiz, wox, woy, woz);
    float4 q[6];                                                 // lookup_trilinear_t's loads: corner-major RGB, float 3 k + ch
    load_cell<LAYOUT>(m, s.cell, q);
    float f[24];
#pragma unroll
    for (int p = 0; p < 6; ++p) { f[4 * p] = q[p].x; f[4 * p + 1] = q[p].y; f[4 * p + 2] = q[p].z; f[4 * p + 3] = q[p].w; }

    // 1. per channel the seven exact differences to corner 0, u_k[c] = f[k][c] - f[0][c], contracted with g: t_k = sum_c g_c u_k[c] (t_0 = 0).
    //    V is sum_c g_c f[0][c] plus the trilinear form of the t_k, the three D_axis the bilinear forms of their differences
    const double g[3] = { (double)g32[0], (double)g32[1], (double)g32[2] };
    const double b0 = (double)f[0], b1 = (double)f[1], b2 = (double)f[2];
    double t[8];
    t[0] = 0.0;
#pragma unroll
    for (int k = 1; k < 8; ++k)
        t[k] = __builtin_fma(g[2], (double)f[3 * k + 2] - b2, __builtin_fma(g[1], (double)f[3 * k + 1] - b1, g[0] * ((double)f[3 * k] - b0)));
    const DirForms F = dir_forms(s, t, __builtin_fma(g[2], b2, __builtin_fma(g[1], b1, g[0] * b0)));
    // 2. through the coordinate map, 3. through the normalisations and the cosine factor
    return dir_tail(m.param, o, s, F);
}

} // namespace fast
} // namespace mrl
