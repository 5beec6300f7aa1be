// merl_ggx_fast.hpp — tuned per-lane GGX rough conductor (row a9; BASELINE config 3).
//
// Same real-valued functions as merl_device.hpp's ggx_* (which mirror the oracle formula for
// formula), re-expressed without libm calls: every division / sqrt goes through the v_rcp_f64 /
// v_rsq_f64 + Newton helpers of merl_table_fast.hpp, and the visible-normal sampler never forms an
// angle — with s the stretched unit incident direction, tan(theta) = |s_xy| / s_z and
// (cos phi, sin phi) = s_xy / |s_xy|, where the generic path calls acos, atan2, tan, cos and sin.
#pragma once
#include "merl_table_fast.hpp"

namespace mrl {
namespace fast {

struct GgxConsts {                 // per material, computed once per launch (SGPRs for a single-material launch)
    double alpha, inv_alpha2, inv_pi_alpha2;
    double eta2_k2[3];             // eta^2 - k^2
    double four_k2_eta2[3];        // 4 k^2 eta^2
    GgxConsts() = default;         // filled in by ggx_consts_exact
    MRL_HD explicit GgxConsts(const MaterialDev &m)
    {
        alpha = m.alpha;
        inv_alpha2 = rcp_nr(m.alpha * m.alpha);
        inv_pi_alpha2 = inv_alpha2 * 0.31830988618379067154;
        for (int c = 0; c < 3; ++c) {
            eta2_k2[c] = m.eta[c] * m.eta[c] - m.k[c] * m.k[c];
            four_k2_eta2[c] = 4.0 * m.k[c] * m.k[c] * m.eta[c] * m.eta[c];
        }
    }
};

// D = 1 / (pi a^2 (cos^2 + sin^2/a^2)^2): the oracle's (1 + tan^2/a^2) cos^2 with the division folded away
__device__ __forceinline__ double ggx_D(const GgxConsts &g, const Vec3 &m)
{
    const double root = __builtin_fma(__builtin_fma(m.x, m.x, m.y * m.y), g.inv_alpha2, m.z * m.z);
    const double r = g.inv_pi_alpha2 * rcp_nr(__builtin_fmax(root * root, kTiny));
    return (m.z <= 0.0 || r * m.z < 1e-20) ? 0.0 : r;
}

// G1 = 2 / (1 + sqrt(1 + a^2 tan^2)) = 2 |vz| / (|vz| + sqrt(vz^2 + a^2 (1 - vz^2))): one sqrt, one reciprocal
__device__ __forceinline__ double ggx_G1(const GgxConsts &g, const Vec3 &v, const Vec3 &m)
{
    const double vm = __builtin_fma(v.x, m.x, __builtin_fma(v.y, m.y, v.z * m.z));
    const double vz2 = v.z * v.z;
    const double s2 = 1.0 - vz2;
    const double az = __builtin_fabs(v.z);
    const double r = 2.0 * az * rcp_nr(__builtin_fmax(az + sqrt_fast(__builtin_fma(g.alpha * g.alpha, s2, vz2)), kTiny));
    const double res = s2 <= 0.0 ? 1.0 : r;
    return vm * v.z <= 0.0 ? 0.0 : res;
}

__device__ __forceinline__ double fresnel_conductor(const GgxConsts &g, int ch, double c)
{
    const double c2 = c * c, s2 = 1.0 - c2, s4 = s2 * s2;
    const double t1 = g.eta2_k2[ch] - s2;
    const double a2pb2 = sqrt_fast(__builtin_fma(t1, t1, g.four_k2_eta2[ch]));
    const double a = sqrt_fast(0.5 * (a2pb2 + t1));
    const double term1 = a2pb2 + c2, term2 = 2.0 * a * c;
    const double term3 = __builtin_fma(a2pb2, c2, s4), term4 = term2 * s2;
    // Rs = (t1-t2)/(t1+t2), Rp = Rs (t3-t4)/(t3+t4): one reciprocal of the product of both denominators
    const double d12 = term1 + term2, d34 = term3 + term4;
    const double inv = rcp_nr(d12 * d34);
    const double rs2 = (term1 - term2) * d34 * inv;
    const double rp2 = rs2 * (term3 - term4) * d12 * inv;
    return 0.5 * (rp2 + rs2);
}

MRL_HD Vec3 unit_sum(const Vec3 &a, const Vec3 &b)
{
    const double x = a.x + b.x, y = a.y + b.y, z = a.z + b.z;
    double s, rs;
    sqrt_rsqrt(__builtin_fma(x, x, __builtin_fma(y, y, z * z)), s, rs);
    return { x * rs, y * rs, z * rs };
}

// eval = F D G / (4 cos theta_i) (cosine of wo folded in), and pdf = D G1(wi) / (4 cos theta_i)
__device__ __forceinline__ void ggx_eval_pdf(const GgxConsts &g, const Vec3 &in, const Vec3 &out, double rgb[3], double &pdf)
{
    const Vec3 m = unit_sum(in, out);
    const double D = ggx_D(g, m);
    const double G1i = ggx_G1(g, in, m);
    const double quarter_inv_cos = 0.25 * rcp_nr(in.z);
    pdf = D * G1i * quarter_inv_cos;
    const double model = pdf * ggx_G1(g, out, m);
    const double c = __builtin_fma(in.x, m.x, __builtin_fma(in.y, m.y, in.z * m.z));
    rgb[0] = D == 0.0 ? 0.0 : fresnel_conductor(g, 0, c) * model;
    rgb[1] = D == 0.0 ? 0.0 : fresnel_conductor(g, 1, c) * model;
    rgb[2] = D == 0.0 ? 0.0 : fresnel_conductor(g, 2, c) * model;
}

// ---- forward-mode twins of ggx_D, ggx_G1 and fresnel_conductor (merl_ggx_grad.hip) ----
// Each returns the value its twin returns (same selects) and the derivative the parameter gradient needs, from the reciprocals
// and square roots the value takes anyway.  The alpha-derivatives are LOG-derivatives: d eval / d alpha = eval x their sum, so
// nothing is divided by a D or G1 that vanishes.  Contraction is off: the gradient-only and the gradient + normal kernel inline
// these in different surroundings and must round alike (mrl_ggx_grad_batch returns the same grad_params bits with and without
// `normal`); every fused multiply-add below is spelt out.

// root = sin^2/a^2 + cos^2, D = 1 / (pi a^2 root^2):  d ln D / d alpha = -2/a + 4 sin^2 / (a^3 root) = (2/a) (sin^2/a^2 - cos^2) / root
MRL_HD double ggx_D_dlog(const GgxConsts &g, const Vec3 &m, double &dlog)
{
#pragma clang fp contract(off)
    const double s_a2 = __builtin_fma(m.x, m.x, m.y * m.y) * g.inv_alpha2, c2 = m.z * m.z;
    const double inv = rcp_nr(__builtin_fmax(s_a2 + c2, kTiny));
    const double r = g.inv_pi_alpha2 * (inv * inv);
    dlog = 2.0 * (g.alpha * g.inv_alpha2) * ((s_a2 - c2) * inv);
    return (m.z <= 0.0 || r * m.z < 1e-20) ? 0.0 : r;
}

// q = sqrt(vz^2 + a^2 sin^2), G1 = 2 |vz| / (|vz| + q):  d ln G1 / d alpha = -(a sin^2 / q) / (|vz| + q)
MRL_HD double ggx_G1_dlog(const GgxConsts &g, const Vec3 &v, const Vec3 &m, double &dlog)
{
#pragma clang fp contract(off)
    const double vm = __builtin_fma(v.x, m.x, __builtin_fma(v.y, m.y, v.z * m.z));
    const double vz2 = v.z * v.z;
    const double s2 = 1.0 - vz2;
    const double az = __builtin_fabs(v.z);
    double q, rq;
    sqrt_rsqrt(__builtin_fma(g.alpha * g.alpha, s2, vz2), q, rq);
    const double inv = rcp_nr(__builtin_fmax(az + q, kTiny));
    const bool flat = s2 <= 0.0;
    dlog = flat ? 0.0 : -(g.alpha * s2) * (rq * inv);
    const double res = flat ? 1.0 : 2.0 * az * inv;
    return vm * v.z <= 0.0 ? 0.0 : res;
}

// F and its derivatives with respect to E = eta^2 - k^2 (GgxConsts::eta2_k2) and Q = 4 k^2 eta^2 (four_k2_eta2); the caller's
// chain rule is dF/d eta = 2 eta F_E + 8 k^2 eta F_Q, dF/dk = -2 k F_E + 8 k eta^2 F_Q.
// With A = sqrt(t1^2 + Q) and a = sqrt((A + t1) / 2):  A_E = t1 / A, A_Q = 1 / (2 A), a_E = a / (2 A), a_Q = 1 / (8 A a);
// Rs = (T1 - T2) / (T1 + T2) gives dRs = 2 (T2 dT1 - T1 dT2) / (T1 + T2)^2, likewise P = (T3 - T4) / (T3 + T4); F = Rs (1 + P) / 2.
MRL_HD double fresnel_conductor_d(const GgxConsts &g, int ch, double c, double &dE, double &dQ)
{
#pragma clang fp contract(off)
    const double c2 = c * c, s2 = 1.0 - c2, s4 = s2 * s2;
    const double t1 = g.eta2_k2[ch] - s2;
    double A, rA, a, ra;
    sqrt_rsqrt(__builtin_fma(t1, t1, g.four_k2_eta2[ch]), A, rA);
    sqrt_rsqrt(0.5 * (A + t1), a, ra);
    const double term1 = A + c2, term2 = 2.0 * a * c;
    const double term3 = __builtin_fma(A, c2, s4), term4 = term2 * s2;
    const double d12 = term1 + term2, d34 = term3 + term4;
    const double inv = rcp_nr(d12 * d34);
    const double inv12 = d34 * inv, inv34 = d12 * inv;
    const double rs = (term1 - term2) * inv12, p1 = 1.0 + (term3 - term4) * inv34;
    const double k12 = 2.0 * (inv12 * inv12) * p1, k34 = 2.0 * (inv34 * inv34) * rs;
    const double two_c = 2.0 * c;
    // dT1 = dA, dT2 = 2 c da, dT3 = c^2 dA, dT4 = 2 c s2 da
    const double A_E = t1 * rA, A_Q = 0.5 * rA, a_E = 0.5 * (a * rA), a_Q = 0.125 * (rA * ra);
    const double t2_E = two_c * a_E, t2_Q = two_c * a_Q;
    dE = 0.5 * __builtin_fma(k12, __builtin_fma(term2, A_E, -(term1 * t2_E)), k34 * __builtin_fma(term4 * c2, A_E, -(term3 * s2 * t2_E)));
    dQ = 0.5 * __builtin_fma(k12, __builtin_fma(term2, A_Q, -(term1 * t2_Q)), k34 * __builtin_fma(term4 * c2, A_Q, -(term3 * s2 * t2_Q)));
    return 0.5 * (rs * p1);
}

// eval of one pair of unit directions and its Jacobian J[c] = d eval_c / d (alpha, eta_c, k_c) at the material's parameters.
// live == false: one of eval's own D / G1 selects returned 0 (the values are then not to be used)
struct GgxJacobian {
    double d_alpha[3], d_eta[3], d_k[3];
    bool live;
};
MRL_HD GgxJacobian ggx_eval_jacobian(const GgxConsts &g, const double eta[3], const double k[3], const Vec3 &in, const Vec3 &out)
{
#pragma clang fp contract(off)
    const Vec3 m = unit_sum(in, out);
    double lD, lGi, lGo;
    const double D = ggx_D_dlog(g, m, lD);
    const double G1i = ggx_G1_dlog(g, in, m, lGi);
    const double G1o = ggx_G1_dlog(g, out, m, lGo);
    const double model = D * G1i * (0.25 * rcp_nr(in.z)) * G1o;
    const double dlog = lD + lGi + lGo;
    const double c = __builtin_fma(in.x, m.x, __builtin_fma(in.y, m.y, in.z * m.z));
    GgxJacobian j;
    j.live = D != 0.0 && G1i != 0.0 && G1o != 0.0;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        double fE, fQ;
        const double F = fresnel_conductor_d(g, ch, c, fE, fQ);
        const double e2 = eta[ch] * eta[ch], k2 = k[ch] * k[ch];
        j.d_alpha[ch] = F * model * dlog;
        j.d_eta[ch] = model * (2.0 * eta[ch] * __builtin_fma(4.0 * k2, fQ, fE));
        // F is even in k: at k = 0 the derivative is 0 whatever fE and fQ are
        j.d_k[ch] = k[ch] == 0.0 ? 0.0 : model * (2.0 * k[ch] * __builtin_fma(4.0 * e2, fQ, -fE));
    }
    return j;
}

// ---- the direction gradient of eval (merl_ggx_dir_grad.hip) ----
// eval_c = F_c(c) M with M = D(m) G1(a) G1(b) / (4 a_z), a = wi / |wi|, b = wo / |wo|, h = a + b, m = h / |h|, c = a . m.  Only two
// scalars depend on the channel, A = M sum g_c F_c and B = M sum g_c dF_c/dc; the vectors are channel-free:
//     d/da = A (dlnD/dm_z (e_z - m m_z) / |h| + (dlnG1/da_z - 1/a_z) e_z) + B (m + (a - c m) / |h|)
//     d/db = A (dlnD/dm_z (e_z - m m_z) / |h| +  dlnG1/db_z          e_z) + B      (a - c m) / |h|
// (m = h / |h| pulls a vector v back to (v - m (m . v)) / |h|), and wi's gradient is (d/da - a (a . d/da)) / |wi|, likewise wo's.
// On unit vectors D depends on m_z alone and G1(v) on v_z alone, and both enter through LOG-derivatives, as the alpha-derivatives
// above do: nothing is divided by a D or G1 that vanishes.  Contraction is off and every fused multiply-add is spelt out: the
// single-material and the material-per-lane kernel, with and without a queue, must round alike.

// the constants of a material from its parameters, rounded the same way wherever this is inlined (the constructor above leaves
// its contraction to the compiler)
MRL_HD GgxConsts ggx_consts_exact(double alpha, const double eta[3], const double k[3])
{
#pragma clang fp contract(off)
    GgxConsts g;
    g.alpha = alpha;
    g.inv_alpha2 = rcp_nr(alpha * alpha);
    g.inv_pi_alpha2 = g.inv_alpha2 * 0.31830988618379067154;
    for (int c = 0; c < 3; ++c) {
        const double e2 = eta[c] * eta[c], k2 = k[c] * k[c];
        g.eta2_k2[c] = e2 - k2;
        g.four_k2_eta2[c] = 4.0 * k2 * e2;
    }
    return g;
}

// D as ggx_D_dlog returns it, and d ln D / d m_z on the unit sphere: root = s / a^2 + m_z^2 with s = 1 - m_z^2 gives
// d root / d m_z = 2 m_z (1 - 1 / a^2) and ln D = -2 ln root + const
MRL_HD double ggx_D_dz(const GgxConsts &g, const Vec3 &m, double &dlog)
{
#pragma clang fp contract(off)
    const double s_a2 = __builtin_fma(m.x, m.x, m.y * m.y) * g.inv_alpha2, c2 = m.z * m.z;
    const double inv = rcp_nr(__builtin_fmax(s_a2 + c2, kTiny));
    const double r = g.inv_pi_alpha2 * (inv * inv);
    dlog = 4.0 * (g.inv_alpha2 - 1.0) * (m.z * inv);
    return (m.z <= 0.0 || r * m.z < 1e-20) ? 0.0 : r;
}

// G1 as ggx_G1_dlog returns it, 1 / v_z, and d ln G1 / d v_z on the unit sphere: with q = sqrt(v_z^2 + a^2 (1 - v_z^2)),
// 1 / v_z - (1 + dq/dv_z) / (v_z + q) = a^2 / (v_z q (v_z + q)).  The exact-normal select (G1 = 1) has derivative 0.
MRL_HD double ggx_G1_dz(const GgxConsts &g, const Vec3 &v, const Vec3 &m, double &dlog, double &inv_vz)
{
#pragma clang fp contract(off)
    const double vm = __builtin_fma(v.x, m.x, __builtin_fma(v.y, m.y, v.z * m.z));
    const double vz2 = v.z * v.z;
    const double s2 = 1.0 - vz2;
    const double az = __builtin_fabs(v.z);
    double q, rq;
    sqrt_rsqrt(__builtin_fma(g.alpha * g.alpha, s2, vz2), q, rq);
    const double inv = rcp_nr(__builtin_fmax(az + q, kTiny));
    inv_vz = rcp_nr(v.z);
    const bool flat = s2 <= 0.0;
    dlog = flat ? 0.0 : (g.alpha * g.alpha) * (rq * inv) * inv_vz;
    const double res = flat ? 1.0 : 2.0 * az * inv;
    return vm * v.z <= 0.0 ? 0.0 : res;
}

// F as fresnel_conductor_d returns it, and dF/dc from the same square roots and reciprocal.  With s2 = 1 - c^2, t1 = E - s2,
// A = sqrt(t1^2 + Q), a = sqrt((A + t1) / 2):  dt1 = 2c, dA = 2c t1 / A, da = (dA + dt1) / (4a) = c a / A;
// dT1 = dA + 2c, dT2 = 2 (a + c da), dT3 = c^2 dA + 2c (A - 2 s2), dT4 = s2 dT2 - 2c T2; dRs and dP as in fresnel_conductor_d.
MRL_HD double fresnel_conductor_dc(const GgxConsts &g, int ch, double c, double &dc)
{
#pragma clang fp contract(off)
    const double c2 = c * c, s2 = 1.0 - c2, s4 = s2 * s2;
    const double t1 = g.eta2_k2[ch] - s2;
    double A, rA, a, ra;
    sqrt_rsqrt(__builtin_fma(t1, t1, g.four_k2_eta2[ch]), A, rA);
    sqrt_rsqrt(0.5 * (A + t1), a, ra);
    const double term1 = A + c2, term2 = 2.0 * a * c;
    const double term3 = __builtin_fma(A, c2, s4), term4 = term2 * s2;
    const double d12 = term1 + term2, d34 = term3 + term4;
    const double inv = rcp_nr(d12 * d34);
    const double inv12 = d34 * inv, inv34 = d12 * inv;
    const double rs = (term1 - term2) * inv12, p1 = 1.0 + (term3 - term4) * inv34;
    const double k12 = 2.0 * (inv12 * inv12) * p1, k34 = 2.0 * (inv34 * inv34) * rs;
    const double two_c = 2.0 * c;
    const double dA = two_c * (t1 * rA);
    const double dT1 = dA + two_c;
    const double dT2 = 2.0 * (a * __builtin_fma(c2, rA, 1.0));
    const double dT3 = __builtin_fma(c2, dA, two_c * (A - 2.0 * s2));
    const double dT4 = __builtin_fma(s2, dT2, -(two_c * term2));
    dc = 0.5 * __builtin_fma(k12, __builtin_fma(term2, dT1, -(term1 * dT2)), k34 * __builtin_fma(term4, dT3, -(term3 * dT4)));
    return 0.5 * (rs * p1);
}

// sum_c g_c d eval_c / d wi and the same in wo, for one pair of raw Float directions (the normalisation is part of the function: each
// gradient is orthogonal to its direction and scales with 1 / |w|).  A unit that eval masks, or for which one of eval's D / G1
// selects returns 0, gets +0 in both — by selects at the end: its values are garbage and its g may be NaN.
struct GgxDirGrad { float wi[3], wo[3]; };
MRL_HD GgxDirGrad ggx_eval_dir_grad(const GgxConsts &g, float wix, float wiy, float wiz, float wox, float woy, float woz, const float g32[3])
{
#pragma clang fp contract(off)
    const Dir di = dir_f32(wix, wiy, wiz), dout = dir_f32(wox, woy, woz);
    const Vec3 a = unit(di), b = unit(dout);
    const double hx = a.x + b.x, hy = a.y + b.y, hz = a.z + b.z;
    double L, rL;
    sqrt_rsqrt(__builtin_fma(hx, hx, __builtin_fma(hy, hy, hz * hz)), L, rL);
    const Vec3 m = { hx * rL, hy * rL, hz * rL };
    double kD, kGa, kGb, inv_az, inv_bz;
    const double D = ggx_D_dz(g, m, kD);
    const double G1a = ggx_G1_dz(g, a, m, kGa, inv_az);
    const double G1b = ggx_G1_dz(g, b, m, kGb, inv_bz);
    const double M = D * G1a * (0.25 * inv_az) * G1b;
    const double c = __builtin_fma(a.x, m.x, __builtin_fma(a.y, m.y, a.z * m.z));
    double sF = 0.0, sdF = 0.0;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        double dF;
        const double F = fresnel_conductor_dc(g, ch, c, dF);
        const double gc = (double)g32[ch];
        sF = __builtin_fma(gc, F, sF);
        sdF = __builtin_fma(gc, dF, sdF);
    }
    const double A = M * sF, B = M * sdF;
    // what both sides share: T = (A dlnD/dm_z / |h|) (e_z - m m_z) + (B / |h|) (a - c m); the z of e_z - m m_z is m_x^2 + m_y^2
    const double p = A * kD * rL, q = B * rL;
    const double tx = __builtin_fma(p, -(m.x * m.z), q * __builtin_fma(-c, m.x, a.x));
    const double ty = __builtin_fma(p, -(m.y * m.z), q * __builtin_fma(-c, m.y, a.y));
    const double tz = __builtin_fma(p, __builtin_fma(m.x, m.x, m.y * m.y), q * __builtin_fma(-c, m.z, a.z));
    const double vax = __builtin_fma(B, m.x, tx), vay = __builtin_fma(B, m.y, ty);
    const double vaz = __builtin_fma(B, m.z, __builtin_fma(A, kGa - inv_az, tz));
    const double vbz = __builtin_fma(A, kGb, tz);
    const double da = __builtin_fma(a.x, vax, __builtin_fma(a.y, vay, a.z * vaz));
    const double db = __builtin_fma(b.x, tx, __builtin_fma(b.y, ty, b.z * vbz));
    const float poison = cos_or_nan32((wix + wiy + wiz), wox, woy, woz, true);
    const bool live = (wiz > 0.0f) && (woz > 0.0f) && (poison == poison) && D != 0.0 && G1a != 0.0 && G1b != 0.0;
    GgxDirGrad r;
    r.wi[0] = live ? (float)(__builtin_fma(-a.x, da, vax) * di.rs) : 0.0f;
    r.wi[1] = live ? (float)(__builtin_fma(-a.y, da, vay) * di.rs) : 0.0f;
    r.wi[2] = live ? (float)(__builtin_fma(-a.z, da, vaz) * di.rs) : 0.0f;
    r.wo[0] = live ? (float)(__builtin_fma(-b.x, db, tx) * dout.rs) : 0.0f;
    r.wo[1] = live ? (float)(__builtin_fma(-b.y, db, ty) * dout.rs) : 0.0f;
    r.wo[2] = live ? (float)(__builtin_fma(-b.z, db, vbz) * dout.rs) : 0.0f;
    return r;
}

// ---- the gradient of pdf (merl_ggx_sample_grad.hip) ----
// P = D(m) G1(a) / (4 a_z) with a, b, h, m as above: ln P = ln D(m_z) + ln G1(a_z) - ln a_z, so with A = g P
//     d/da = A (dlnD/dm_z (e_z - m m_z) / |h| + (dlnG1/da_z - 1/a_z) e_z)        d/db = A dlnD/dm_z (e_z - m m_z) / |h|
//     d/dalpha = A (dlnD/dalpha + dlnG1(a)/dalpha)
// the same twins, the same pull-back through the two normalisations and the same selects at the end as ggx_eval_dir_grad.
struct GgxPdfGrad { float wi[3], wo[3], alpha; };
MRL_HD GgxPdfGrad ggx_pdf_grad(const GgxConsts &g, float wix, float wiy, float wiz, float wox, float woy, float woz, float g32)
{
#pragma clang fp contract(off)
    const Dir di = dir_f32(wix, wiy, wiz), dout = dir_f32(wox, woy, woz);
    const Vec3 a = unit(di), b = unit(dout);
    const double hx = a.x + b.x, hy = a.y + b.y, hz = a.z + b.z;
    double L, rL;
    sqrt_rsqrt(__builtin_fma(hx, hx, __builtin_fma(hy, hy, hz * hz)), L, rL);
    const Vec3 m = { hx * rL, hy * rL, hz * rL };
    double kD, kGa, inv_az, lD, lGa;
    const double D = ggx_D_dz(g, m, kD);
    const double G1a = ggx_G1_dz(g, a, m, kGa, inv_az);
    (void)ggx_D_dlog(g, m, lD);
    (void)ggx_G1_dlog(g, a, m, lGa);
    const double A = (double)g32 * (D * G1a * (0.25 * inv_az));
    const double p = A * kD * rL;
    const double tx = p * -(m.x * m.z), ty = p * -(m.y * m.z), tz = p * __builtin_fma(m.x, m.x, m.y * m.y);
    const double vaz = __builtin_fma(A, kGa - inv_az, tz);
    const double da = __builtin_fma(a.x, tx, __builtin_fma(a.y, ty, a.z * vaz));
    const double db = __builtin_fma(b.x, tx, __builtin_fma(b.y, ty, b.z * tz));
    const float poison = cos_or_nan32((wix + wiy + wiz), wox, woy, woz, true);
    const bool live = (wiz > 0.0f) && (woz > 0.0f) && (poison == poison) && D != 0.0 && G1a != 0.0;
    GgxPdfGrad r;
    r.wi[0] = live ? (float)(__builtin_fma(-a.x, da, tx) * di.rs) : 0.0f;
    r.wi[1] = live ? (float)(__builtin_fma(-a.y, da, ty) * di.rs) : 0.0f;
    r.wi[2] = live ? (float)(__builtin_fma(-a.z, da, vaz) * di.rs) : 0.0f;
    r.wo[0] = live ? (float)(__builtin_fma(-b.x, db, tx) * dout.rs) : 0.0f;
    r.wo[1] = live ? (float)(__builtin_fma(-b.y, db, ty) * dout.rs) : 0.0f;
    r.wo[2] = live ? (float)(__builtin_fma(-b.z, db, tz) * dout.rs) : 0.0f;
    r.alpha = live ? (float)(A * (lD + lGa)) : 0.0f;
    return r;
}

// sin / cos of 2 pi u for u in [0,1): only the normal-incidence branch of the sampler needs it.  That branch is taken
// when the stretched s_z >= 0.99999, i.e. alpha tan(theta_i) < 4.47e-3: almost never at alpha >= 0.1, but for every
// incident direction up to 77 degrees at alpha = 1e-3 — for smooth materials it is the sampler's main branch.
MRL_HD void sincos_2pi(double u, double &s, double &c)
{   // declared in merl_table_fast.hpp
    // octant reduction: 2 pi u = q pi/2 + t, |t| <= pi/4
    const double x = 4.0 * u;
    const double q = __builtin_rint(x);
    const double t = (x - q) * kHalfPi;
    const double z = t * t;
    double ps = -2.5052108385441720e-08;           // Taylor coefficients: |t| <= pi/4 gives < 1e-13 abs error
    ps = __builtin_fma(ps, z, 2.7557319223985893e-06);
    ps = __builtin_fma(ps, z, -1.9841269841269841e-04);
    ps = __builtin_fma(ps, z, 8.3333333333333332e-03);
    ps = __builtin_fma(ps, z, -1.6666666666666666e-01);
    const double st = __builtin_fma(ps * z, t, t);
    double pc = 2.0876756987868099e-09;
    pc = __builtin_fma(pc, z, -2.7557319223985888e-07);
    pc = __builtin_fma(pc, z, 2.4801587301587302e-05);
    pc = __builtin_fma(pc, z, -1.3888888888888889e-03);
    pc = __builtin_fma(pc, z, 4.1666666666666664e-02);
    pc = __builtin_fma(pc, z, -0.5);
    const double ct = __builtin_fma(pc, z, 1.0);
    const int qi = (int)q & 3;
    s = qi == 0 ? st : (qi == 1 ? ct : (qi == 2 ? -st : -ct));
    c = qi == 0 ? ct : (qi == 1 ? -st : (qi == 2 ? -ct : st));
}

// visible-normal sampling (Heitz & d'Eon 2014); returns false when the sample is rejected
__device__ __forceinline__ bool ggx_sample(const GgxConsts &g, const Vec3 &in, float u0, float u1,
                                           float wo[3], float &pdf, float weight[3])
{
    const double al = g.alpha;
    // 1. stretch
    double sx = al * in.x, sy = al * in.y, sz = in.z;
    double sl, srs;
    sqrt_rsqrt(__builtin_fma(sx, sx, __builtin_fma(sy, sy, sz * sz)), sl, srs);
    sx *= srs; sy *= srs; sz *= srs;
    double slx, sly, cp = 1.0, sp = 0.0;
    double u2 = (double)u1;
    if (sz < 0.99999) {
        // 2. P22 slopes for alpha = 1; tan(theta) and (cos phi, sin phi) straight from the stretched vector
        double rho, rrho;
        sqrt_rsqrt(__builtin_fma(sx, sx, sy * sy), rho, rrho);
        cp = sx * rrho; sp = sy * rrho;
        const double inv_tan = sz * rrho;
        const double tan_i = rho * rcp_nr(sz);
        const double G1 = 2.0 * rcp_nr(1.0 + sqrt_fast(__builtin_fma(tan_i, tan_i, 1.0)));
        double A = __builtin_fma(2.0 * (double)u0, rcp_nr(G1), -1.0);
        if (__builtin_fabs(A) == 1.0) A -= (A > 0 ? 1.0 : -1.0) * 1e-12;
        const double tmp = rcp_nr(__builtin_fma(A, A, -1.0));
        const double B = tan_i;
        const double disc = B * B * tmp * tmp - (A * A - B * B) * tmp;
        const double D = disc > 0.0 ? sqrt_fast(disc) : 0.0;
        const double s1 = B * tmp - D, s2 = B * tmp + D;
        slx = (A < 0.0 || s2 > inv_tan) ? s1 : s2;
        double S;
        if (u2 > 0.5) { S = 1.0; u2 = 2.0 * (u2 - 0.5); }
        else { S = -1.0; u2 = 2.0 * (0.5 - u2); }
        const double num = u2 * (u2 * (u2 * (-0.365728915865723) + 0.790235037209296) - 0.424965825137544) + 0.000152998850436920;
        const double den = u2 * (u2 * (u2 * (u2 * 0.169507819808272 - 0.397203533833404) - 0.232500544458471) + 1.0) - 0.539825872510702;
        sly = S * num * rcp_nr(den) * sqrt_fast(__builtin_fma(slx, slx, 1.0));
    } else {
        // normal incidence: theta = phi = 0
        const double q = (double)u0 * rcp_nr(1.0 - (double)u0);
        const double r = q > 0.0 ? sqrt_fast(q) : 0.0;
        double s2pi, c2pi;
        sincos_2pi(u2, s2pi, c2pi);
        slx = r * c2pi; sly = r * s2pi;
    }
    // 3. rotate, 4. unstretch, 5. normal
    const double mx = (cp * slx - sp * sly) * al, my = (sp * slx + cp * sly) * al;
    double nl, nrm;
    sqrt_rsqrt(__builtin_fma(mx, mx, __builtin_fma(my, my, 1.0)), nl, nrm);
    const Vec3 m = { -mx * nrm, -my * nrm, nrm };
    const double c = __builtin_fma(in.x, m.x, __builtin_fma(in.y, m.y, in.z * m.z));
    const Vec3 out = { __builtin_fma(2.0 * c, m.x, -in.x), __builtin_fma(2.0 * c, m.y, -in.y), __builtin_fma(2.0 * c, m.z, -in.z) };
    const double D = ggx_D(g, m);
    const double p = D * ggx_G1(g, in, m) * 0.25 * rcp_nr(in.z);
    const float wx = (float)out.x, wy = (float)out.y, wz = (float)out.z;
    const bool ok = (out.z > 0.0) && (c > 0.0) && (p > 0.0) && (wz > 0.0f);
    const double G1o = ggx_G1(g, out, m);
    wo[0] = ok ? wx : 0.0f; wo[1] = ok ? wy : 0.0f; wo[2] = ok ? wz : 0.0f;
    pdf = ok ? (float)p : 0.0f;
    weight[0] = ok ? (float)(fresnel_conductor(g, 0, c) * G1o) : 0.0f;
    weight[1] = ok ? (float)(fresnel_conductor(g, 1, c) * G1o) : 0.0f;
    weight[2] = ok ? (float)(fresnel_conductor(g, 2, c) * G1o) : 0.0f;
    return ok;
}

// ---- the gradient of sample (merl_ggx_sample_grad.hip) ----
// (wo', p', w') = ggx_sample(wi, u) before its results are rounded to Float, differentiated in wi and in (alpha, eta, k) on the
// branch the forward call takes — every select of ggx_sample above is held fixed, and so is u.  The forward chain is recomputed
// with ggx_sample's own expressions for out.z, c and p and its (float)out.z > 0 test, then ONE reverse sweep carries the seven
// cotangents go = (g_wo xyz, g_pdf, g_weight rgb) back:
//     w'_c = F_c(c) G1(o)          c~ = G1(o) sum g_w F'_c          weight on ln G1(o):  W = G1(o) sum g_w F_c
//     p'   = D(m) G1(i) / (4 i_z)  weight on ln p':  P = g_p p'
//     o    = 2 c m - i             o~ = g_wo + W dlnG1/do_z e_z;    c~ += 2 o~ . m;   m~ = 2 c o~ + c~ i + P dlnD/dm_z e_z
//                                  i~ = -o~ + c~ m + P (dlnG1/di_z - 1/i_z) e_z
//     m    = n / |n|, n = (-m_x, -m_y, 1):  n~ = (m~ - m (m . m~)) / |n|   (which also projects D's sphere gradient)
//     (m_x, m_y) = alpha R(phi) (sl_x, sl_y):  alpha~ += n~ . d n / d alpha, and through the rotation to sl~, cos~, sin~
//     general branch: sl_y = Z sqrt(1 + sl_x^2) (Z is a function of u alone) and sl_x = sl_x(B), B = tan(theta) of the stretched
//     direction = alpha |i_xy| / i_z, (cos phi, sin phi) = i_xy / |i_xy| (the stretch cancels): B~ and the rotation go to i~, alpha~.
//     normal-incidence branch: the slopes depend on u alone and phi = 0.
// d sl_x / d B is taken from the closed form of the forward's root: with T = 1 / (A^2 - 1) and R = sqrt(1 + B^2 - A^2) the forward's
// disc is T^2 A^2 R^2, so sl_x = T (B + s A R), s = -+1 the sign the forward's selects fix — the forward's own expression for disc
// cancels to 0 at A -> 0 and its derivative cannot be taken term by term.  A = u0 (1 + sqrt(1 + B^2)) - 1 gives A' = u0 B / sqrt(1 + B^2).
// A unit is dead exactly when the forward rejects it (pdf = 0): selects at the end, its values are garbage and its go may be NaN.
struct GgxSampleGrad { float wi[3], params[7]; };
MRL_HD GgxSampleGrad ggx_sample_grad(const GgxConsts &g, const double eta[3], const double k[3], float wix, float wiy, float wiz,
                                     float u0, float u1, const float go[7])
{
#pragma clang fp contract(off)
    const Dir di = dir_f32(wix, wiy, wiz);
    const Vec3 in = unit(di);
    const double al = g.alpha;
    // ---- forward, as ggx_sample
    double sx = al * in.x, sy = al * in.y, sz = in.z;
    double sl, srs;
    sqrt_rsqrt(__builtin_fma(sx, sx, __builtin_fma(sy, sy, sz * sz)), sl, srs);
    sx *= srs; sy *= srs; sz *= srs;
    double slx, sly, cp = 1.0, sp = 0.0;
    double u2 = (double)u1;
    const bool general = sz < 0.99999;
    double B = 0.0, slx_B = 0.0, sly_slx = 0.0, inv_rho = 0.0;       // B, d sl_x / d B, d sl_y / d sl_x, 1 / |i_xy|
    if (general) {
        double rho, rrho;
        sqrt_rsqrt(__builtin_fma(sx, sx, sy * sy), rho, rrho);
        cp = sx * rrho; sp = sy * rrho;
        inv_rho = al * srs * rrho;
        const double inv_tan = sz * rrho;
        const double tan_i = rho * rcp_nr(sz);
        const double q1 = sqrt_fast(__builtin_fma(tan_i, tan_i, 1.0));
        const double G1 = 2.0 * rcp_nr(1.0 + q1);
        double A = __builtin_fma(2.0 * (double)u0, rcp_nr(G1), -1.0);
        if (__builtin_fabs(A) == 1.0) A -= (A > 0 ? 1.0 : -1.0) * 1e-12;
        const double tmp = rcp_nr(__builtin_fma(A, A, -1.0));
        B = tan_i;
        const double disc = B * B * tmp * tmp - (A * A - B * B) * tmp;
        const double Dq = disc > 0.0 ? sqrt_fast(disc) : 0.0;
        const double s1 = B * tmp - Dq, s2 = B * tmp + Dq;
        const bool first = A < 0.0 || s2 > inv_tan;
        slx = first ? s1 : s2;
        double S;
        if (u2 > 0.5) { S = 1.0; u2 = 2.0 * (u2 - 0.5); }
        else { S = -1.0; u2 = 2.0 * (0.5 - u2); }
        const double num = u2 * (u2 * (u2 * (-0.365728915865723) + 0.790235037209296) - 0.424965825137544) + 0.000152998850436920;
        const double den = u2 * (u2 * (u2 * (u2 * 0.169507819808272 - 0.397203533833404) - 0.232500544458471) + 1.0) - 0.539825872510702;
        const double n2 = __builtin_fma(slx, slx, 1.0);
        sly = S * num * rcp_nr(den) * sqrt_fast(n2);
        // d sl_x / d B from sl_x = T (B + s A R)
        const double sgn = (first ? -1.0 : 1.0) * (tmp < 0.0 ? -1.0 : 1.0) * (A < 0.0 ? -1.0 : 1.0);
        const double s = (disc > 0.0 && A != 0.0) ? sgn : 0.0;
        double R, rR;
        sqrt_rsqrt((q1 - A) * (q1 + A), R, rR);
        const double A_B = (double)u0 * B * rcp_nr(q1);
        const double AR_B = __builtin_fma(A_B, R, A * __builtin_fma(-A, A_B, B) * rR);
        slx_B = tmp * __builtin_fma(s, AR_B, __builtin_fma(-2.0 * A * A_B, slx, 1.0));
        sly_slx = sly * slx * rcp_nr(n2);
    } else {
        const double q = (double)u0 * rcp_nr(1.0 - (double)u0);
        const double r = q > 0.0 ? sqrt_fast(q) : 0.0;
        double s2pi, c2pi;
        sincos_2pi(u2, s2pi, c2pi);
        slx = r * c2pi; sly = r * s2pi;
    }
    const double rx = cp * slx - sp * sly, ry = sp * slx + cp * sly;
    const double mx = rx * al, my = ry * al;
    double nl, nrm;
    sqrt_rsqrt(__builtin_fma(mx, mx, __builtin_fma(my, my, 1.0)), nl, nrm);
    const Vec3 m = { -mx * nrm, -my * nrm, nrm };
    const double c = __builtin_fma(in.x, m.x, __builtin_fma(in.y, m.y, in.z * m.z));
    const Vec3 out = { __builtin_fma(2.0 * c, m.x, -in.x), __builtin_fma(2.0 * c, m.y, -in.y), __builtin_fma(2.0 * c, m.z, -in.z) };
    double kD, kGi, kGo, inv_iz, inv_oz, lD, lGi, lGo;
    const double D = ggx_D_dz(g, m, kD);
    const double G1i = ggx_G1_dz(g, in, m, kGi, inv_iz);
    const double G1o = ggx_G1_dz(g, out, m, kGo, inv_oz);
    (void)ggx_D_dlog(g, m, lD);
    (void)ggx_G1_dlog(g, in, m, lGi);
    (void)ggx_G1_dlog(g, out, m, lGo);
    const double p = D * G1i * 0.25 * inv_iz;
    // ggx_sample's decision restated, and the wi.z > 0 its callers add; a NaN / inf wi fails it as it fails theirs: its c is NaN.
    // The same expressions, NOT the same instructions: ggx_sample leaves contraction to the compiler and takes D, G1 and the
    // material's constants from ggx_D, ggx_G1 and the GgxConsts constructor, this copy has contraction off and takes them from the
    // twins and ggx_consts_exact, so out.z, c and p can differ from the forward's in the last bits and a unit within that of a
    // threshold can be decided the other way.  The tests hold the two dead sets equal on every unit they run.
    const bool ok = (wiz > 0.0f) && (out.z > 0.0) && (c > 0.0) && (p > 0.0) && ((float)out.z > 0.0f);
    // ---- reverse
    const double gp = (double)go[3];
    double sF = 0.0, sdF = 0.0, g_eta[3], g_k[3];
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        double dF, fE, fQ;
        const double F = fresnel_conductor_dc(g, ch, c, dF);
        (void)fresnel_conductor_d(g, ch, c, fE, fQ);
        const double gw = (double)go[4 + ch] * G1o;
        sF = __builtin_fma(gw, F, sF);
        sdF = __builtin_fma(gw, dF, sdF);
        const double e2 = eta[ch] * eta[ch], k2 = k[ch] * k[ch];
        g_eta[ch] = gw * (2.0 * eta[ch] * __builtin_fma(4.0 * k2, fQ, fE));
        // F is even in k: at k = 0 the derivative is 0 whatever fE and fQ are
        g_k[ch] = k[ch] == 0.0 ? 0.0 : gw * (2.0 * k[ch] * __builtin_fma(4.0 * e2, fQ, -fE));
    }
    const double P = gp * p;
    double g_alpha = __builtin_fma(P, lD + lGi, sF * lGo);
    const double obx = (double)go[0], oby = (double)go[1], obz = __builtin_fma(sF, kGo, (double)go[2]);
    const double cb = __builtin_fma(2.0, __builtin_fma(obx, m.x, __builtin_fma(oby, m.y, obz * m.z)), sdF);
    const double mbx = __builtin_fma(2.0 * c, obx, cb * in.x), mby = __builtin_fma(2.0 * c, oby, cb * in.y);
    const double mbz = __builtin_fma(2.0 * c, obz, __builtin_fma(cb, in.z, P * kD));
    double ibx = __builtin_fma(cb, m.x, -obx), iby = __builtin_fma(cb, m.y, -oby);
    double ibz = __builtin_fma(cb, m.z, __builtin_fma(P, kGi - inv_iz, -obz));
    const double md = __builtin_fma(m.x, mbx, __builtin_fma(m.y, mby, m.z * mbz));
    const double mxb = -(__builtin_fma(-m.x, md, mbx) * nrm), myb = -(__builtin_fma(-m.y, md, mby) * nrm);     // cotangents of m_x, m_y
    g_alpha = __builtin_fma(mxb, rx, __builtin_fma(myb, ry, g_alpha));
    const double rxb = al * mxb, ryb = al * myb;
    if (general) {
        const double slyb = __builtin_fma(-sp, rxb, cp * ryb);
        const double slxb = __builtin_fma(cp, rxb, __builtin_fma(sp, ryb, slyb * sly_slx));
        const double cpb = __builtin_fma(slx, rxb, sly * ryb), spb = __builtin_fma(-sly, rxb, slx * ryb);
        const double Bb = slxb * slx_B * B;                          // B~ B: every use of B~ carries the factor B
        const double t = __builtin_fma(-sp, cpb, cp * spb) * inv_rho;
        g_alpha = __builtin_fma(Bb, al * g.inv_alpha2, g_alpha);
        ibx += __builtin_fma(Bb * inv_rho, cp, -(sp * t));
        iby += __builtin_fma(Bb * inv_rho, sp, cp * t);
        ibz -= Bb * inv_iz;
    }
    const double dd = __builtin_fma(in.x, ibx, __builtin_fma(in.y, iby, in.z * ibz));
    GgxSampleGrad r;
    r.wi[0] = ok ? (float)(__builtin_fma(-in.x, dd, ibx) * di.rs) : 0.0f;
    r.wi[1] = ok ? (float)(__builtin_fma(-in.y, dd, iby) * di.rs) : 0.0f;
    r.wi[2] = ok ? (float)(__builtin_fma(-in.z, dd, ibz) * di.rs) : 0.0f;
    r.params[0] = ok ? (float)g_alpha : 0.0f;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) { r.params[1 + ch] = ok ? (float)g_eta[ch] : 0.0f; r.params[4 + ch] = ok ? (float)g_k[ch] : 0.0f; }
    return r;
}

} // namespace fast
} // namespace mrl
