// merl_nch_dir_grad.hpp — the per-lane gradient of eval in the directions on an n-channel table material (include/merl_hip_diff_nch.h,
// DESIGN.md §5k): the function k_table_grad_dir_nch runs, __host__ __device__ and free of HIP calls so that a host harness can run it.
//
// The operator and the math are those of merl_table_dir_grad.hpp with c running over n_ch channels: E_c = T_c(x(a, b)) kappa, T_c the
// exact trilinear interpolant of the stored Float texels in the cell eval_nch selects (trilinear_cell / nearest_cell of merl_device.hpp, which nch_cell of
// merl_nch.hip and fast::dir_cell both call: the RGB path's split, shift and clamps).  Step 1 walks the cell's channel groups:
//   t_k = sum_c g_c (f[k][c] - f[0][c]), k = 1 .. 7, each difference exact in f64 BEFORE it meets g;   base = sum_c g_c f[0][c],
// both accumulated channel by channel in ascending channel order in ONE chain, t = g_0 d_0, then t = fma(g_c, d_c, t): for three
// channels this is the RGB function's expression, and a channel whose g is 0 leaves the chain's value as it was — an RGB table embedded
// in a wider one returns the RGB function's numbers.  Channels >= n_ch of a padded group are never read from g and never enter a sum.
// Steps 2 and 3 — V, D_h, D_d, D_p, the clamp / nearest masks, the pull-back, the normalisations, the cosine term, the dead-unit select —
// ARE fast::dir_forms and fast::dir_tail of merl_table_dir_grad.hpp.
// Only the seven t_k, base and two groups' texels are live across the group loop (the next group's loads are issued before the
// current group is contracted), not n_ch channels.  Contraction is off and the FMAs are spelt out.
#pragma once
#include "merl_table_dir_grad.hpp"

namespace mrl {
namespace fast {

// a stream value read once
MRL_HD float nch_stream(const float *p) { return __builtin_nontemporal_load(p); }

// one channel group of a cell as loaded: corner-major, v[k * CPAD + ch] (the brick of merl_nch.hip), and the group's g
template <int CPAD>
struct NchGroup { float4 q[2 * CPAD]; float g[CPAD]; };

// all loads of group `group` of the cell at `cell` (its first brick): 2 CPAD sixteen-byte pieces and up to CPAD floats of g
template <int CPAD>
MRL_HD void nch_load_group(const float4 *cell, const float *g, int group, int n_ch, NchGroup<CPAD> &out)
{
    const float4 *q = cell + (size_t)group * (2 * CPAD);
#pragma unroll
    for (int p = 0; p < 2 * CPAD; ++p) out.q[p] = q[p];
#pragma unroll
    for (int ch = 0; ch < CPAD; ++ch) {
        const int c = CPAD * group + ch;
        out.g[ch] = nch_stream(g + (c < n_ch ? c : n_ch - 1));     // a padded channel re-reads the row's last one and is never used
    }
}

// the group's channels into the chains: FIRST: the chains start here (channel 0 is a product, not an fma onto zero)
template <int CPAD, bool FIRST>
MRL_HD void nch_contract_group(const NchGroup<CPAD> &s, int group, int n_ch, double t[8], double &base)
{
#pragma clang fp contract(off)
    float v[8 * CPAD];
#pragma unroll
    for (int p = 0; p < 2 * CPAD; ++p) { v[4 * p] = s.q[p].x; v[4 * p + 1] = s.q[p].y; v[4 * p + 2] = s.q[p].z; v[4 * p + 3] = s.q[p].w; }
#pragma unroll
    for (int ch = 0; ch < CPAD; ++ch) {
        if (CPAD * group + ch >= n_ch) continue;                   // wave-uniform
        const double g = (double)s.g[ch], b = (double)v[ch];
        if (FIRST && ch == 0) {
            base = g * b;
#pragma unroll
            for (int k = 1; k < 8; ++k) t[k] = g * ((double)v[k * CPAD] - b);
        } else {
            base = __builtin_fma(g, b, base);
#pragma unroll
            for (int k = 1; k < 8; ++k) t[k] = __builtin_fma(g, (double)v[k * CPAD + ch] - b, t[k]);
        }
    }
}

// grad_wi = sum_c g_c dE_c / d wi and grad_wo of ONE unit on the n-channel table m (kind TABLE_NCH, n_ch = m's channel count, bricks
// padded to CPAD channels: 1, 2, or groups of 4) under the options o; g: the unit's n_ch cotangents (4-byte aligned).  Dead units get
// +0.0f from a select at the very end, whatever g holds.
template <int CPAD>
MRL_HD TableDirGrad nch_eval_dir_grad(const MaterialDev &m, const Options &o, float wix, float wiy, float wiz, float wox, float woy, float woz,
                                      const float *g, int n_ch)
{
#pragma clang fp contract(off)
    const DirCell s = dir_cell(m, o, wix, wiy, wiz, wox, woy, woz);
    const int groups = CPAD == 4 ? (n_ch + 3) / 4 : 1;             // wave-uniform: n_ch is an argument of the call
    const float4 *cell = m.texels + (cell_index(s.cell, m.n_td, m.n_pd) * groups) * (2 * CPAD);
    NchGroup<CPAD> cur, next;
    nch_load_group<CPAD>(cell, g, 0, n_ch, cur);
    next = cur;
    if (groups > 1) nch_load_group<CPAD>(cell, g, 1, n_ch, next);
    double t[8], base = 0.0;
    t[0] = 0.0;
    nch_contract_group<CPAD, true>(cur, 0, n_ch, t, base);
    for (int group = 1; group < groups; ++group) {
        cur = next;
        if (group + 1 < groups) nch_load_group<CPAD>(cell, g, group + 1, n_ch, next);     // in flight while this group is contracted
        nch_contract_group<CPAD, false>(cur, group, n_ch, t, base);
    }
    const DirForms F = dir_forms(s, t, base);
    return dir_tail(m.param, o, s, F);
}

} // namespace fast
} // namespace mrl
