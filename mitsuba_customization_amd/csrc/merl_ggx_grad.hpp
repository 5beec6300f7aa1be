// merl_ggx_grad.hpp — what the two parameter-gradient translation units share (merl_ggx_grad.hip: one material over whole arrays;
// merl_ggx_grad_mat.hip: a material id per unit, queues, several targets): the layout of a row of partial sums, the order of the
// normal matrix's terms in it, and the wave sum.  Each file keeps its kernels, its grid and its workspace.
#pragma once
#include <hip/hip_runtime.h>

namespace mrl {

constexpr int kParams = 7;               // alpha, eta_r, eta_g, eta_b, k_r, k_g, k_b
constexpr int kNormalTerms = 16;         // the unique non-zero entries of the normal matrix, in normal_entry's order
constexpr int kRow = 32;                 // doubles per workspace row (256 B): kParams (+ kNormalTerms) used

// term j of the normal matrix -> its entry (a, b), a <= b:  0: alpha.alpha;  then per channel c, three at a time:
// alpha.eta_c, alpha.k_c, eta_c.eta_c, eta_c.k_c, k_c.k_c.  Entries that couple two channels are structurally zero.
__host__ __device__ inline void normal_entry(int j, int &a, int &b)
{
    if (j == 0) { a = 0; b = 0; return; }
    const int q = (j - 1) / 3, c = (j - 1) % 3;
    a = q < 2 ? 0 : (q < 4 ? 1 + c : 4 + c);
    b = (q == 0 || q == 2) ? 1 + c : 4 + c;
}

// the sum over the wave in every lane, in an order that depends on nothing (xor butterfly; an f64 moves as two dwords)
__device__ __forceinline__ double wave_sum(double v)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

} // namespace mrl
