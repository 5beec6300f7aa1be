// merl_dir_grad.hpp — what the direction-gradient kernels share (merl_ggx_dir_grad.hip, merl_table_dir_grad.hip, merl_nch_dir_grad.hip;
// DESIGN.md §5i - §5k): the arrays beside BatchArgs and the grid-stride loop with its masked stores.  The material record a unit's
// id names is lane_material of merl_unit.hpp; a.mat, a.idx -> PER_LANE, INDEXED at a launch is with_flags of merl_kernels.hpp.  The
// host call that ends in these launches is grad_dir_call of merl_calls.hip.  Each family keeps its __global__ kernel, its launch
// bounds and its per-lane function.
#pragma once
#include "merl_unit.hpp"

namespace mrl {

struct DirGradOut { const float *g; float *grad_wi, *grad_wo; };     // g: [n][3], or [n][n_ch] for the n-channel kernels

// The body of a direction-gradient kernel of BLOCK threads: a grid-stride loop over the units (INDEXED: over a.idx), one lane = one
// unit.  unit(i, out_wi, out_wo) fills the two gradients of unit i and says whether its material is one the family evaluates; the
// gradients of a unit whose material is not are stored as zeros.  A null output is neither computed into memory nor written.
template <int BLOCK, bool INDEXED, class Unit>
__device__ __forceinline__ void dir_grad_loop(const BatchArgs &a, const DirGradOut &o, Unit &&unit)
{
#pragma clang fp contract(off)
    const size_t stride = (size_t)gridDim.x * BLOCK;
    const size_t n_items = item_count<INDEXED>(a);
    for (size_t j = (size_t)blockIdx.x * BLOCK + threadIdx.x; j < n_items; j += stride) {
        const size_t i = INDEXED ? (size_t)a.idx[j] : j;
        float r_wi[3], r_wo[3];
        const bool known = unit(i, r_wi, r_wo);
        if (o.grad_wi) {
            const float v[3] = { known ? r_wi[0] : 0.0f, known ? r_wi[1] : 0.0f, known ? r_wi[2] : 0.0f };
            store3s<true>(o.grad_wi, i, v);
        }
        if (o.grad_wo) {
            const float v[3] = { known ? r_wo[0] : 0.0f, known ? r_wo[1] : 0.0f, known ? r_wo[2] : 0.0f };
            store3s<true>(o.grad_wo, i, v);
        }
    }
}

} // namespace mrl
