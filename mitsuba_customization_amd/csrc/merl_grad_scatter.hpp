// merl_grad_scatter.hpp — what the scatter kernels of the four adjoints of eval share (merl_table_grad.hip, merl_table_grad_nch.hip,
// merl_rgl_values_grad.hip, merl_rgl_spectral_values_grad.hip; DESIGN.md "What the adjoints share"): the small helpers, and the protocol by which a wave adds its units'
// records.  Device code only.  A kernel parks, per lane, the key of its unit's record (s_key, -1 for a dead unit) and the unit's
// factors in LDS, passes a barrier, and then the wave works through its units L lanes at a time: lane group `lane / L` carries one
// record per wave-instruction, slot `lane % L` of it, so that a record is one contiguous run of f64 atomic adds.  What a slot's term
// is and where a record lives come in as callables; the LDS arrays, the per-unit computation and the barriers stay in the kernels.
// The host side of the same calls is grad_scatter_call (merl_ctx.hpp, merl_grad_scatter.hip).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <type_traits>

namespace mrl {

constexpr int kMergeMin = 4;             // merge a wave's lanes by record when at least this many share the first live lane's record

// f64 add without a compare-and-swap loop (global_atomic_add_f64 / flat_atomic_add_f64); the destinations are device allocations
__device__ __forceinline__ void add_f64(double *p, double v) { (void)unsafeAtomicAdd(p, v); }

// the units of a launch over n slots; INDEXED: a queue of capacity n with a device-side length (every thread reads the same count)
template <bool INDEXED> __device__ __forceinline__ size_t grad_items(size_t n, const uint32_t *idx_count)
{
    if constexpr (INDEXED) { const size_t c = (size_t)*idx_count; return c < n ? c : n; }
    else return n;
}

// the brick slots that reach texel i of an axis of n texels: source s = 0: cell i, corner offset 0; 1: cell i - 1, offset 1;
// 2: the folded corner index n — cell n - 1, offset 1 — onto texel n - 1 (clamped axis) or texel 0 (periodic axis)
__device__ __forceinline__ bool fold_source(int s, int i, int n, bool periodic, int &cell, int &off)
{
    cell = s == 0 ? i : (s == 1 ? i - 1 : n - 1);
    off = s == 0 ? 0 : 1;
    return s == 0 ? true : (s == 1 ? i >= 1 : (periodic ? i == 0 : i == n - 1));
}

// Are the wave's lanes summed by record before they are added?  merge: 0 the wave-uniform choice (at least kMergeMin lanes hold the
// first live lane's key), 1 never, 2 always.  live: the ballot of key >= 0; s_key[wbase + lane] holds each lane's key.  Wave-uniform.
__device__ __forceinline__ bool wave_merge_rule(int merge, int key, const int *s_key, unsigned wbase, uint64_t live)
{
    if (merge != 0 || live == 0ull) return merge == 2;
    const int k0 = s_key[wbase + (unsigned)__builtin_ctzll(live)];
    return __popcll(__ballot(key == k0)) >= kMergeMin;
}

__device__ __forceinline__ unsigned lowest_bit(uint32_t v) { return (unsigned)__builtin_ctz(v); }
__device__ __forceinline__ unsigned lowest_bit(uint64_t v) { return (unsigned)__builtin_ctzll(v); }

// The wave adds its live units' records, L lanes per record and so 64 / L units per wave-instruction.  Not merged: unit after unit.
// Merged, the leader loop: the lanes that hold the first remaining lane's key are summed by the slot lanes of each group of L lanes
// (a group sums its members among its own lanes, in ascending lane order), one atomic per slot and group.
//   active(ref)       does this lane's slot exist in the record of unit `ref`?
//   term(m, ref)      unit m's term for this lane's slot
//   accum(acc, m, ref)  acc and unit m's term, accumulated the kernel's own way (its merged sums keep their bits)
//   dest(ref)         this lane's slot of the record of unit `ref`
// m and ref index the block's LDS arrays; ref is m itself (not merged) or the first lane of m's key (merged: the same record).
template <unsigned L, class Active, class Term, class Accum, class Dest>
__device__ __forceinline__ void wave_scatter(uint64_t live, bool merged, int key, const int *s_key, unsigned wbase, unsigned lane,
                                             Active active, Term term, Accum accum, Dest dest)
{
    constexpr unsigned U = 64u / L;
    using Members = std::conditional_t<(L <= 32u), uint32_t, uint64_t>;      // of one lane group
    const unsigned sub = lane / L;
    if (live == 0ull) return;                                    // wave-uniform, like everything decided from live and merged
    if (!merged) {
        for (unsigned j = 0; j < 64u; j += U) {
            if (((live >> j) & ((1ull << U) - 1ull)) == 0ull) continue;
            const unsigned m = wbase + j + sub;
            if (s_key[m] >= 0 && active(m)) add_f64(dest(m), term(m, m));
        }
        return;
    }
    uint64_t rem = live;
    while (rem != 0ull) {
        const unsigned first = wbase + (unsigned)__builtin_ctzll(rem);
        const uint64_t members = __ballot(key == s_key[first]);
        rem &= ~members;
        Members mm = (Members)members;
        if constexpr (L < 64u) mm = (Members)(members >> (sub * L)) & (Members)((1ull << L) - 1ull);
        if (active(first) && mm != 0) {
            double acc = 0.0;
            while (mm != 0) {
                const unsigned m = wbase + sub * L + lowest_bit(mm);
                mm &= mm - 1;
                acc = accum(acc, m, first);
            }
            add_f64(dest(first), acc);
        }
    }
}

} // namespace mrl
