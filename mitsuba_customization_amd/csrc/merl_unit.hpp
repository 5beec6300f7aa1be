// merl_unit.hpp — the per-unit steps more than one kernel takes (k_batch, k_table, k_table_dma of merl_kernels.hip; k_table_nch,
// k_table_nch_wide of merl_nch.hip; the direction-gradient kernels; DESIGN.md §5, "What the forward kernels share"): which material a
// unit has and whether this call may evaluate it, and the pdf of a given wo.  Each kernel keeps its loop, its loads and stores, its
// LDS and its waits.  A predicate that differs between kernels (what gates the table's pdf) is an argument, never decided here.
#pragma once
#include "merl_kernels.hpp"
#include "merl_table_fast.hpp"

namespace mrl {

// the record a material id names; an id out of range: record 0 and in_range = false, so that the caller's loads stay branch-free
struct LaneMaterial { const MaterialDev &m; bool in_range; };
__device__ __forceinline__ LaneMaterial id_material(const BatchArgs &a, int id)
{
    const bool in_range = id >= 0 && id < a.n_materials;
    return { a.materials[in_range ? id : 0], in_range };
}
__device__ __forceinline__ LaneMaterial lane_material(const BatchArgs &a, size_t i) { return id_material(a, a.mat[i]); }

// RGB path: the material of a unit with id `id` (MULTI; else a.single) into m.  False: the id names nothing this call can evaluate
// (out of range, released, another kind) — m is then a.safe, and the caller zeroes wi.z.  MODE_PDF also admits n-channel tables.
template <int MODE, bool MULTI>
__device__ __forceinline__ bool rgb_material(const BatchArgs &a, int id, MaterialDev &m)
{
    if constexpr (MULTI) {
        const LaneMaterial l = id_material(a, id);
        m = l.m;
        const bool known = l.in_range && (kind_is_rgb_path(m.kind) || (MODE == MODE_PDF && m.kind == KIND_TABLE_NCH));
        if (!known) m = a.safe;
        return known;
    } else {
        m = a.single;
        return true;
    }
}

// n-channel path: the record of unit i into m; true: an n-channel table of the width the call was made for.  False: m is not used
// for a lookup — the caller reads a harmless source (the material array itself) at dims 1 x 1 x 1 and zeroes wi.z.
template <bool MULTI>
__device__ __forceinline__ bool nch_material(const BatchArgs &a, size_t i, int n_ch, MaterialDev &m)
{
    if constexpr (MULTI) {
        const LaneMaterial l = lane_material(a, i);
        m = l.m;
        return l.in_range && m.kind == KIND_TABLE_NCH && m.n_ch == n_ch;
    } else {
        m = a.single;
        return true;
    }
}

// the pdf of a given wo: `lambert`, or the table's when the option asks for it and `gate` holds.  The gate is the caller's: k_table
// gates on lambert > 0, k_table_dma and the n-channel kernels on wi.z > 0 && wo.z > 0 (&& known) — for a denormal wo.z these differ.
__device__ __forceinline__ float lambert_pdf(bool valid, float woz) { return valid ? woz * kInvPiF : 0.0f; }
__device__ __forceinline__ float wo_pdf(const MaterialDev &m, int sampling, bool gate, float lambert, const fast::Vec3 &in, float wox, float woy, float woz)
{
    float pdf = lambert;
    if (sampling && gate) pdf = (float)fast::table_pdf(m, in, fast::normalize_f32(wox, woy, woz), woz, sampling);
    return pdf;
}

} // namespace mrl
