// merl_kernels.hpp — launch interface between the C-ABI layer and the gfx950 kernels.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include <string>
#include <type_traits>
#include <vector>

#include "merl_device.hpp"
#include "merl_image_file.hpp"       // RglFields / RglLayout, rgl_plan_layout, nch_brick_float4s: shapes -> sizes, pure host

namespace mrl {

// What a unit computes: eval(wi, wo) -> rgb, pdf(wi, wo), sample(wi, u) -> (wo', pdf', weight'), or one of two fusions.  Kernels
// take the mode as an `int MODE` template parameter (their mangled names carry the number, and the ISA tests and profiles match on them).
enum Mode : int { MODE_EVAL = 0, MODE_PDF = 1, MODE_SAMPLE = 2, MODE_EVAL_SAMPLE = 3, MODE_EVAL_PDF = 4 };
constexpr bool mode_eval(int m) { return m == MODE_EVAL || m == MODE_EVAL_SAMPLE || m == MODE_EVAL_PDF; }
constexpr bool mode_pdf(int m) { return m == MODE_PDF || m == MODE_EVAL_SAMPLE || m == MODE_EVAL_PDF; }
constexpr bool mode_sample(int m) { return m == MODE_SAMPLE || m == MODE_EVAL_SAMPLE; }

// runtime mode -> f(std::integral_constant<int, MODE>{}); hipErrorInvalidValue for a value that names no mode
template <class F>
hipError_t with_mode(int mode, F &&f)
{
    switch (mode) {
        case MODE_EVAL:        return f(std::integral_constant<int, MODE_EVAL>{});
        case MODE_PDF:         return f(std::integral_constant<int, MODE_PDF>{});
        case MODE_SAMPLE:      return f(std::integral_constant<int, MODE_SAMPLE>{});
        case MODE_EVAL_SAMPLE: return f(std::integral_constant<int, MODE_EVAL_SAMPLE>{});
        case MODE_EVAL_PDF:    return f(std::integral_constant<int, MODE_EVAL_PDF>{});
    }
    return hipErrorInvalidValue;
}

// runtime flags -> f(std::bool_constant<flag>{}...), the way with_mode turns a mode into a template argument: every launcher
// names its kernel once, with `decltype(flag)::value` (or the constant itself) as the template arguments
template <class F> auto with_flags(F &&f) { return f(); }
template <class F, class... Rest>
auto with_flags(F &&f, bool flag, Rest... rest)
{
    auto bind = [&](auto c) { return with_flags([&](auto... cs) { return f(c, cs...); }, rest...); };
    return flag ? bind(std::true_type{}) : bind(std::false_type{});
}

// blocks of a grid-stride launch over n units at `threads` per block: at most cap, at least 1; whole_xcds: rounded up to whole
// rounds over the 8 XCDs (workgroups are dealt to them round-robin; BatchArgs::block_map relies on it)
inline unsigned grid_blocks(size_t n, size_t threads, size_t cap, bool whole_xcds = false)
{
    size_t blocks = (n + threads - 1) / threads;
    if (blocks > cap) blocks = cap;
    if (blocks < 1) blocks = 1;
    if (whole_xcds) blocks = (blocks + 7) / 8 * 8;
    return (unsigned)blocks;
}

// Kernel arguments of one batched call; pointers are device-accessible.
struct BatchArgs {
    const float *wi, *wo, *u;
    const int32_t *mat;              // nullptr: single
    size_t n;
    float *out_rgb, *out_pdf, *out_wo, *out_pdf2, *out_weight;
    MaterialDev single;              // by value -> SGPRs (single-material launches)
    const MaterialDev *materials;    // device array (mixed-material launches)
    int n_materials;
    // what a unit evaluates when its material id names nothing this call can evaluate (out of range, released,
    // another kind such as an n-channel table): a 1 x 1 x 1 table of zeros in valid device memory.  Its outputs are
    // forced to zero anyway, but its lookups run (the code is branch-free) and must touch memory that exists — an
    // n-channel table's cells are narrower than the 128-B bricks these kernels read.
    MaterialDev safe;
    int any_standard;                // some table this launch may meet is in a standard parameterisation (MaterialDev::param != 0)
    int block_map;                   // k_table_dma: 0 interleaved grid-stride tiles, 1 one contiguous eighth of the batch per XCD
    Options opts;
    // queue launches (idx != nullptr): the units idx[0 .. min(*idx_count, n)) — a caller's wavefront queue (n: its capacity) or one
    // kind's queue built by k_partition_kinds (n: the units of the whole batch); n sizes the grid and clamps the device-side count
    const uint32_t *idx;
    const uint32_t *idx_count;               // its length, in device memory
};

// ---- stream access of the batch kernels ----
__device__ __forceinline__ void load3(const float *p, size_t i, float &x, float &y, float &z)
{
    const float *q = p + 3 * i;
    x = q[0]; y = q[1]; z = q[2];
}
__device__ __forceinline__ void store3(float *p, size_t i, const float v[3])
{
    float *q = p + 3 * i;
    q[0] = v[0]; q[1] = v[1]; q[2] = v[2];
}
// streaming (read-once / write-once) accesses: the nt hint keeps them from displacing table
// lines in the XCD's L2
template <bool NT> __device__ __forceinline__ float ldf(const float *p) { if constexpr (NT) return __builtin_nontemporal_load(p); else return *p; }
template <bool NT> __device__ __forceinline__ void stf(float *p, float v) { if constexpr (NT) __builtin_nontemporal_store(v, p); else *p = v; }
template <bool NT> __device__ __forceinline__ void load3s(const float *p, size_t i, float &x, float &y, float &z)
{
    const float *q = p + 3 * i;
    x = ldf<NT>(q); y = ldf<NT>(q + 1); z = ldf<NT>(q + 2);
}
template <bool NT> __device__ __forceinline__ void store3s(float *p, size_t i, const float v[3])
{
    float *q = p + 3 * i;
    stf<NT>(q, v[0]); stf<NT>(q + 1, v[1]); stf<NT>(q + 2, v[2]);
}

// number of work items of a launch: a.n, or for a queue launch the device-side count clamped to the capacity a.n
template <bool INDEXED> __device__ __forceinline__ size_t item_count(const BatchArgs &a)
{
    if constexpr (INDEXED) { const size_t c = (size_t)*a.idx_count; return c < a.n ? c : a.n; }
    else return a.n;
}

// ---- table re-layout: what the brick builders share (k_build_bricks, k_rows_to_bricks, k_build_bricks_nch) ----
// source texel of corner k = 4 a + 2 b + c of cell (ih, id, ip) in a planar [n_th][n_td][n_pd] table: theta_h and theta_d clamp at
// the last node, phi_d clamps or wraps
__device__ __forceinline__ size_t brick_corner(int ih, int id, int ip, int k, int n_th, int n_td, int n_pd, int phi_periodic)
{
    const int sh = min(ih + (k >> 2), n_th - 1), sd = min(id + ((k >> 1) & 1), n_td - 1), sp = phi_periodic ? (ip + (k & 1)) % n_pd : min(ip + (k & 1), n_pd - 1);
    return ((size_t)sh * n_td + sd) * n_pd + sp;
}
// an RGB brick: 8 corners x 3 channels packed, 8 floats of zero padding -> 128 B
__device__ __forceinline__ void store_rgb_brick(float4 *dst, float v[32])
{
#pragma unroll
    for (int pad = 24; pad < 32; ++pad) v[pad] = 0.0f;
#pragma unroll
    for (int q = 0; q < 8; ++q) dst[q] = make_float4(v[4 * q], v[4 * q + 1], v[4 * q + 2], v[4 * q + 3]);
}

// ---- which kernel serves a batch launch ----
// What the choice depends on beyond BatchArgs (a.mat: a material id per unit, a.idx: the launch walks a queue).
struct BatchRoute {
    int variant;                     // MRL_OPT_KERNEL: 0 generic, 1 tuned table path, 2 + non-temporal streams, 3 + LDS-DMA brick fetch, 4 + kind partition
    int layout;                      // the context-wide table layout (every table of a context has the same one)
    bool has_ggx, has_table;         // what a batch with material ids may contain: analytic (GGX) / table materials
    bool whole_xcds;                 // k_table_dma's grid is rounded up to whole rounds over the 8 XCDs
};
// One kernel instantiation and its grid: grid_blocks(a.n, block, compute units * blocks_per_cu, whole_xcds) blocks of `block` threads.
enum KernelFamily : int { KERNEL_BATCH = 0, KERNEL_TABLE = 1, KERNEL_TABLE_DMA = 2, KERNEL_GGX = 3 };
struct KernelChoice {
    int family, mode;
    bool multi;                      // MULTI (k_ggx: PER_LANE): the material comes from a.mat
    bool indexed;                    // INDEXED (k_table has no queue form)
    bool nt;                         // k_table: NT
    int lookup, layout;              // k_table: LOOKUP, LAYOUT
    bool ggx, standard;              // k_table_dma: GGX, STD
    int block, blocks_per_cu;
    bool whole_xcds;
};
// Pure arithmetic, no HIP call.  The first rule that matches, with V = r.variant for whole arrays and 3 for a queue (queues ignore
// MRL_OPT_KERNEL), multi = a.mat != nullptr, indexed = a.idx != nullptr:
//   1. V >= 1, a single GGX material                              k_ggx<M, true, false, indexed>       tuned analytic kernel
//   2. V >= 1, multi, has_ggx, no table                           k_ggx<M, true, true, indexed>        ... over several analytic materials
//   3. M != PDF, V >= 3, brick layout, trilinear lookup           k_table_dma<M, multi, true, multi && has_ggx, indexed, STD>
//        STD: a.any_standard or the renormalising blend; its LDS lets a CU hold 2 (fused mode) or 4 blocks
//   4. whole arrays, V >= 1, not the renormalising blend          k_table<M, multi, V >= 2, lookup, layout>   (blends the texels as stored)
//   5. otherwise                                                  k_batch<M, multi, indexed>           generic: every kind, ocml f64 math
KernelChoice route_batch(int mode, const BatchArgs &a, const BatchRoute &r);
// the kernel's name as the code object spells it (demangled, without namespaces and arguments): "k_table_dma<3, false, true, false, false, false>"
std::string kernel_name(const KernelChoice &k);
// MRL_OPT_KERNEL >= 4: a whole-array batch that may mix table and analytic materials is split into one dense queue per kind
// (launch_partition_kinds), and each queue runs as a queue launch of kind_queue_route: k_table_dma without the GGX code (the one
// DMA grid that is not rounded to whole XCD rounds: block_map applies there only when the capped grid is a multiple of 8), k_ggx.
inline bool route_partitions(int mode, const BatchArgs &a, const BatchRoute &r)
{
    return !a.idx && a.mat && r.has_ggx && r.has_table && r.variant >= 4 && mode != MODE_PDF && r.layout == LAYOUT_BRICK && a.opts.lookup == 1 &&
           a.n < ((size_t)1 << 32);
}
inline BatchRoute kind_queue_route(const BatchRoute &r, bool ggx_queue) { return { r.variant, r.layout, ggx_queue, !ggx_queue, false }; }
// launches the kernel route_batch names
hipError_t launch_batch(int mode, const BatchArgs &a, const BatchRoute &r, int compute_units, hipStream_t stream);
// kind-partitioned mixed batches: build the two queues (a.idx / a.idx_count of the two queue launches; a.n stays the whole batch)
void partition_geometry(size_t n, int compute_units, uint32_t *segments, uint32_t *seg_len);
// work: 4*segments + 2 uint32 (counts, offsets, totals[2] at work + 4*segments)
hipError_t launch_partition_kinds(const int32_t *mat, size_t n, const MaterialDev *materials, int n_materials,
                                  uint32_t *queue_table, uint32_t *queue_ggx, uint32_t *work,
                                  uint32_t segments, uint32_t seg_len, hipStream_t stream);
// per-material compaction for wavefront callers (mrl_partition_by_material): stable partition of [0, n) by material id
constexpr int kMaxPartitionMaterials = 2048;
void material_partition_geometry(size_t n, int compute_units, uint32_t *chunks, uint32_t *chunk_len);
// work: chunks*K + K uint32; queue: n uint32; offsets: K + 1; counts: K (all device)
hipError_t launch_partition_materials(const int32_t *mat, size_t n, int K, uint32_t *queue, uint32_t *offsets, uint32_t *counts,
                                      uint32_t *work, uint32_t chunks, uint32_t chunk_len, int compute_units, hipStream_t stream);
// a1: planar f64 table (device copy of the file payload) -> padded rows or bricks; clamp: negative values become 0 (MRL_OPT_NEGATIVE = 0)
hipError_t launch_build_table(const double *d_planar, const int dims[3], const double scale[3], int layout, int param, int clamp, float4 *d_out,
                              int compute_units, hipStream_t stream);
// one RGB table layout to the other (the on-disk image cache stores the rows form): padded rows <-> bricks, same Float values
hipError_t launch_rows_to_bricks(const float4 *d_rows, const int dims[3], float4 *d_bricks, int compute_units, hipStream_t stream);
hipError_t launch_bricks_to_rows(const float4 *d_bricks, const int dims[3], int param, float4 *d_rows, int compute_units, hipStream_t stream);
// the conditional sampling table P(theta_h | theta_i) of a resident RGB table (MRL_OPT_SAMPLING = 2): a quadrature kernel
// and a prefix-scan kernel; d_rows: n_ti x (2 n_th + 1) doubles, d_work: n_ti x n_th doubles
constexpr int kSamplingIncidentBins = 32;
hipError_t launch_build_sampling2d(const MaterialDev &m, const Options &opts, int n_ti, double *d_rows, double *d_work, hipStream_t stream);
// ---- n-channel tables (merl_nch.hip): a.out_rgb / a.out_weight hold n x n_ch values ----
constexpr int kMaxChannels = 32;
// nch_brick_float4s(n_ch): float4s per cell: 2 (1 ch), 4 (2 ch), 8 * ceil(n_ch / 4)  (merl_image_file.hpp)
// mode: any but MODE_PDF (pdf alone: the RGB pdf kernel serves every table kind)
hipError_t launch_batch_nch(int mode, const BatchArgs &a, int n_ch, int compute_units, hipStream_t stream);
hipError_t launch_build_table_nch(const double *d_planar, const double *d_scale, const int dims[3], int n_ch, int param, int clamp, float4 *d_out,
                                  int compute_units, hipStream_t stream);
// ---- the adaptive-parameterisation measured BSDF (merl_rgl.hip; RGL *.bsdf) ----
struct RglDev;
int rgl_reduction(const RglFields &f);                                   // 1, 2, 4: the part of the azimuth an anisotropic file stores
const char *rgl_check_fields(const RglFields &f);                        // nullptr, or what is wrong
RglLayout rgl_build_image(const RglFields &f, std::vector<float> &blob); // normalised tables + running integrals, host f64
RglDev rgl_descriptor(const RglFields &f, const RglLayout &l, const float *base);
// r != nullptr: a single-material launch; r == nullptr: a batch with material ids (a.mat) — the units whose id names an RGL material
// are evaluated and written, every other unit is left as it is.  a.idx != nullptr: walk the queue a.idx / a.idx_count.
// search (MRL_OPT_RGL_SEARCH): 0 = a single-material launch reads the distributions' search tables from a copy in LDS when they fit
// a CU's LDS, 1 = always from memory (the results are the same bits)
hipError_t launch_rgl(int mode, const BatchArgs &a, const RglDev *r, int search, int compute_units, hipStream_t stream);
// a spectral RGL material: a.out_rgb / a.out_weight hold n x W values at the per-unit wavelengths wl [n][W] (nullptr: the file's own
// wavelength nodes, W = their number) — whole arrays, over a queue (a.idx != nullptr: a.idx / a.idx_count, a.n = the capacity) and / or
// with a material id per unit (r == nullptr: a.mat, a.materials; a unit whose id names no live spectral RGL material gets zeros in
// every output of the mode); any mode but MODE_PDF
hipError_t launch_rgl_spectral_q(int mode, const BatchArgs &a, const RglDev *r, const float *wl, int W, int search, int compute_units,
                                 hipStream_t stream);
// Which kernels serve those two entries, the way route_batch does it for the RGB tables: pure arithmetic, no HIP call (lds_limit: the
// device's LDS per workgroup, an input).  Exported as mrl_rgl_route; tests/test_rgl_route_cpu.py restates the rules.
enum RglFamily : int { KERNEL_RGL = 0, KERNEL_RGL_LDS = 1, KERNEL_RGL_SPECTRAL = 2, KERNEL_RGL_SPECTRAL_Q = 3 };
// where a single-material kernel reads the distributions' running integrals: the cell records in memory, a copy in LDS, or the
// marginal rows from LDS and the rest from memory
enum RglTables : int { RGL_TABLES_MEM = 0, RGL_TABLES_LDS = 1, RGL_TABLES_LDS_MARG = 2 };
struct RglShape { int n_phi, n_theta, nx, ny, n_wl; };      // of the launch's one file (material ids: unused)
struct RglChoice {
    int family, mode;
    bool indexed;                    // INDEXED (k_rgl_spectral has no queue form: k_rgl_spectral_q serves its queues)
    bool multi;                      // k_rgl, k_rgl_spectral_q: MULTI, the material comes from a.mat
    int tables;                      // k_rgl_lds: MARG_ONLY = RGL_TABLES_LDS_MARG; k_rgl_spectral, k_rgl_spectral_q: LDS = RGL_TABLES_LDS
    int mask;                        // MASK: 5 isotropic (n_phi == 1, n_theta > 1), 15 anisotropic (both > 1), 0 the shape is tested at run time
    int block, blocks_per_cu;        // grid_blocks(n, block, compute units * blocks_per_cu): 1 for the kernels that copy tables into LDS, else 8
    size_t lds_bytes;                // dynamic LDS: the parameter grids, and the tables by `tables`
};
struct RglRoute { int count; RglChoice launch[2]; };
// multi: one launch of the memory kernel, mask 0.  One file, with copy = search == 0 && n >= 2^15 and fits = its integrals <= lds_limit:
//   copy && fits                                        the LDS kernel, mask 5 or 0
//   copy && !fits, RGB, MODE_EVAL_SAMPLE                two launches: MODE_EVAL_PDF then MODE_SAMPLE, each by these rules
//   copy && !fits, RGB, MODE_SAMPLE, marginal rows fit  k_rgl_lds<2, ., true, 15 or 0>
//   otherwise                                           the memory kernel, mask 5 / 15 / 0 (spectral: 5 / 0)
// count 0: a value that names no mode, or MODE_PDF on a spectral file.
RglRoute route_rgl(int mode, bool spectral, bool multi, bool indexed, int search, size_t n, const RglShape &s, size_t lds_limit);
std::string kernel_name(const RglChoice &k);
// ---- one-unit calls (merl_scalar.hip): a bounded-lifetime service kernel answers requests posted in pinned host memory ----
struct ScalarBoard;
struct ScalarArgs {
    const MaterialDev *materials;    // the context's material array (the host stops the service before it changes)
    int n_materials;
    MaterialDev safe;
    Options opts;
    ScalarBoard *board;              // pinned, coherent host memory (device-visible address)
    uint32_t gen;                    // this instance's generation: written to board->started_gen / exited_gen
    uint32_t max_polls;              // hard bound on the poll loop, whatever the clock says
    uint64_t lifetime_ticks;         // of wall_clock64() (100 MHz)
};
hipError_t launch_scalar_service(const ScalarArgs &a, hipStream_t stream);
hipError_t launch_generate_pairs(uint64_t seed, uint64_t first, size_t n, float *wi, float *wo, float *u,
                                 int compute_units, hipStream_t stream);
hipError_t launch_generate_materials(uint64_t seed, uint64_t first, size_t n, int n_materials, int32_t *mat,
                                     int compute_units, hipStream_t stream);

} // namespace mrl
