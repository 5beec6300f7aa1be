// merl_ctx.hpp — what the translation units behind the C ABI (include/merl_hip.h) share: the context, its material records, the
// error / lock macros and the internal functions one file defines and another calls.  Not installed; nothing here is part of the ABI.
//   merl_abi.hip           contexts, options, streams, memory helpers, one-unit call service, errors
//   merl_materials.hip     material constructors (MERL / customized_measurement / n-channel / GGX / RGL), release, host images
//   merl_calls.hip         batch, queue and n-channel calls: a call's arrays as a stream list, the two host-array movers, launches;
//                          grad_dir_call, the host side of every direction-gradient call
//   merl_host_stage.hpp    host-array path, host C++ only: stream list, slot layout, the chunk loop, the copy threads
//   merl_image_cache.hip   on-disk cache of a material's device image
//   merl_rgl_spectral.hip  spectral RGL materials: constructor + calls
//   merl_table_grad.hip    the adjoint of eval on RGB tables (mrl_table_grad_batch; with material ids and queues, onto several
//                          tables: mrl_table_grad_batch_mat / mrl_table_grad_queue of merl_hip_fit_table.h): scatter kernels + calls
//   merl_table_grad_nch.hip  the same adjoint on n-channel tables (mrl_table_grad_batch_nch / mrl_table_grad_queue_nch of
//                          merl_hip_fit_nch.h): scatter kernels per (cell, channel group of 4) + calls
//   merl_grad_scatter.hpp  what the scatter kernels of the four adjoints share (the two above, merl_rgl_values_grad.hip and
//                          merl_rgl_spectral_values_grad.hip): the wave's merge rule and its record-by-record scatter, fold_source, the f64 add.  Device code only
//   merl_grad_scatter.hip  grad_scatter_call, the host side of every adjoint call, and the kernel that clears their workspace
//   merl_update.hip        new values for a resident material in place (include/merl_hip_update.h): table images through the upload's
//                          build kernels, the row marginal on the device (reduction + finishing kernel), GGX parameters
//   merl_ggx_grad.hip      the parameter gradient of eval on a GGX conductor (mrl_ggx_grad_batch): reduction kernels + call
//   merl_ggx_grad_mat.hip  the same with a material id per unit and over queues, onto several GGX materials in one launch
//                          (mrl_ggx_grad_batch_mat / mrl_ggx_grad_queue of merl_hip_fit_ggx.h): segmented reduction kernels + calls
//   merl_dir_grad.hpp      what the direction-gradient kernels share: the grid-stride loop with its masked stores, the record a
//                          material id names, the PER_LANE / INDEXED dispatch; their one host call is grad_dir_call of merl_calls.hip
//   merl_ggx_dir_grad.hip  the direction gradient of eval on GGX conductors (mrl_ggx_grad_dir_batch / _queue): streaming kernel + calls
//   merl_ggx_sample_grad.hip  the gradients of pdf and sample on GGX conductors (mrl_ggx_pdf_grad_* / mrl_ggx_sample_grad_*): kernels + calls
//   merl_table_dir_grad.hip  the same on RGB tables (mrl_table_grad_dir_batch / _queue)
//   merl_nch_dir_grad.hip  the same on n-channel tables (mrl_table_grad_dir_batch_nch / _queue_nch)
//   merl_rgl_dir_grad.hip  the same on RGB RGL materials (mrl_rgl_grad_dir_batch / _queue)
//   merl_rgl_values_grad.hip  the adjoint of eval in the measured values of RGB RGL materials and their update in place
//                          (include/merl_hip_fit_rgl.h): scatter, fold and write kernels + calls
//   merl_rgl_spectral_values_grad.hip  the same adjoint in the spectra of spectral RGL materials and their update in place
//                          (include/merl_hip_fit_rgl_spectral.h): scatter, fold and write kernels + calls
#pragma once
#include "../../include/merl_hip.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <condition_variable>
#include <functional>
#include <mutex>
#include <thread>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <vector>
#include <unistd.h>

#include "merl_kernels.hpp"
#include "merl_rgl.hpp"
#include "merl_image_file.hpp"
#include "merl_scalar_host.hpp"
#include "merl_host_table.hpp"
#include "merl_host_stage.hpp"

namespace mrlabi {


inline constexpr int kMerlDims[3] = { 90, 90, 180 };
inline constexpr double kMerlScale[3] = { 1.0 / 1500.0, 1.15 / 1500.0, 1.66 / 1500.0 };

// a device buffer that only grows
struct DeviceBuf {
    void *p = nullptr;
    size_t bytes = 0;
    // at least `need` bytes: as it is, or (after the context's stream has drained) freed and allocated anew; contents are not kept
    int reserve(mrl_ctx *ctx, size_t need);
};

struct MaterialHost {
    mrl::MaterialDev dev;
    float4 *d_texels = nullptr;
    bool in_arena = false;           // d_texels is a slice of the context's table arena (MRL_OPT_TABLE_ARENA_MB): not freed on its own
    double *d_sampling = nullptr;
    double *d_sampling2d = nullptr;  // P(theta_h | theta_i) rows (RGB tables), built on the device at upload
    size_t bytes = 0;                // device bytes this material holds (table + sampling marginal)
    mrl::RglDev rgl{};               // KIND_RGL: the five functions' descriptor (pointers into d_texels)
    bool released = false;           // tombstone left by mrl_material_release; the slot may be reused
    int rows_lookup = 1, rows_node = 0;      // the lookup / node options the conditional sampling rows were integrated under (at upload)
    // RGB tables uploaded as planar arrays: the channel scales the image was built with (the image itself is pre-scaled).
    // mrl_table_grad_batch needs them; a table restored from an image file does not carry them (has_scale stays false)
    double scale[3] = { 1.0, 1.0, 1.0 };
    bool has_scale = false;
    // n-channel tables uploaded as planar arrays: their n_ch channel scales (all ones when the caller passed none), which the
    // n-channel table adjoint needs (merl_table_grad_nch.hip); empty for every other material and for one restored from an image file
    std::vector<double> nch_scale;
    // what mrl_material_update_table needs beside the image (merl_update.hip): sized by the material's first update, never moved
    // afterwards (a captured update points at it), freed with the material; workspace bytes, not material bytes
    DeviceBuf update_ws;
};

} // namespace mrlabi
using mrlabi::MaterialHost;
using mrlabi::DeviceBuf;


// the pipelined mover's state (merl_calls.hip): two pinned, device-mapped slots (slot_layout), an event per slot, the copy threads
struct HostPipe {
    char *pin[2] = { nullptr, nullptr };
    size_t slot_bytes = 0;
    hipEvent_t done[2] = { nullptr, nullptr };
    mrlabi::CopyPool pool;
    int threads = -1;                                // workers the pool was started with
};

// the device side of the one-unit call service (merl_scalar_host.hpp): where the mailbox lives and how an instance of
// the service kernel is put on its own stream
struct ScalarDevice {
    mrl_ctx *ctx = nullptr;
    mrl::ScalarBoard *b = nullptr;           // pinned, coherent host memory; nullptr until the first scalar call
    mrl::ScalarBoard *b_dev = nullptr;       // the same memory as the device addresses it
    hipStream_t stream = nullptr;            // non-blocking: batch launches on the context's stream never queue behind an instance
    uint64_t lifetime_ticks = 50000;         // 500 us of the 100 MHz wall clock
    std::atomic<bool> ok{ true };
    mrl::ScalarBoard *board() { return b; }
    bool launch(uint32_t gen);
    bool healthy() { return ok.load(std::memory_order_relaxed); }
};
using ScalarSvc = mrl::ScalarService<ScalarDevice>;

struct mrl_ctx {
    // every entry point that touches the context takes this lock: calls from several host threads are safe and serialise
    // (device-pointer calls only enqueue, so the lock is held for microseconds; host-array calls hold it for their duration)
    mutable std::recursive_mutex mu;
    int device = 0;
    int compute_units = 256;
    std::string device_name;
    size_t total_mem = 0;
    hipStream_t own_stream = nullptr;
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    // the grow-only workspaces (freed by mrl_destroy, summed by mrl_memory_info):
    //   BUF_STAGE        one slot of a staged host-array call (slot_layout)
    //   BUF_QUEUES       kind-partitioned mixed batches: [2][n] unit indices + partition work area behind them
    //   BUF_PART_WORK    mrl_partition_by_material: per-chunk count table + totals
    //   BUF_GRAD_BRICKS  the table-gradient calls: gradient bricks, one 256-B record per cell of every table of a call (merl_table_grad.hip),
    //                    per cell and channel group of 4 for n-channel tables (merl_table_grad_nch.hip), one 128 / 256 / 512-B record per
    //                    (bracket, cell) of every RGL target (merl_rgl_values_grad.hip), n_wl x S x 32 B per (bracket, cell) of every
    //                    spectral RGL target (merl_rgl_spectral_values_grad.hip)
    //   BUF_GGX_GRAD     mrl_ggx_grad_batch: one 256-B row of partial sums per block + the sums of a host-array call (merl_ggx_grad.hip)
    //   BUF_GGX_GRAD_MAT mrl_ggx_grad_batch_mat / mrl_ggx_grad_queue: one 256-B row per block and target + the sums of a host-array
    //                    call (merl_ggx_grad_mat.hip); its own buffer, so that what a captured graph points at never moves
    enum { BUF_STAGE, BUF_QUEUES, BUF_PART_WORK, BUF_GRAD_BRICKS, BUF_GGX_GRAD, BUF_GGX_GRAD_MAT, BUF_COUNT };
    DeviceBuf buf[BUF_COUNT];
    int table_grad_kernel = 0;       // MRL_OPT_TABLE_GRAD_KERNEL
    std::vector<MaterialHost> materials;
    mrl::MaterialDev *d_materials = nullptr;
    size_t d_materials_cap = 0;
    size_t material_bytes = 0;       // sum of MaterialHost::bytes over live materials
    size_t memory_limit = 0;         // MRL_OPT_MEMORY_LIMIT_MB in bytes; 0 = none
    // what a tombstone points at: one all-zero cell (valid in both layouts) + a 1-row sampling marginal
    void *d_dummy = nullptr;
    mrl::Options opts{ 1, 0, 0, 0, 0, 0 };
    int kernel_variant = 3;          // MRL_OPT_KERNEL default: cooperative LDS-DMA brick fetch
    int table_layout = 1;            // layout of tables uploaded from now on (mrl::Layout)
    int table_param = 0;             // parameterisation of customized_measurement tables uploaded from now on (mrl::Param)
    size_t host_chunk = (size_t)1 << 22;
    int block_map = 0;               // MRL_OPT_BLOCK_MAP
    int rgl_search = 0;              // MRL_OPT_RGL_SEARCH
    int device_cus = 256;            // the device's compute units (compute_units = device_cus - reserved_cus sizes the persistent grids)
    int reserved_cus = 0;            // MRL_OPT_RESERVED_CUS
    hipStream_t masked_stream = nullptr;     // own stream restricted to the unreserved CUs (created by MRL_OPT_RESERVED_CUS > 0)
    int host_threads = 4;            // MRL_OPT_HOST_THREADS: copy threads of the pipelined host-array path; 0 = staged hipMemcpy path
    HostPipe pipe;
    ScalarDevice scalar_dev;
    std::atomic<ScalarSvc *> scalar{ nullptr };      // created by the first mrl_scalar_eval_sample
    // MRL_OPT_TABLE_ARENA_MB: one device allocation that RGB tables are placed in back to back (2 MiB aligned)
    char *arena = nullptr;
    size_t arena_bytes = 0, arena_used = 0;
    int arena_live = 0;              // tables currently placed in it; the bump pointer rewinds when the last one leaves
    std::string last_error;
};


#define MRL_GUARD(ctx) std::lock_guard<std::recursive_mutex> mrl_guard_((ctx)->mu)

#define MRL_HIP(ctx, expr)                                                                   \
    do {                                                                                     \
        hipError_t _e = (expr);                                                              \
        if (_e != hipSuccess) {                                                              \
            (void)hipGetLastError();                                                         \
            return fail((ctx), MRL_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(_e)); \
        }                                                                                    \
    } while (0)

// an allocation: out-of-memory is its own status (MRL_ERR_OOM), everything else MRL_ERR_HIP
#define MRL_ALLOC(ctx, expr)                                                                 \
    do {                                                                                     \
        hipError_t _e = (expr);                                                              \
        if (_e != hipSuccess) {                                                              \
            (void)hipGetLastError();                                                         \
            return fail((ctx), _e == hipErrorOutOfMemory ? MRL_ERR_OOM : MRL_ERR_HIP,        \
                        std::string(#expr) + ": " + hipGetErrorString(_e));                  \
        }                                                                                    \
    } while (0)

namespace mrlabi {

inline constexpr size_t kMaxSegments = 256 * 8 + 64;     // partition_geometry caps segments at 8 per CU

// ---- merl_calls.hip ----
// A whole-array call, host or device pointers: the RGB and n-channel entry points, and (wl / n_ch = W) the spectral ones
struct BatchCall {
    int mode;                                    // a mrl::Mode
    const float *wi, *wo, *u;
    const int32_t *mat;
    int32_t single_id;
    size_t n;
    float *out_rgb, *out_pdf, *out_wo, *out_pdf2, *out_weight;
    int n_ch = 0;                                // values per unit in out_rgb / out_weight.  0: three, the RGB entry points; > 0: *_nch and spectral calls
    const float *wl = nullptr;                   // spectral calls: n_ch wavelengths per unit, or NULL for the file's own nodes
};
StreamList streams_of(const BatchCall &c);                                   // the arrays a call of this mode touches
BatchCall on_slot(BatchCall c, char *const *addr, size_t m);                 // the same call on m units at one address per listed stream
mrl::BatchArgs batch_args(const mrl_ctx *ctx, const BatchCall &c);           // streams, materials, n_materials, opts; the rest zero
using HostLaunch = std::function<int(char *const *addr, size_t m)>;
// host arrays through the context's stage buffer, one chunk at a time (cap_bytes > 0: chunks so small that the slot stays below it)
int run_host_staged(mrl_ctx *ctx, const StreamList &streams, size_t n, size_t cap_bytes, const HostLaunch &launch);

// A direction-gradient call (include/merl_hip_diff*.h), whole arrays or a queue, and what its family of materials supplies
// a further per-unit array of a direction-gradient call (the spectral RGL gradient: wavelengths in, grad_wavelengths out)
struct DirGradExtra {
    void *ptr;                                   // null: the call goes without it — unless `required`
    size_t unit_bytes;
    bool out;                                    // an output counts among the outputs of which one must be given
    const char *name;
    bool required;                               // null is MRL_ERR_INVALID ("null array argument")
};
struct DirGradCall {
    const float *wi, *wo, *g;
    const int32_t *mat;
    int32_t single_id;
    size_t n;                                    // units; queued: the queue's capacity
    bool queued;
    const uint32_t *queue, *queue_count;
    float *grad_wi, *grad_wo;                    // either may be null; one output (an `out` extra counts) must be given
    std::vector<DirGradExtra> extra = {};        // in the order the family's launch receives their addresses
};
struct DirGradFamily {
    size_t g_bytes;                              // of g per unit
    const char *g_name;
    std::function<bool(const MaterialHost &)> evaluates;     // a call without ids: is its material one of the family's?
    std::string not_evaluated;                   // the MRL_ERR_MATERIAL message if it is not
    bool refuses_renormalise;                    // MRL_OPT_NEGATIVE = renormalise: MRL_ERR_INVALID
    std::function<mrl::MaterialDev()> single_with_ids;       // BatchArgs::single of a launch with ids: what a unit of another id reads
    // the family's kernel on device-accessible arrays; a: everything but the outputs; extra: one address per DirGradCall::extra
    // entry (null where the call goes without it; nullptr itself when the call lists none)
    std::function<hipError_t(const mrl::BatchArgs &a, const float *g, float *grad_wi, float *grad_wo, void *const *extra)> launch;
    size_t cap_bytes = 0;                        // host arrays: > 0, chunks so small that the staging slot stays below it
    // the second input of a unit, DirGradCall::wo / BatchArgs::wo: a direction — or the two random numbers of the sample gradient
    // (merl_ggx_sample_grad.hip: 8, "u"; that family has no grad_wo)
    size_t second_bytes = 12;
    const char *second_name = "wo";
};
// checks in the order the headers document, then f.launch on the caller's device arrays or chunk by chunk on staged host arrays
int grad_dir_call(mrl_ctx *ctx, const DirGradCall &c, const DirGradFamily &f);

// ---- merl_grad_scatter.hip ----
// An adjoint-of-eval call (include/merl_hip.h mrl_table_grad_batch, merl_hip_fit_table.h, merl_hip_fit_nch.h, merl_hip_fit_rgl.h,
// merl_hip_fit_rgl_spectral.h):
// a gradient scattered into the measured data of the call's targets, whole arrays or a queue, and what its family supplies
struct GradScatterCall {
    const float *wi, *wo, *g;
    size_t g_bytes;                              // of g per unit
    const char *g_name;
    const int32_t *mat;
    int32_t single_id;
    size_t n;                                    // units; queued: the queue's capacity
    bool queued;
    const uint32_t *queue, *queue_count;
    const int32_t *target_ids;
    int n_targets, max_targets;
    double *out;                                 // the targets' gradients end to end, added to
    // one further per-unit input array (the spectral RGL adjoint: wavelengths); null: the call goes without it
    const void *extra = nullptr;
    size_t extra_bytes = 0;                      // of extra per unit
    const char *extra_name = nullptr;
    size_t cap_bytes = 0;                        // host arrays: > 0, chunks so small that the staging slot stays below it
};
struct GradScatterLayout {
    size_t brick_bytes;                          // of BUF_GRAD_BRICKS; 0: the launch adds straight into `out` — no reserve, no clear, no fold
    size_t out_doubles;                          // of `out`, over all targets
    bool nothing_to_add = false;                 // the call is MRL_OK once its arguments are checked; no workspace is touched
};
struct GradScatterFamily {
    std::function<int(int32_t id)> check_target;             // MRL_OK, or the failure (through fail) the family's header documents
    std::function<int(GradScatterLayout &)> layout;          // after every target passed: fills the family's own descriptors
    bool refuses_renormalise;                    // MRL_OPT_NEGATIVE = renormalise: MRL_ERR_INVALID
    // the accumulate kernel on m units at device-accessible arrays: addr[0..2] wi, wo, g and, where the call has one, addr[3] mat;
    // where the call has an extra array it follows as the last address (addr[4] with mat, addr[3] without);
    // into the cleared bricks, or (brick_bytes = 0: bricks is null) into out
    std::function<hipError_t(char *const *addr, size_t m, double *bricks, double *out)> launch;
    std::function<hipError_t(const double *bricks, double *out)> fold;   // once per call, target by target; not called without bricks
};
// checks in the order the headers document; clear, launch and fold on the caller's device arrays, or chunk by chunk on staged host
// arrays with the sums gathered on the device and added to the caller's on the host.  A queue call copies nothing from host memory
// at call time and is capturable: so is the clear, which is why it is a kernel (launch_grad_clear)
int grad_scatter_call(mrl_ctx *ctx, const GradScatterCall &c, const GradScatterFamily &f);
// zeros `bytes` (a multiple of 16) of gradient bricks with 16-B stores
hipError_t launch_grad_clear(double *bricks, size_t bytes, int compute_units, hipStream_t stream);

// ---- merl_abi.hip ----
// a non-blocking stream whose kernels may use all but `reserved` of the device's `device_cus` compute units (reserved = 0: a plain
// stream).  The reserved CUs are spread evenly over the mask (one per XCD for 8): what a communication library's kernels — RCCL's
// send / receive — run on while a persistent compute grid owns the rest (include/merl_hip.h, MRL_OPT_RESERVED_CUS).
hipError_t create_compute_stream(int device_cus, int reserved, hipStream_t *out);
int fail(mrl_ctx *ctx, int status, const std::string &msg);
int pointer_kind(const void *p);                                  // 1 = the device can dereference it, 0 = plain host
int common_kind(std::initializer_list<const void *> ptrs, const StreamList &streams = {});    // 0 / 1, or -1 on a mix
int sync_material_array(mrl_ctx *ctx);
int ensure_dummy(mrl_ctx *ctx);
mrl::MaterialDev tombstone_dev(const mrl_ctx *ctx);
int budget_check(mrl_ctx *ctx, size_t need, size_t in_arena = 0);
bool arena_has_room(const mrl_ctx *ctx, size_t bytes);           // would table_alloc place `bytes` in the context's arena?
int place_material(mrl_ctx *ctx, const MaterialHost &m, int *out_id);
hipError_t table_alloc(mrl_ctx *ctx, size_t bytes, float4 **out, bool *in_arena);
void table_free(mrl_ctx *ctx, float4 *p, bool in_arena);

// Whoever changes what a running service instance reads (the material array, the tables behind it, the options) holds one
// of these: no scalar call is in flight and no instance is running while it lives (merl_scalar_host.hpp, "writer").
struct ScalarPause {
    ScalarSvc *svc;
    explicit ScalarPause(mrl_ctx *ctx) : svc(ctx->scalar.load(std::memory_order_acquire))
    {
        if (svc && !svc->pause()) ctx->scalar_dev.ok.store(false, std::memory_order_relaxed);
    }
    ~ScalarPause() { if (svc) svc->resume(); }
    ScalarPause(const ScalarPause &) = delete;
    ScalarPause &operator=(const ScalarPause &) = delete;
};

} // namespace mrlabi
