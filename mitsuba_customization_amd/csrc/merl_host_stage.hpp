// merl_host_stage.hpp — the host-array path of every call that takes whole arrays (RGB, n-channel, spectral, table gradient), host
// C++ only (no HIP: tests/host_stage_asan.cpp drives it on the CPU).  A call's arrays are DATA: an ordered list of streams.  The null
// check, the host-or-device kind, the layout of a staging slot and the copies of a chunk are all derived from that one list; the
// chunk loop is written once and moves the data through a Mover (merl_calls.hip: staged through HBM, or pipelined through pinned
// double buffers).
#pragma once
#include <algorithm>
#include <condition_variable>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <mutex>
#include <thread>
#include <vector>

namespace mrlabi {

// one array of a call: `unit_bytes` per unit, read (in) or written (out) by the kernel.  A stream the mode does not use is not listed.
struct HostStream {
    void *ptr;                       // the caller's array (an in-stream is never written through it)
    size_t unit_bytes;               // 12 wi / wo / out_wo, 8 u, 4 mat / pdf, 4 * C values and weights, 4 * W wavelengths
    bool out;
    const char *name;                // for error text
};
using StreamList = std::vector<HostStream>;

inline const HostStream *first_null(const StreamList &streams)
{
    for (const HostStream &s : streams) if (!s.ptr) return &s;
    return nullptr;
}

// where each stream of a `chunk`-unit slot starts (256-byte aligned, list order); one more entry at the end: the size of the slot
inline std::vector<size_t> slot_layout(const StreamList &streams, size_t chunk)
{
    std::vector<size_t> offset{ 0 };
    for (const HostStream &s : streams) offset.push_back(offset.back() + ((s.unit_bytes * chunk + 255) & ~(size_t)255));
    return offset;
}

// units per chunk: at most `max_chunk`, and (cap_bytes > 0) so few that the slot stays within cap_bytes
inline size_t chunk_units(const StreamList &streams, size_t n, size_t max_chunk, size_t cap_bytes)
{
    size_t unit = 0;
    for (const HostStream &s : streams) unit += s.unit_bytes;
    const size_t pad = 256 * streams.size();
    if (cap_bytes && unit) max_chunk = std::min(max_chunk, cap_bytes > pad + unit ? (cap_bytes - pad) / unit : 1);
    return std::max<size_t>(1, std::min(n, max_chunk));
}

struct CopySeg { void *dst; const void *src; size_t bytes; const char *name = nullptr; };      // name: the stream's, for error text

// The chunk loop.  Per chunk k: copy-in -> launch on slot k -> copy-out of chunk k - depth.  A Mover provides
//   depth            0: one slot, the copy-out of chunk k follows its launch;  1: two slots, the copy-out of chunk k - 1 overlaps kernel k
//   prepare(bytes)   slots of `bytes` each
//   slot(k)          the address of chunk k's slot as the device sees it
//   copy_in(k, segs), launched(k), copy_out(k, segs)   (copy_out returns when the caller's arrays hold chunk k)
//   drain()          nothing of this call is in flight any more
// and returns 0 or a status, as does launch(slot address of each listed stream, units of the chunk).  The first status other than 0
// ends the call: no later launch, no copy-out of the failed chunk, and drain() before it is returned.
template <class Mover, class Launch>
int run_chunks(Mover &mv, const StreamList &streams, size_t n, size_t max_chunk, size_t cap_bytes, Launch &&launch)
{
    const size_t chunk = chunk_units(streams, n, max_chunk, cap_bytes), steps = (n + chunk - 1) / chunk;
    const std::vector<size_t> offset = slot_layout(streams, chunk);
    auto units = [&](size_t k) { return std::min(chunk, n - k * chunk); };
    auto copies = [&](size_t k, bool out) {                  // the copies of chunk k in one direction
        const size_t first = k * chunk, m = units(k);
        std::vector<CopySeg> segs;
        for (size_t i = 0; i < streams.size(); ++i) {
            const HostStream &s = streams[i];
            if (s.out != out) continue;
            char *user = (char *)s.ptr + first * s.unit_bytes, *slot = mv.slot(k) + offset[i];
            segs.push_back(out ? CopySeg{ user, slot, m * s.unit_bytes, s.name } : CopySeg{ slot, user, m * s.unit_bytes, s.name });
        }
        return segs;
    };
    int rc = mv.prepare(offset.back());
    if (rc) return rc;
    std::vector<char *> addr(streams.size());
    for (size_t k = 0; k < steps + mv.depth && !rc; ++k) {
        if (k < steps) {
            rc = mv.copy_in(k, copies(k, false));
            for (size_t i = 0; i < streams.size(); ++i) addr[i] = mv.slot(k) + offset[i];
            if (!rc) rc = launch(addr.data(), units(k));
            if (!rc) rc = mv.launched(k);
        }
        if (!rc && k >= mv.depth) rc = mv.copy_out(k - mv.depth, copies(k - mv.depth, true));
    }
    if (rc) mv.drain();
    return rc;
}

// ---- the copy threads of the pipelined mover -------------------------------------------------------------------------
// A host that holds plain (pageable) arrays — what a CPU renderer hands over — used to be staged with hipMemcpyAsync,
// which the runtime serialises through one bounce buffer at ~11 GB/s (140-150 M units/s).  Instead: a few copy threads
// move chunk c+1 of the caller's arrays into pinned, device-mapped buffers and chunk c-1 of the results out of them,
// while the kernel of chunk c reads and writes the pinned buffers over PCIe itself (zero copy, no staging in HBM).
struct CopyPool {
    using Seg = CopySeg;
    std::vector<std::thread> workers;
    std::mutex mu;
    std::condition_variable wake, done;
    std::vector<Seg> segs;
    size_t next = 0, finished = 0;
    uint64_t generation = 0;
    bool quit = false;

    void start(int n)
    {
        for (int t = 0; t < n; ++t)
            workers.emplace_back([this]() {
                uint64_t seen = 0;
                for (;;) {
                    std::unique_lock<std::mutex> lk(mu);
                    wake.wait(lk, [&]() { return quit || (generation != seen && next < segs.size()) || (generation != seen && segs.empty()); });
                    if (quit) return;
                    if (next >= segs.size()) { seen = generation; continue; }
                    while (next < segs.size()) {
                        const Seg sg = segs[next++];
                        lk.unlock();
                        std::memcpy(sg.dst, sg.src, sg.bytes);
                        lk.lock();
                        if (++finished == segs.size()) done.notify_all();
                    }
                    seen = generation;
                }
            });
    }
    // copies every segment, split into slices so that all workers (and the caller) share the work; returns when done
    void run(const std::vector<Seg> &whole)
    {
        constexpr size_t kSlice = (size_t)2 << 20;
        std::vector<Seg> sliced;
        for (const Seg &w : whole)
            for (size_t off = 0; off < w.bytes; off += kSlice)
                sliced.push_back({ (char *)w.dst + off, (const char *)w.src + off, std::min(kSlice, w.bytes - off) });
        if (sliced.empty()) return;
        if (workers.empty()) { for (const Seg &sg : sliced) std::memcpy(sg.dst, sg.src, sg.bytes); return; }
        std::unique_lock<std::mutex> lk(mu);
        segs = std::move(sliced); next = 0; finished = 0; ++generation;
        wake.notify_all();
        while (next < segs.size()) {                              // the caller copies too
            const Seg sg = segs[next++];
            lk.unlock();
            std::memcpy(sg.dst, sg.src, sg.bytes);
            lk.lock();
            ++finished;
        }
        done.wait(lk, [&]() { return finished == segs.size(); });
        segs.clear();
    }
    void stop()
    {
        { std::lock_guard<std::mutex> lk(mu); quit = true; }
        wake.notify_all();
        for (auto &t : workers) t.join();
        workers.clear();
    }
};

} // namespace mrlabi
