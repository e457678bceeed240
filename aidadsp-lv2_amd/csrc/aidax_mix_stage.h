// aidax_mix_stage.h — the mix buses behind a pool's last stage (include/aidax.h, "Mix buses"): MixBook, the host-only half (no HIP
// call: the sends, their ramps, the CSR plan built from them, what the device has not seen, the advance per pass and per prefix;
// aidax_mix_book.cpp), and MixStage, the device half around k_mix (aidax_mix.hip). Issues HIP calls: include it last.
#pragma once

#include <algorithm>
#include <cstddef>
#include <utility>
#include <vector>

#include "aidax_snapshot_ring.h"

namespace aidax {

// A send is (bus, gain ramp). `bus` is what the next pass plays; `played_bus` and `now` are the state behind the last pass issued for
// the stream: the bus the send was on and the fp32 gain of its last frame there. Every aidax_pool_set_send is judged against that
// state alone, so of several calls between two passes the last one wins and starts from the same g0.
// The ramp is IrPlan::Ramp's: g0 -> g1 over `len` frames, `k` of which have been issued (saturating at max(len, 1)); ramp frame k
// carries g1 once k + 1 >= len, so a ramp of 0 or 1 frames is a jump at the block boundary (ramp_value, aidax_kernels.h).
//
// The plan (bus_start, entries: what k_mix reads) is rebuilt ahead of the pass that follows any aidax_pool_set_send, with every
// entry's ramp as it stands. It is NOT rebuilt as ramps move on: the frames issued since the rebuild travel as k_mix's k_off
// (since_build, the same for every entry, since a pass advances them all; saturating at kMixMaxRampOffset, beyond any ramp's end), so a
// pass without a changed send uploads nothing, running ramps or not. A prefix pass that leaves out a stream whose entry was moving
// at the rebuild, and may still be (fewer than moving_left frames issued since), marks the plan for another one: that entry is
// where it was, the others are not.
struct MixBook {
    struct Send {
        int32_t bus = AIDAX_BUS_NONE, played_bus = AIDAX_BUS_NONE;
        float g0 = 0.f, g1 = 0.f, now = 0.f;
        uint32_t len = 0, k = 1;
    };
    uint32_t n_streams = 0, n_buses = 0;
    std::vector<Send> sends;                 // [n_streams][AIDAX_SENDS]
    std::vector<uint32_t> bus_start;         // [n_buses + 1]
    std::vector<MixEntry> entries;           // [n_streams * AIDAX_SENDS], n_entries of them in use
    uint32_t n_entries = 0, max_entries = 0; // max_entries: the longest bus's
    uint32_t since_build = 0;
    int64_t moving_hi = -1;                  // the last stream with an entry that was still moving at the rebuild (-1: none)
    uint32_t moving_left = 0;                // the most frames any entry had left at the rebuild: since_build beyond it, none moves
    uint32_t n_unsettled = 0;                // sends whose state behind the next pass differs from the one behind the last
    bool dirty = true;

    void init(uint32_t streams, uint32_t buses);      // (set-up side: the only allocation)
    Send& at(uint32_t stream, uint32_t send) { return sends[static_cast<size_t>(stream) * AIDAX_SENDS + send]; }
    const Send& at(uint32_t stream, uint32_t send) const { return sends[static_cast<size_t>(stream) * AIDAX_SENDS + send]; }
    static uint32_t frames_left(const Send& x) { return std::max(x.len, 1u) - x.k; }
    static bool unsettled(const Send& x) { return x.bus != x.played_bus || frames_left(x) != 0; }
    // g_now: the gain of the send's last issued frame on the bus it is set to (0: never played there)
    static float gain_now(const Send& x) { return x.bus != AIDAX_BUS_NONE && x.bus == x.played_bus ? x.now : 0.f; }
    // aidax_pool_set_send for one stream (arguments checked by the caller)
    void set(uint32_t stream, uint32_t send, int32_t bus, float gain, uint32_t len);
    // the plan for the pass about to be issued
    void rebuild();
    // a pass of n_frames for the first n_active streams has been issued: their sends move on
    void advance(uint32_t n_active, uint32_t n_frames);
    // The plan's bytes on the device and in a snapshot: bus_start, then the entries. serialise() returns the length to upload.
    size_t entries_off() const { return sizeof(uint32_t) * (static_cast<size_t>(n_buses) + 1u); }
    size_t plan_bytes() const { return entries_off() + sizeof(MixEntry) * entries.size(); }
    size_t serialise(uint8_t* snapshot) const;
};

// The device half: nothing until enable(), the set-up side's first aidax_pool_set_buses with a count; from then on `on` is a host record
// of the audio side, and a pass issued while it is set ends with k_mix over the block it returns. HIP failures leave as HipFail.
struct MixStage {
    MixBook book;
    DevBuf<float> d_bus;             // the bus block: [n_buses][max_frames] floats, rows dense at the last mixed pass's n_frames; empty: never enabled
    DevBuf<uint8_t> d_plan;          // bus_start and entries (MixBook::serialise)
    PinnedBuf<float> h_bus;          // pinned staging of the reads, the bus block's size
    SnapshotRing ring;
    bool on = false;
    uint32_t last_frames = 0;        // n_frames of the last pass mixed (0: none yet)

    bool enabled() const { return static_cast<bool>(d_bus); }
    // the bus block (zeroed), the plan, its snapshots and the pinned staging of the reads; all or nothing
    void enable(uint32_t n_streams, uint32_t max_frames, uint32_t n_buses, hipStream_t q)
    {
        MixStage fresh;
        const size_t block = n_buses * static_cast<size_t>(max_frames);
        fresh.book.init(n_streams, n_buses);
        fresh.d_bus.alloc(block);
        fresh.d_plan.alloc(fresh.book.plan_bytes());
        fresh.h_bus.alloc(block);
        fresh.d_bus.zero(0, block, q);
        HIP_TRY(hipStreamSynchronize(q));                // (a pass on a caller's stream must find it zeroed)
        fresh.ring.alloc(fresh.book.plan_bytes());
        fresh.on = true;
        *this = std::move(fresh);
    }
    // Behind the last stage of a pass of n_frames > 0: the plan, if a send has changed since the last one went up, then k_mix over the
    // block the pass returns, then the sends move on (a pass that fails on its way here leaves them where they were). `d_raw`: where k_mix
    // writes instead of the bus block while the bus limiters are on (aidax_limit_stage.h: k_bus_limit then writes the bus block)
    void after_pass(const float* d_out, uint32_t n_active, uint32_t n_frames, hipStream_t s, float* d_raw = nullptr)
    {
        if (book.dirty) {
            book.rebuild();
            const size_t bytes = book.serialise(ring.take());
            ring.send(d_plan.get(), 0, bytes, s);
        }
        MixArgs a{};
        a.bus_start = reinterpret_cast<const uint32_t*>(d_plan.get());
        a.entries = reinterpret_cast<const MixEntry*>(d_plan.get() + book.entries_off());
        a.y = d_out;
        a.out = d_raw ? d_raw : d_bus.get();
        a.n_buses = book.n_buses; a.n_streams = n_active; a.n_frames = n_frames; a.k_off = book.since_build;
        HIP_TRY(launch_mix(a, book.max_entries, s));
        book.advance(n_active, n_frames);
        last_frames = n_frames;
    }
    // rows [first, first + count) of the last mixed pass's bus block, count * last_frames floats, behind everything on q (waits)
    void read(uint32_t first, uint32_t count, float* out, hipStream_t q)
    {
        const size_t at = static_cast<size_t>(first) * last_frames;
        read_back(out, h_bus.get() + at, d_bus.get() + at, sizeof(float) * count * static_cast<size_t>(last_frames), q);
    }
};

}  // namespace aidax
