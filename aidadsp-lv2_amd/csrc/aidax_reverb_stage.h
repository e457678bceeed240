// aidax_reverb_stage.h — the bus reverbs between k_mix and k_bus_limit (include/aidax.h, "Bus reverbs"): ReverbBook, the host-only half
// (no HIP call: the buses' records and parameters, what the device has not seen of them, the frame position, the epochs and their
// refresh), and ReverbStage, the device half around k_bus_reverb (aidax_bus_reverb.hip). Issues HIP calls: include it last.
#pragma once

#include <cmath>
#include <cstddef>
#include <utility>
#include <vector>

#include "aidax_snapshot_ring.h"

namespace aidax {

static_assert(sizeof(aidax_bus_reverb_rec) == sizeof(ReverbRec) && offsetof(aidax_bus_reverb_rec, gq) == offsetof(ReverbRec, gq) &&
                  offsetof(aidax_bus_reverb_rec, a) == offsetof(ReverbRec, a) && offsetof(aidax_bus_reverb_rec, dry) == offsetof(ReverbRec, dry) &&
                  offsetof(aidax_bus_reverb_rec, on) == offsetof(ReverbRec, on) && offsetof(aidax_bus_reverb_rec, epoch) == offsetof(ReverbRec, epoch),
              "k_bus_reverb's record is aidax_bus_reverb_rec");
static_assert(AIDAX_BUS_REVERB_LINES == kReverbLines && AIDAX_BUS_REVERB_MIN_DELAY == kReverbMinDelay && AIDAX_BUS_REVERB_MAX_DELAY == kReverbMaxDelay,
              "the header's bounds are the kernel's");

// The reverbs' host records, all of them the audio side's; sized once (init), so that a change allocates nothing. `frames` counts the
// reverberated frames issued so far; its low 32 bits are the absolute frame of the next reverberated pass's first frame, what
// k_bus_reverb takes as its position. since[b] is `frames` at bus b's epoch; the record's own `epoch` is the device's view of it, modulo
// 2^32, which refresh() keeps less than half the range behind the position.
struct ReverbBook {
    // an epoch this far behind the position is moved forward; looked for once in kScanEvery frames, so that no epoch the kernel
    // compares with is ever 2^31 frames behind (2^30 + 2^24 + a pass of at most 2^16 frames)
    static constexpr uint32_t kStale = 1u << 30, kScanEvery = 1u << 24;
    uint32_t n_buses = 0, max_delay = 0;
    std::vector<ReverbRec> h_rec;
    std::vector<aidax_bus_reverb_params> params;         // as last set by parameters; zeros for a bus set by a record of the caller's own
    std::vector<uint64_t> since;
    DirtyRange dirty;                                    // records the device has not seen
    uint64_t frames = 0;
    uint64_t next_scan = kScanEvery;                     // `frames` at which refresh() looks at the epochs again
    bool refreshes = true;                               // (false: tests/asan_reverb_harness.cpp shows what breaks without the refresh)

    void init(uint32_t buses, uint32_t delay_cap)
    {
        n_buses = buses; max_delay = delay_cap;
        h_rec.assign(buses, ReverbRec{});
        params.assign(buses, aidax_bus_reverb_params{});
        since.assign(buses, 0);
        dirty.clear();
        frames = 0;
        next_scan = kScanEvery;
    }
    uint32_t pos() const { return static_cast<uint32_t>(frames); }
    // floats of one line's ring row: the smallest power of two that holds the longest history a record within the capacity reads
    // (max_delay + 1 frames) next to a pass of max_frames
    static uint32_t ring_row(uint32_t delay_cap, uint32_t max_frames)
    {
        return pow2_at_least(delay_cap + 1u + max_frames);
    }
    // the record's own conditions (include/aidax.h), whatever the capacity; `on` and `epoch` are the book's and are not read
    static bool valid(const aidax_bus_reverb_rec& r)
    {
        auto level = [](float v) { return std::isfinite(v) && std::fabs(v) <= 4.f; };
        for (uint32_t i = 0; i < kReverbLines; ++i) {
            if (r.m[i] < kReverbMinDelay || r.m[i] > kReverbMaxDelay) return false;
            if (!(r.gq[i] >= 0.f && static_cast<double>(r.gq[i]) < 0.35355339059327373)) return false;      // (1 / sqrt(8); false for a NaN)
        }
        return r.a >= 0.f && r.a <= 0.5f && level(r.wet) && level(r.dry);
    }
    bool fits(const aidax_bus_reverb_rec& r) const
    {
        for (uint32_t i = 0; i < kReverbLines; ++i)
            if (r.m[i] > max_delay) return false;
        return true;
    }
    // Buses [lo, hi) get the record and, where it was designed from parameters, those (set_params == nullptr: a record of the caller's
    // own), or (rec == nullptr) their reverbs go off. A bus that goes on, or whose delays change, starts a new epoch at the next pass's
    // first frame; a change of gq, a, wet or dry alone keeps its memories. false, and nothing changed: a delay beyond the capacity.
    bool set(uint32_t lo, uint32_t hi, const aidax_bus_reverb_rec* rec, const aidax_bus_reverb_params* set_params)
    {
        if (rec && !fits(*rec)) return false;
        for (uint32_t b = lo; b < hi; ++b) {
            ReverbRec& h = h_rec[b];
            if (!rec) { h.on = 0u; continue; }
            const bool cut = h.on == 0u || std::memcmp(h.m, rec->m, sizeof h.m) != 0;
            std::memcpy(h.m, rec->m, sizeof h.m);
            std::memcpy(h.gq, rec->gq, sizeof h.gq);
            h.a = rec->a; h.wet = rec->wet; h.dry = rec->dry;
            h.on = 1u;
            if (cut) { h.epoch = pos(); since[b] = frames; }
            params[b] = set_params ? *set_params : aidax_bus_reverb_params{};
        }
        dirty.mark(lo, hi - 1);
        return true;
    }
    // the memories of buses [lo, hi) are cut at the next pass's first frame (a bus whose reverb is off starts a new epoch when it goes on anyway)
    void reset(uint32_t lo, uint32_t hi)
    {
        for (uint32_t b = lo; b < hi; ++b) { h_rec[b].epoch = pos(); since[b] = frames; }
        dirty.mark(lo, hi - 1);
    }
    uint64_t since_epoch(uint32_t bus) const { return frames - since[bus]; }
    // Ahead of a reverberated pass: the device compares frame positions modulo 2^32, so an epoch may not fall half the range behind.
    // Any epoch older than the longest delay + 1 gives the same result; a stale one moves to exactly there.
    void refresh()
    {
        if (!refreshes || frames < next_scan) return;
        next_scan = frames + kScanEvery;
        for (uint32_t b = 0; b < n_buses; ++b) {
            ReverbRec& h = h_rec[b];
            if (h.on == 0u || pos() - h.epoch < kStale) continue;          // (an off bus takes a new epoch when it goes on)
            h.epoch = pos() - (max_delay + 1u);
            dirty.mark(b, b);
        }
    }
    // a reverberated pass of n_frames has been issued at pos()
    void advance(uint32_t n_frames) { frames += n_frames; }
};

// The device half: nothing until enable(), the set-up side's first aidax_pool_set_bus_reverbs with on != 0; from then on `on` is a host
// record of the audio side. While it is set, k_bus_reverb of a pass works in place on the block k_mix wrote. HIP failures leave as HipFail.
struct ReverbStage {
    ReverbBook book;
    DevBuf<float> d_ring;            // [n_buses][8][ring_row]: every line's memory; empty: never enabled
    DevBuf<ReverbRec> d_rec;         // [n_buses]
    SnapshotRing ring;
    uint32_t ring_row = 0;
    bool on = false;

    bool enabled() const { return static_cast<bool>(d_ring); }
    // the rings (zeroed), the records (all off) and the snapshots; all or nothing
    void enable(uint32_t n_buses, uint32_t max_frames, uint32_t delay_cap, hipStream_t q)
    {
        const size_t n = n_buses;
        ReverbStage fresh;
        fresh.ring_row = ReverbBook::ring_row(delay_cap, max_frames);
        const size_t ring_floats = n * kReverbLines * fresh.ring_row;
        fresh.d_ring.alloc(ring_floats);
        fresh.d_rec.alloc(n);
        fresh.d_ring.zero(0, ring_floats, q);
        fresh.d_rec.zero(0, n, q);
        HIP_TRY(hipStreamSynchronize(q));                // (a pass on a caller's stream must find them cleared)
        fresh.ring.alloc(sizeof(ReverbRec) * n);
        fresh.book.init(n_buses, delay_cap);
        fresh.on = true;
        *this = std::move(fresh);
    }
    // Behind k_mix of a pass of n_frames > 0 that wrote `block`: the records, if one has changed since the last upload, then
    // k_bus_reverb in place, then the position moves on (a pass that fails on its way here leaves it where it was)
    void after_mix(float* block, uint32_t n_frames, hipStream_t s)
    {
        book.refresh();
        ring.upload_dirty(d_rec.get(), book.h_rec.data(), book.dirty, s);
        BusReverbArgs a{};
        a.block = block; a.ring = d_ring.get(); a.rec = d_rec.get();
        a.n_buses = book.n_buses; a.n_frames = n_frames; a.mask = ring_row - 1u; a.pos = book.pos(); a.max_delay = book.max_delay;
        HIP_TRY(launch_bus_reverb(a, s));
        book.advance(n_frames);
    }
};

}  // namespace aidax
