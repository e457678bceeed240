// aidax_limit_stage.h — the bus limiters and bus meters behind k_mix (include/aidax.h, "Bus limiters"): LimitBook, the host-only half (no
// HIP call: the buses' records, what the device has not seen of them, the ring position), and LimitStage, the device half around
// k_bus_limit (aidax_bus_limit.hip). Issues HIP calls: include it last.
#pragma once

#include <cstddef>
#include <utility>
#include <vector>

#include "aidax_snapshot_ring.h"

namespace aidax {

static_assert(sizeof(aidax_bus_limit_rec) == sizeof(LimitRec) && offsetof(aidax_bus_limit_rec, lookahead) == offsetof(LimitRec, lookahead) &&
                  offsetof(aidax_bus_limit_rec, hold) == offsetof(LimitRec, hold) && offsetof(aidax_bus_limit_rec, on) == offsetof(LimitRec, on),
              "k_bus_limit's record is aidax_bus_limit_rec");
static_assert(sizeof(aidax_bus_meter) == sizeof(BusMeterRec) && offsetof(aidax_bus_meter, limited) == offsetof(BusMeterRec, limited) &&
                  offsetof(aidax_bus_meter, in_peak) == offsetof(BusMeterRec, in_peak) && offsetof(aidax_bus_meter, min_gain) == offsetof(BusMeterRec, min_gain),
              "k_bus_limit's meter record is aidax_bus_meter");
static_assert(AIDAX_BUS_LOOKAHEAD_MAX == kLimitMaxLookahead && AIDAX_BUS_HOLD_MAX == kLimitMaxHold, "the header's bounds are the kernel's");

// The limiters' host records, all of them the audio side's; sized once (init), so that a change allocates nothing. `pos` is the absolute
// frame, modulo 2^32, of the next limited pass's first frame: what k_bus_limit takes as its ring position.
struct LimitBook {
    uint32_t n_buses = 0, max_lookahead = 0, max_hold = 0;
    std::vector<LimitRec> h_rec;
    std::vector<aidax_bus_limit_params> params;          // as last set, kept for the buses whose limiter is on
    DirtyRange dirty;                                    // records the device has not seen
    uint32_t pos = 0;

    void init(uint32_t buses, uint32_t lookahead_cap, uint32_t hold_cap)
    {
        n_buses = buses; max_lookahead = lookahead_cap; max_hold = hold_cap;
        h_rec.assign(buses, LimitRec{});
        params.assign(buses, aidax_bus_limit_params{});
        dirty.clear();
        pos = 0;
    }
    // floats of a bus's ring row: the smallest power of two that holds the longest history a record within the capacities reads
    // (2 L + H - 1 frames) next to a pass of max_frames
    static uint32_t ring_row(uint32_t lookahead_cap, uint32_t hold_cap, uint32_t max_frames)
    {
        return pow2_at_least(2u * lookahead_cap + hold_cap - 1u + max_frames);
    }
    bool fits(const aidax_bus_limit_rec& r) const { return r.lookahead >= 1u && r.lookahead <= max_lookahead && r.hold <= max_hold; }
    // Buses [lo, hi) get the designed record and its parameters, or (designed == nullptr) their limiters go off. false, and nothing
    // changed: the record lies beyond the capacities.
    bool set(uint32_t lo, uint32_t hi, const aidax_bus_limit_rec* designed, const aidax_bus_limit_params* set_params)
    {
        if (designed && !fits(*designed)) return false;
        for (uint32_t b = lo; b < hi; ++b) {
            if (designed) { std::memcpy(&h_rec[b], designed, sizeof(LimitRec)); h_rec[b].on = 1u; params[b] = *set_params; }
            else h_rec[b].on = 0u;
        }
        dirty.mark(lo, hi - 1);
        return true;
    }
    uint32_t latency(uint32_t bus) const { return h_rec[bus].on ? h_rec[bus].lookahead : 0u; }
    // a limited pass of n_frames has been issued at `pos`
    void advance(uint32_t n_frames) { pos += n_frames; }
};

// The device half: nothing until enable(), the set-up side's first aidax_pool_set_bus_limiting with on != 0; from then on `on` is a host
// record of the audio side. While it is set, k_mix of a pass writes into the raw side block and k_bus_limit turns that into the pool's
// bus block. HIP failures leave as HipFail.
struct LimitStage {
    LimitBook book;
    DevBuf<float> d_raw;             // the raw bus block k_mix writes while the stage is on: [n_buses][max_frames]; empty: never enabled
    DevBuf<float> d_ring;            // [n_buses][ring_row]: the sanitised samples of every bus's past
    DevBuf<LimitRec> d_rec;          // [n_buses]
    DevBuf<BusMeterRec> d_meter;     // [n_buses]
    PinnedBuf<BusMeterRec> h_meter;  // [n_buses] staging of the read, then [n_buses] cleared records (what a clear copies up)
    SnapshotRing ring;
    uint32_t ring_row = 0;
    bool on = false;

    bool enabled() const { return static_cast<bool>(d_raw); }
    // the side block, the rings (zeroed), the records (all off), the meter records (cleared), the snapshots and the pinned staging; all or nothing
    void enable(uint32_t n_buses, uint32_t max_frames, uint32_t lookahead_cap, uint32_t hold_cap, hipStream_t q)
    {
        const size_t n = n_buses;
        LimitStage fresh;
        fresh.ring_row = LimitBook::ring_row(lookahead_cap, hold_cap, max_frames);
        fresh.d_raw.alloc(n * max_frames);
        fresh.d_ring.alloc(n * fresh.ring_row);
        fresh.d_rec.alloc(n);
        fresh.d_meter.alloc(n);
        fresh.h_meter.alloc(2u * n);
        BusMeterRec* cleared = fresh.h_meter.get() + n;
        for (size_t b = 0; b < n; ++b) { cleared[b] = BusMeterRec{}; cleared[b].min_gain = 1.f; }
        fresh.d_ring.zero(0, n * fresh.ring_row, q);
        fresh.d_rec.zero(0, n, q);
        HIP_TRY(hipMemcpyAsync(fresh.d_meter.get(), cleared, sizeof(BusMeterRec) * n, hipMemcpyHostToDevice, q));
        HIP_TRY(hipStreamSynchronize(q));                // (a pass on a caller's stream must find them cleared)
        fresh.ring.alloc(sizeof(LimitRec) * n);
        fresh.book.init(n_buses, lookahead_cap, hold_cap);
        fresh.on = true;
        *this = std::move(fresh);
    }
    // Behind k_mix of a pass of n_frames > 0 that wrote d_raw: the records, if one has changed since the last upload, then k_bus_limit
    // into the pool's bus block, then the ring position moves on (a pass that fails on its way here leaves it where it was)
    void after_mix(float* d_bus, uint32_t n_frames, hipStream_t s)
    {
        ring.upload_dirty(d_rec.get(), book.h_rec.data(), book.dirty, s);
        BusLimitArgs a{};
        a.raw = d_raw.get(); a.out = d_bus; a.ring = d_ring.get(); a.rec = d_rec.get(); a.meter = d_meter.get();
        a.n_buses = book.n_buses; a.n_frames = n_frames; a.mask = ring_row - 1u; a.pos = book.pos;
        HIP_TRY(launch_bus_limit(a, s));
        book.advance(n_frames);
    }
    // records [first, first + count), behind everything on q (waits); clear: exactly those records are cleared behind the copy
    void read(uint32_t first, uint32_t count, aidax_bus_meter* out, bool clear, hipStream_t q)
    {
        const size_t bytes = sizeof(BusMeterRec) * count;
        read_back(out, h_meter.get() + first, d_meter.get() + first, bytes, q,
                  [&] { if (clear) HIP_TRY(hipMemcpyAsync(d_meter.get() + first, h_meter.get() + book.n_buses + first, bytes, hipMemcpyHostToDevice, q)); });
    }
};

}  // namespace aidax
