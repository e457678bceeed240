// aidax_stream_stages.h — the two per-stream stages around a pool's pass (include/aidax.h, "Noise gate" and "Stream meters"): the gate
// ahead of the model (k_gate) and the meters on both sides of it (k_meter). GateBook is the gate's host-only half (no HIP call: which
// gates are on, their records, what the device has not seen), GateStage and MeterStage the device halves. Issues HIP calls: include it last.
#pragma once

#include <cstddef>
#include <utility>
#include <vector>

#include "aidax_snapshot_ring.h"

namespace aidax {

static_assert(sizeof(aidax_stream_meter) == sizeof(MeterRec) && offsetof(aidax_stream_meter, out_over) == offsetof(MeterRec, out_over) &&
                  offsetof(aidax_stream_meter, out_energy) == offsetof(MeterRec, out_energy) && offsetof(aidax_stream_meter, out_peak) == offsetof(MeterRec, out_peak),
              "k_meter's record is aidax_stream_meter");
static_assert(sizeof(aidax_gate_rec) == sizeof(GateRec) && offsetof(aidax_gate_rec, hold) == offsetof(GateRec, hold) && offsetof(aidax_gate_rec, on) == offsetof(GateRec, on) &&
                  sizeof(aidax_gate_state) == sizeof(GateState) && offsetof(aidax_gate_state, atten) == offsetof(GateState, atten),
              "k_gate's record and state are aidax_gate_rec and aidax_gate_state");

// The gates' host records, all of them the audio side's. `runs` is sized once (init), so that a change allocates nothing.
struct GateBook {
    using Run = std::pair<uint32_t, uint32_t>;           // streams [first, second)
    std::vector<GateRec> h_rec;
    std::vector<aidax_gate_params> params;               // as last set, kept for the streams whose gate is on
    DirtyRange dirty;                                    // records the device has not seen
    uint32_t n_on = 0;                                   // streams whose gate is on: a pass launches k_gate while this is not 0
    std::vector<Run> runs;

    void init(uint32_t n) { h_rec.assign(n, GateRec{}); params.assign(n, aidax_gate_params{}); runs.reserve((n + 1u) / 2u); }
    // Streams [lo, hi) get the designed record and its parameters, or (designed == nullptr) their gates go off. Returns the maximal runs
    // of streams that went from off to on: they restart at unity gain, so the caller zeroes those runs' states.
    const std::vector<Run>& apply(uint32_t lo, uint32_t hi, const aidax_gate_rec* designed, const aidax_gate_params* set_params)
    {
        runs.clear();
        for (uint32_t s = lo; s < hi; ++s) {
            GateRec& r = h_rec[s];
            if (designed && !r.on) {
                ++n_on;
                if (!runs.empty() && runs.back().second == s) runs.back().second = s + 1;
                else runs.emplace_back(s, s + 1);
            } else if (!designed && r.on) {
                --n_on;
            }
            if (designed) { std::memcpy(&r, designed, sizeof r); params[s] = *set_params; }
            else r.on = 0u;
        }
        dirty.mark(lo, hi - 1);
        return runs;
    }
};

// The device half: nothing until enable(), the set-up side's first call that switches a gate on; from then on the book's records are
// uploaded ahead of the pass that follows a change. HIP failures leave as HipFail.
struct GateStage {
    GateBook book;
    DevBuf<GateRec> d_rec;           // [n_streams], empty: never enabled
    DevBuf<GateState> d_state;       // [n_streams]
    PinnedBuf<GateState> h_state;    // pinned staging of read(), [n_streams]
    DevBuf<float> d_side;            // the gated block a pass's model launch reads: [n_streams][max_frames]
    SnapshotRing ring;

    bool enabled() const { return static_cast<bool>(d_rec); }
    // records, states (zeroed), the side block, the snapshots and the pinned staging of the read; all or nothing
    void enable(uint32_t n_streams, uint32_t max_frames, hipStream_t q)
    {
        const size_t n = n_streams;
        GateStage fresh;
        fresh.d_rec.alloc(n);
        fresh.d_state.alloc(n);
        fresh.d_side.alloc(n * max_frames);
        fresh.h_state.alloc(n);
        HIP_TRY(hipMemsetAsync(fresh.d_rec.get(), 0, sizeof(GateRec) * n, q));
        HIP_TRY(hipMemsetAsync(fresh.d_state.get(), 0, sizeof(GateState) * n, q));
        HIP_TRY(hipStreamSynchronize(q));                // (a pass on a caller's stream must find them zeroed)
        fresh.ring.alloc(sizeof(GateRec) * n);
        fresh.book.init(n_streams);
        *this = std::move(fresh);
    }
    // audio side: host records; the runs that restart are zeroed by clear_states() on the pool's own stream, behind the passes issued so far
    const std::vector<GateBook::Run>& set(uint32_t lo, uint32_t hi, const aidax_gate_rec* designed, const aidax_gate_params* params) { return book.apply(lo, hi, designed, params); }
    void clear_states(uint32_t first, uint32_t count, hipStream_t q) { if (d_state) HIP_TRY(hipMemsetAsync(d_state.get() + first, 0, sizeof(GateState) * count, q)); }
    // Ahead of the model's launch of a pass: the records it plays under, then the gated block into the side block. Returns what that
    // launch reads: the side block, or d_in while no gate is on (the pass's end markers stay with the model's launch: the gate is ahead of it)
    const float* before_pass(const float* d_in, const StreamCtl* d_ctl, uint32_t n_active, uint32_t n_frames, hipStream_t s)
    {
        if (n_frames == 0 || book.n_on == 0) return d_in;
        ring.upload_dirty(d_rec.get(), book.h_rec.data(), book.dirty, s);
        HIP_TRY(launch_gate(d_in, d_side.get(), d_rec.get(), d_state.get(), d_ctl, n_active, n_frames, s));
        return d_side.get();
    }
    void read(uint32_t first, uint32_t count, aidax_gate_state* out, hipStream_t q)      // waits
    {
        read_back(out, h_state.get() + first, d_state.get() + first, sizeof(GateState) * count, q);
    }
};

// The stream meters: nothing until enable(), the set-up side's first call that switches them on; from then on `on` is a host record of
// the audio side. A metered pass is k_meter over the block it was handed, the pass, k_meter over the block it returns.
struct MeterStage {
    DevBuf<MeterRec> d_rec;          // [n_streams], empty: never enabled
    PinnedBuf<MeterRec> h_rec;       // pinned staging of read(), [n_streams]
    bool on = false;

    bool enabled() const { return static_cast<bool>(d_rec); }
    void enable(uint32_t n_streams, hipStream_t q)       // the records, zeroed, and the staging; switches the meters on; all or nothing
    {
        MeterStage fresh;
        fresh.h_rec.alloc(n_streams);
        fresh.d_rec.alloc(n_streams);
        HIP_TRY(hipMemsetAsync(fresh.d_rec.get(), 0, sizeof(MeterRec) * n_streams, q));
        HIP_TRY(hipStreamSynchronize(q));                // (a pass on a caller's stream must find them zeroed)
        fresh.on = true;
        *this = std::move(fresh);
    }
    void launch_in(const float* d_in, uint32_t n_active, uint32_t n_frames, hipStream_t s) { HIP_TRY(launch_meter(d_in, d_rec.get(), n_active, n_frames, kMeterIn, s)); }
    void launch_out(const float* d_out, uint32_t n_active, uint32_t n_frames, hipStream_t s) { HIP_TRY(launch_meter(d_out, d_rec.get(), n_active, n_frames, kMeterOut, s)); }
    void read(uint32_t first, uint32_t count, aidax_stream_meter* out, bool clear, hipStream_t q)      // waits
    {
        const size_t bytes = sizeof(MeterRec) * count;
        read_back(out, h_rec.get() + first, d_rec.get() + first, bytes, q, [&] { if (clear) HIP_TRY(hipMemsetAsync(d_rec.get() + first, 0, bytes, q)); });
    }
};

}  // namespace aidax
