// aidax_stream_stages.h — the per-stream stages around a pool's pass (include/aidax.h, "Noise gate", "Stream meters" and "Stream
// tuners"): the gate ahead of the model (k_gate), the meters on both sides of it (k_meter) and the tuners ahead of it (k_tune). GateBook
// is the gate's host-only half (no HIP call: which gates are on, their records, what the device has not seen) and TunerBook
// (aidax_tuner_book.h) the tuners'; GateStage, MeterStage and TunerStage are the device halves. Issues HIP calls: include it last.
#pragma once

#include <cstddef>
#include <utility>
#include <vector>

#include "aidax_snapshot_ring.h"
#include "aidax_tuner_book.h"

namespace aidax {

static_assert(sizeof(aidax_stream_meter) == sizeof(MeterRec) && offsetof(aidax_stream_meter, out_over) == offsetof(MeterRec, out_over) &&
                  offsetof(aidax_stream_meter, out_energy) == offsetof(MeterRec, out_energy) && offsetof(aidax_stream_meter, out_peak) == offsetof(MeterRec, out_peak),
              "k_meter's record is aidax_stream_meter");
static_assert(sizeof(aidax_gate_rec) == sizeof(GateRec) && offsetof(aidax_gate_rec, hold) == offsetof(GateRec, hold) && offsetof(aidax_gate_rec, on) == offsetof(GateRec, on) &&
                  sizeof(aidax_gate_state) == sizeof(GateState) && offsetof(aidax_gate_state, atten) == offsetof(GateState, atten),
              "k_gate's record and state are aidax_gate_rec and aidax_gate_state");

// The gates' host records, all of them the audio side's. n_on: streams whose gate is on; runs: sized once (init).
struct GateBook : OnRuns {
    using Run = aidax::Run;
    std::vector<GateRec> h_rec;
    std::vector<aidax_gate_params> params;               // as last set, kept for the streams whose gate is on
    DirtyRange dirty;                                    // records the device has not seen

    void init(uint32_t n) { h_rec.assign(n, GateRec{}); params.assign(n, aidax_gate_params{}); reserve(n); }
    // Streams [lo, hi) get the designed record and its parameters, or (designed == nullptr) their gates go off. Returns the maximal runs
    // of streams that went from off to on: they restart at unity gain, so the caller zeroes those runs' states.
    const std::vector<Run>& apply(uint32_t lo, uint32_t hi, const aidax_gate_rec* designed, const aidax_gate_params* set_params)
    {
        begin_change();
        for (uint32_t s = lo; s < hi; ++s) {
            GateRec& r = h_rec[s];
            note(s, r.on != 0u, designed != nullptr);
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
        fresh.d_rec.zero(0, n, q);
        fresh.d_state.zero(0, n, q);
        HIP_TRY(hipStreamSynchronize(q));                // (a pass on a caller's stream must find them zeroed)
        fresh.ring.alloc(sizeof(GateRec) * n);
        fresh.book.init(n_streams);
        *this = std::move(fresh);
    }
    // audio side: host records; the runs that restart are zeroed by clear_states() on the pool's own stream, behind the passes issued so far
    const std::vector<GateBook::Run>& set(uint32_t lo, uint32_t hi, const aidax_gate_rec* designed, const aidax_gate_params* params) { return book.apply(lo, hi, designed, params); }
    void clear_states(uint32_t first, uint32_t count, hipStream_t q) { if (d_state) d_state.zero(first, count, q); }
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
        fresh.d_rec.zero(0, n_streams, q);
        HIP_TRY(hipStreamSynchronize(q));                // (a pass on a caller's stream must find them zeroed)
        fresh.on = true;
        *this = std::move(fresh);
    }
    void launch_in(const float* d_in, uint32_t n_active, uint32_t n_frames, hipStream_t s) { HIP_TRY(launch_meter(d_in, d_rec.get(), n_active, n_frames, kMeterIn, s)); }
    void launch_out(const float* d_out, uint32_t n_active, uint32_t n_frames, hipStream_t s) { HIP_TRY(launch_meter(d_out, d_rec.get(), n_active, n_frames, kMeterOut, s)); }
    void read(uint32_t first, uint32_t count, aidax_stream_meter* out, bool clear, hipStream_t q)      // waits
    {
        const size_t bytes = sizeof(MeterRec) * count;
        read_back(out, h_rec.get() + first, d_rec.get() + first, bytes, q, [&] { if (clear) d_rec.zero(first, count, q); });
    }
};

// The stream tuners: nothing until enable(), the set-up side's first aidax_pool_set_tuning with parameters; from then on `on` and the
// book's records are the audio side's. A tuned pass is k_tune over the block it was handed, ahead of the model's launch.
static_assert(sizeof(aidax_tuner_reading) == sizeof(TunerReading) && offsetof(aidax_tuner_reading, analyses) == offsetof(TunerReading, analyses) &&
                  offsetof(aidax_tuner_reading, hz) == offsetof(TunerReading, hz) && offsetof(aidax_tuner_reading, level) == offsetof(TunerReading, level),
              "k_tune's reading is aidax_tuner_reading");
struct TunerStage {
    TunerBook book;
    DevBuf<float> d_ring;            // [n_streams][ring_row], empty: never enabled
    DevBuf<uint64_t> d_pos;          // [n_streams]
    DevBuf<uint32_t> d_on;           // [n_streams]
    DevBuf<TunerReading> d_reading;  // [n_streams]
    DevBuf<float> d_curve;           // [n_streams][curve_row]
    PinnedBuf<TunerReading> h_reading;   // pinned staging of read(), [n_streams]
    PinnedBuf<float> h_curve;        // ... and of read_curve(), [curve_row]
    SnapshotRing ring;
    uint32_t ring_row = 0, curve_row = 0;
    bool on = false;

    bool enabled() const { return static_cast<bool>(d_ring); }
    // rings, counts, `on` words, readings and curves (all zeroed), the snapshots and the pinned staging; switches the stage on; all or nothing
    void enable(uint32_t n_streams, uint32_t max_frames, const aidax_tuner_rec& designed, hipStream_t q)
    {
        const size_t n = n_streams;
        TunerStage fresh;
        fresh.ring_row = pow2_at_least(designed.window + max_frames);
        fresh.curve_row = designed.tmax + 2u;
        fresh.d_ring.alloc(n * fresh.ring_row);
        fresh.d_pos.alloc(n);
        fresh.d_on.alloc(n);
        fresh.d_reading.alloc(n);
        fresh.d_curve.alloc(n * fresh.curve_row);
        fresh.h_reading.alloc(n);
        fresh.h_curve.alloc(fresh.curve_row);
        fresh.d_ring.zero(0, n * fresh.ring_row, q);
        fresh.d_pos.zero(0, n, q);
        fresh.d_on.zero(0, n, q);
        fresh.d_reading.zero(0, n, q);
        fresh.d_curve.zero(0, n * fresh.curve_row, q);
        HIP_TRY(hipStreamSynchronize(q));                // (a pass on a caller's stream must find them zeroed)
        fresh.ring.alloc(sizeof(uint32_t) * n);
        fresh.book.init(n_streams, designed);
        fresh.on = true;
        *this = std::move(fresh);
    }
    // a restart's device half, on the pool's own stream behind the passes issued so far: count, reading and curve (the ring needs no
    // clear: a window never reaches behind the restart, rule 1 asks for b >= window)
    void clear_streams(uint32_t first, uint32_t count, hipStream_t q)
    {
        if (!d_ring) return;
        d_pos.zero(first, count, q);
        d_reading.zero(first, count, q);
        d_curve.zero(static_cast<size_t>(first) * curve_row, static_cast<size_t>(count) * curve_row, q);
    }
    // Ahead of the model's launch of a pass: the `on` words it plays under, then k_tune over the block it was handed
    void before_pass(const float* d_in, uint32_t n_active, uint32_t n_frames, hipStream_t s)
    {
        if (!on || n_frames == 0 || book.n_on == 0) return;
        ring.upload_dirty(d_on.get(), book.h_on.data(), book.dirty, s);
        const bool analyse = book.advance(n_active, n_frames);
        const aidax_tuner_rec& r = book.rec;
        TuneArgs a{};
        a.in = d_in; a.ring = d_ring.get(); a.pos = d_pos.get(); a.on = d_on.get(); a.reading = d_reading.get(); a.curve = d_curve.get();
        a.samplerate = r.samplerate;
        a.n_active = n_active; a.n_frames = n_frames; a.mask = ring_row - 1u; a.curve_row = curve_row;
        a.window = r.window; a.hop = r.hop; a.tmin = r.tmin; a.tmax = r.tmax;
        a.threshold = r.threshold; a.clarity_min = r.clarity_min; a.level_min = r.level_min;
        HIP_TRY(launch_tune(a, analyse, s));
    }
    void read(uint32_t first, uint32_t count, aidax_tuner_reading* out, hipStream_t q)      // waits
    {
        read_back(out, h_reading.get() + first, d_reading.get() + first, sizeof(TunerReading) * count, q);
    }
    void read_curve(uint32_t stream, float* out, uint32_t count, hipStream_t q)             // waits
    {
        read_back(out, h_curve.get(), d_curve.get() + static_cast<size_t>(stream) * curve_row, sizeof(float) * count, q);
    }
};

}  // namespace aidax
