// aidax_delay_stage.h — the stream delays behind the cabinet IR stage (include/aidax.h, "Stream delays"): DelayStage, the device half
// around k_delay (aidax_delay.hip); DelayBook (aidax_delay_book.h, no HIP) is the host-only half. Issues HIP calls: include it last.
#pragma once

#include <cstddef>
#include <utility>

#include "aidax_delay_book.h"
#include "aidax_snapshot_ring.h"

namespace aidax {

static_assert(sizeof(aidax_delay_rec) == sizeof(DelayRec) && offsetof(aidax_delay_rec, fade) == offsetof(DelayRec, fade) && offsetof(aidax_delay_rec, fb) == offsetof(DelayRec, fb) &&
                  offsetof(aidax_delay_rec, dry) == offsetof(DelayRec, dry) && offsetof(aidax_delay_rec, on) == offsetof(DelayRec, on) &&
                  sizeof(aidax_delay_state) == sizeof(DelayState) && offsetof(aidax_delay_state, m_cur) == offsetof(DelayState, m_cur) &&
                  offsetof(aidax_delay_state, fade_left) == offsetof(DelayState, fade_left) && offsetof(aidax_delay_state, replaced) == offsetof(DelayState, replaced),
              "k_delay's record and state are aidax_delay_rec and aidax_delay_state");
static_assert(AIDAX_DELAY_MIN == kDelayMin && AIDAX_DELAY_MAX == kDelayMax && AIDAX_DELAY_MAX_DEPTH == kDelayMaxDepth && AIDAX_DELAY_MAX_FADE == kDelayMaxFade,
              "the header's bounds are the kernel's");

// The device half: nothing until enable(), the set-up side's first aidax_pool_set_delays with on != 0; from then on `on` is a host record
// of the audio side. While it is set and a delay is on, k_delay of a pass works in place on the block the pass returns. HIP failures
// leave as HipFail.
struct DelayStage {
    DelayBook book;
    DevBuf<float> d_ring;            // [n_streams][ring_row]: every line's memory; empty: never enabled
    DevBuf<DelayRec> d_rec;          // [n_streams]
    DevBuf<DelayState> d_state;      // [n_streams]
    PinnedBuf<DelayState> h_state;   // pinned staging of read(), [n_streams]
    SnapshotRing ring;
    uint32_t ring_row = 0;
    bool on = false;

    bool enabled() const { return static_cast<bool>(d_ring); }
    bool plays() const { return on && book.n_on != 0; }
    // the rings (not cleared: a line reads 0 before its frame 0, whatever the slot holds), the records (all off), the states (zeroed),
    // the snapshots and the pinned staging of the read; all or nothing
    void enable(uint32_t n_streams, uint32_t max_frames, uint32_t capacity, hipStream_t q)
    {
        const size_t n = n_streams;
        DelayStage fresh;
        fresh.ring_row = DelayBook::ring_row(capacity, max_frames);
        fresh.d_ring.alloc(n * fresh.ring_row);
        fresh.d_rec.alloc(n);
        fresh.d_state.alloc(n);
        fresh.h_state.alloc(n);
        fresh.d_rec.zero(0, n, q);
        fresh.d_state.zero(0, n, q);
        HIP_TRY(hipStreamSynchronize(q));                // (a pass on a caller's stream must find them zeroed)
        fresh.ring.alloc(sizeof(DelayRec) * n);
        fresh.book.init(n_streams, capacity);
        fresh.on = true;
        *this = std::move(fresh);
    }
    // a restart's device half, on the pool's own stream behind the passes issued so far
    void clear_states(uint32_t first, uint32_t count, hipStream_t q) { if (d_state) d_state.zero(first, count, q); }
    // Behind the IR stage of a pass of n_frames > 0 that returns `d_out`: the records, if one has changed since the last upload, then
    // k_delay in place
    void after_pass(float* d_out, const StreamCtl* d_ctl, uint32_t n_active, uint32_t n_frames, hipStream_t s)
    {
        if (n_frames == 0 || !plays()) return;
        ring.upload_dirty(d_rec.get(), book.h_rec.data(), book.dirty, s);
        DelayArgs a{};
        a.block = d_out; a.ring = d_ring.get(); a.rec = d_rec.get(); a.state = d_state.get(); a.ctl = d_ctl;
        a.n_active = n_active; a.n_frames = n_frames; a.mask = ring_row - 1u; a.cap = book.cap;
        HIP_TRY(launch_delay(a, s));
    }
    void read(uint32_t first, uint32_t count, aidax_delay_state* out, hipStream_t q)      // waits
    {
        read_back(out, h_state.get() + first, d_state.get() + first, sizeof(DelayState) * count, q);
    }
};

}  // namespace aidax
