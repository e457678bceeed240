// aidax_delay_book.h — the stream delays' host-only half (include/aidax.h, "Stream delays"): DelayBook. No HIP call and no HIP header:
// the capacity and what fits it, the streams' records and their parameters as last set, which delays are on, the records the device has
// not seen and the runs of streams that restart. tests/asan_delay_harness.cpp holds it against a restatement under the sanitizers.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <utility>
#include <vector>

#include "../../include/aidax.h"
#include "aidax_stage_book.h"

namespace aidax {

struct DelayBook : OnRuns {                              // n_on: streams whose delay is on; runs: sized once (init)
    using Run = aidax::Run;
    uint32_t cap = 0;                                    // the capacity in frames, fixed by init
    std::vector<aidax_delay_rec> h_rec;                  // the records k_delay reads
    std::vector<aidax_delay_params> params;              // as last set by parameters; zeros for a stream set by a record of the caller's own
    DirtyRange dirty;                                    // records the device has not seen

    void init(uint32_t n, uint32_t capacity)
    {
        cap = capacity;
        h_rec.assign(n, aidax_delay_rec{});
        params.assign(n, aidax_delay_params{});
        reserve(n);
        dirty.clear(); n_on = 0;
    }
    // floats of a stream's ring row: the smallest power of two that holds the longest history a record within the capacity reads
    // (cap + 3 frames: the frame itself and the three taps behind the longest read position) next to a pass of max_frames
    static uint32_t ring_row(uint32_t capacity, uint32_t max_frames)
    {
        uint32_t row = 1;
        while (row < capacity + 3u + max_frames) row <<= 1;
        return row;
    }
    // the record's own conditions (include/aidax.h), whatever the capacity; `on` is the book's and is not read
    static bool valid(const aidax_delay_rec& r)
    {
        auto level = [](float v) { return std::isfinite(v) && std::fabs(v) <= 4.f; };
        return r.m >= AIDAX_DELAY_MIN && r.m <= AIDAX_DELAY_MAX && r.depth_q16 <= (static_cast<uint32_t>(AIDAX_DELAY_MAX_DEPTH) << 16) && r.fade <= AIDAX_DELAY_MAX_FADE &&
               std::fabs(r.fb) <= 0.98f && r.damp >= 0.f && r.damp <= 0.5f && level(r.wet) && level(r.dry);      // (false for a NaN)
    }
    // m + ceil(depth) <= cap: the longest read position of the record lies inside the line
    bool fits(const aidax_delay_rec& r) const
    {
        const uint64_t reach = static_cast<uint64_t>(r.m) + ((static_cast<uint64_t>(r.depth_q16) + 0xffffu) >> 16);
        return reach <= cap;
    }
    // Streams [lo, hi) get the record and, where it was designed from parameters, those (set_params == nullptr: a record of the caller's
    // own), or (rec == nullptr) their delays go off. Returns the maximal runs of streams that went from off to on: their lines restart,
    // so the caller zeroes those runs' states. *ok = false, and nothing changed: a record beyond the capacity.
    const std::vector<Run>& set(uint32_t lo, uint32_t hi, const aidax_delay_rec* rec, const aidax_delay_params* set_params, bool* ok)
    {
        begin_change();
        *ok = !rec || fits(*rec);
        if (!*ok) return runs;
        for (uint32_t s = lo; s < hi; ++s) {
            aidax_delay_rec& h = h_rec[s];
            note(s, h.on != 0u, rec != nullptr);
            if (rec) {
                h = *rec;
                h.on = 1u;
                h.reserved[0] = h.reserved[1] = h.reserved[2] = 0u;
                params[s] = set_params ? *set_params : aidax_delay_params{};
            } else {
                h.on = 0u;
            }
        }
        dirty.mark(lo, hi - 1);
        return runs;
    }
};

}  // namespace aidax
