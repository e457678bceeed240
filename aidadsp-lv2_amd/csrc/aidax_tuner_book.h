// aidax_tuner_book.h — the stream tuners' host-only half (include/aidax.h, "Stream tuners"): TunerBook. No HIP call and no HIP header:
// which tuners are on, the mirror of every stream's frame count (the device keeps its own: k_tune decides per stream; the mirror tells
// whether ANY stream of a pass crosses a hop boundary, which picks the launch's form), the `on` words the device has not seen and the
// runs of streams that restart. tests/asan_tuner_harness.cpp holds it against a restatement under the sanitizers.
#pragma once

#include <algorithm>
#include <cstdint>
#include <utility>
#include <vector>

#include "../../include/aidax.h"
#include "aidax_stage_book.h"

namespace aidax {

struct TunerBook : OnRuns {                              // n_on: streams whose tuner is on; runs: sized once (init)
    using Run = aidax::Run;
    aidax_tuner_rec rec{};                               // the design, fixed by init
    std::vector<uint32_t> h_on;                          // the words k_tune reads
    std::vector<uint64_t> pos;                           // frames handed to the stream since its tuner went on or was restarted
    DirtyRange dirty;                                    // `on` words the device has not seen

    void init(uint32_t n, const aidax_tuner_rec& designed)
    {
        rec = designed;
        h_on.assign(n, 0u);
        pos.assign(n, 0u);
        reserve(n);
        dirty.clear(); n_on = 0;
    }
    // Rule 1: does a pass that takes a count from p0 to p1 analyse, and at which boundary
    static bool crosses(uint64_t p0, uint64_t p1, uint32_t window, uint32_t hop, uint64_t* boundary)
    {
        const uint64_t b = (p1 / hop) * hop;
        if (boundary) *boundary = b;
        return b > p0 && b >= window;
    }
    // Streams [lo, hi) go on or off. Returns the maximal runs of streams that went from off to on: they restart (their counts are
    // zeroed here, the caller zeroes those runs' device records).
    const std::vector<Run>& apply(uint32_t lo, uint32_t hi, bool on)
    {
        begin_change();
        bool changed = false;
        for (uint32_t s = lo; s < hi; ++s) {
            const bool was_on = h_on[s] != 0u;
            if (note(s, was_on, on)) pos[s] = 0;
            changed = changed || was_on != on;
            h_on[s] = on ? 1u : 0u;
        }
        if (changed) dirty.mark(lo, hi - 1);             // (only when a word changed: a call that changes none uploads nothing)
        return runs;
    }
    void restart(uint32_t s) { pos[s] = 0; }             // aidax_pool_reset_stream (the caller zeroes the stream's device records)
    // A pass of n_frames over the first n_active streams: the counts of the tuned ones move; true when at least one of them analyses
    bool advance(uint32_t n_active, uint32_t n_frames)
    {
        bool any = false;
        if (n_frames == 0) return false;
        for (uint32_t s = 0; s < n_active; ++s) {
            if (!h_on[s]) continue;
            const uint64_t p0 = pos[s], p1 = p0 + n_frames;
            any = crosses(p0, p1, rec.window, rec.hop, nullptr) || any;
            pos[s] = p1;
        }
        return any;
    }
};

}  // namespace aidax
