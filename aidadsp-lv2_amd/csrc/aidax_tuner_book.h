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

namespace aidax {

struct TunerBook {
    using Run = std::pair<uint32_t, uint32_t>;           // streams [first, second)
    aidax_tuner_rec rec{};                               // the design, fixed by init
    std::vector<uint32_t> h_on;                          // the words k_tune reads
    std::vector<uint64_t> pos;                           // frames handed to the stream since its tuner went on or was restarted
    uint32_t dirty_lo = 1, dirty_hi = 0;                 // `on` words [lo, hi] the device has not seen; empty when lo > hi
    uint32_t n_on = 0;                                   // streams whose tuner is on: a pass launches k_tune while this is not 0
    std::vector<Run> runs;                               // sized once (init), so that a change allocates nothing

    void init(uint32_t n, const aidax_tuner_rec& designed)
    {
        rec = designed;
        h_on.assign(n, 0u);
        pos.assign(n, 0u);
        runs.reserve((n + 1u) / 2u);
        dirty_lo = 1; dirty_hi = 0; n_on = 0;
    }
    bool dirty() const { return dirty_lo <= dirty_hi; }
    void mark(uint32_t lo, uint32_t hi)
    {
        const bool e = !dirty();
        dirty_lo = e ? lo : std::min(dirty_lo, lo);
        dirty_hi = e ? hi : std::max(dirty_hi, hi);
    }
    void flushed() { dirty_lo = 1; dirty_hi = 0; }
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
        runs.clear();
        bool changed = false;
        for (uint32_t s = lo; s < hi; ++s) {
            if (on && !h_on[s]) {
                ++n_on;
                pos[s] = 0;
                if (!runs.empty() && runs.back().second == s) runs.back().second = s + 1;
                else runs.emplace_back(s, s + 1);
            } else if (!on && h_on[s]) {
                --n_on;
            }
            changed = changed || (h_on[s] != 0u) != on;
            h_on[s] = on ? 1u : 0u;
        }
        if (changed) mark(lo, hi - 1);
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
