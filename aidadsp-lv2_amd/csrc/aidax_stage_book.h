// aidax_stage_book.h — what the stages' host-only halves (GateBook, TunerBook, DelayBook, LimitBook, ReverbBook, ModelBank, the pool's
// control records) share. No HIP call and no HIP header: the range of records the device has not seen (DirtyRange; SnapshotRing::upload_dirty
// sends it) and the rule of the streams that restart when a stage of theirs goes from off to on (OnRuns). The sanitizer harnesses of the
// gate, the tuners and the delays hold the rule against a restatement.
#pragma once

#include <algorithm>
#include <cstdint>
#include <utility>
#include <vector>

namespace aidax {

struct DirtyRange {                                      // records [lo, hi] to upload; empty when lo > hi
    uint32_t lo = 1, hi = 0;
    bool empty() const { return lo > hi; }
    void clear() { lo = 1; hi = 0; }
    void mark(uint32_t l, uint32_t h) { const bool e = empty(); lo = e ? l : std::min(lo, l); hi = e ? h : std::max(hi, h); }
};

using Run = std::pair<uint32_t, uint32_t>;               // streams [first, second)

// Which streams of a per-stream stage are on, as a count, and the maximal runs of streams that one change took from off to on: they
// restart, so the caller zeroes those runs' device state. A book is one of these (its n_on and runs are the book's). `runs` is sized
// once (reserve: n streams hold at most (n + 1) / 2 runs at once), so that a change, which is the audio side's, allocates nothing.
struct OnRuns {
    uint32_t n_on = 0;                                   // a pass launches the stage's kernel while this is not 0
    std::vector<Run> runs;

    void reserve(uint32_t n) { runs.reserve((n + 1u) / 2u); }
    void begin_change() { runs.clear(); }
    // stream s of the change, in rising order; true: it went from off to on
    bool note(uint32_t s, bool was_on, bool goes_on)
    {
        if (goes_on && !was_on) {
            ++n_on;
            if (!runs.empty() && runs.back().second == s) runs.back().second = s + 1;
            else runs.emplace_back(s, s + 1);
            return true;
        }
        if (!goes_on && was_on) --n_on;
        return false;
    }
};

}  // namespace aidax
