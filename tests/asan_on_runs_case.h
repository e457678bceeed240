// One fixed case of the off-to-on rule (OnRuns, aidax_stage_book.h) for the three books that are one: GateBook, TunerBook and DelayBook,
// from tests/asan_gate_harness.cpp, asan_tuner_harness.cpp and asan_delay_harness.cpp. Seven streams. 0, 2, 4 and 6 go on in a call
// each, then one call over [0, 7) switches all on: the runs are {1,2},{3,4},{5,6}. All off, the same pattern again, all off, then 1, 3 and
// 5 go on and one call over [0, 7) switches all on: {0,1},{2,3},{4,5},{6,7}, the (n + 1) / 2 = 4 runs that n streams can hold at once.
// Across all of it `runs` keeps the capacity and the storage it had after init (the audio side allocated nothing) and n_on is the count
// of streams that are on.
#pragma once

#include <cstdint>
#include <cstdio>
#include <vector>

#include "../aidadsp-lv2_amd/csrc/aidax_stage_book.h"

// `b`: the book after its init for 7 streams; set(lo, hi, on): the book's own call for streams [lo, hi), which returns its runs.
// Returns the number of calls that did not do what is expected of them.
template <class Book, class Set>
int on_runs_case(const char* who, Book& b, Set&& set)
{
    using Runs = std::vector<aidax::Run>;
    constexpr uint32_t n = 7;
    const size_t capacity = b.runs.capacity();
    const aidax::Run* const storage = b.runs.data();
    bool on[n] = {};
    int missed = 0, calls = 0;
    auto call = [&](uint32_t lo, uint32_t hi, bool goes_on, const Runs& want) {
        const Runs& got = set(lo, hi, goes_on);
        uint32_t count = 0;
        for (uint32_t s = 0; s < n; ++s) {
            if (s >= lo && s < hi) on[s] = goes_on;
            count += on[s] ? 1u : 0u;
        }
        ++calls;
        if (&got == &b.runs && got == want && b.n_on == count && b.runs.capacity() == capacity && b.runs.data() == storage) return;
        std::fprintf(stderr, "%s: on_runs_case: call %d ([%u, %u) %s) is not what the rule gives\n", who, calls, lo, hi, goes_on ? "on" : "off");
        ++missed;
    };
    if (capacity < (n + 1u) / 2u || storage == nullptr) { std::fprintf(stderr, "%s: on_runs_case: init reserved too little\n", who); ++missed; }
    for (int round = 0; round < 2; ++round) {
        for (uint32_t s = 0; s < n; s += 2) call(s, s + 1, true, { { s, s + 1 } });
        if (round == 0) call(0, n, true, { { 1, 2 }, { 3, 4 }, { 5, 6 } });
        call(0, n, false, {});
    }
    for (uint32_t s = 1; s < n; s += 2) call(s, s + 1, true, { { s, s + 1 } });
    call(0, n, true, { { 0, 1 }, { 2, 3 }, { 4, 5 }, { 6, 7 } });
    call(0, n, true, {});                                                       // (all on already: no run, and n_on stands)
    return missed;
}
