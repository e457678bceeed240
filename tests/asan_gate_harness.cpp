// The noise gate's host half under AddressSanitizer + UndefinedBehaviorSanitizer (`make asan_gate`, tests/test_asan_gate.py): GateBook
// (aidax_stream_stages.h: which gates are on, the records and parameters, the runs of streams that restart, the dirty range) held
// against a direct restatement of its rules over seeded random sets and clears of one stream or of all. CPU only: no device half is built.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <utility>
#include <vector>

#include "aidax.h"
#include "../aidadsp-lv2_amd/csrc/aidax_stream_stages.h"
#include "asan_on_runs_case.h"

namespace aidax {
// (aidax_model.cpp, linked for fail() and aidax_last_error(), asks the pool which models have a kernel: no model is loaded here)
bool model_supported(const aidax_model&) { return true; }
}  // namespace aidax

static int failures = 0, steps = 0;
#define EXPECT(c) do { if (!(c)) { std::fprintf(stderr, "asan_gate_harness: %s failed at line %d (%s)\n", #c, __LINE__, aidax_last_error()); ++failures; } } while (0)

using aidax::GateBook;
using aidax::GateRec;

static uint32_t lcg_state = 88172645u;
static uint32_t rnd(uint32_t n) { lcg_state = lcg_state * 1664525u + 1013904223u; return (lcg_state >> 8) % n; }

static bool same(const aidax_gate_params& a, const aidax_gate_params& b) { return std::memcmp(&a, &b, sizeof a) == 0; }

// parameters of their own at every call, so that a kept record can be told from a replaced one
static aidax_gate_params some_params()
{
    aidax_gate_params p{};
    p.open_db = -10.f - static_cast<float>(rnd(20));
    p.close_db = p.open_db - 1.f - static_cast<float>(rnd(10));
    p.floor_db = -20.f - static_cast<float>(rnd(60));
    p.attack_ms = 0.1f * static_cast<float>(1 + rnd(50));
    p.hold_ms = 1.f * static_cast<float>(rnd(40));
    p.release_ms = 1.f * static_cast<float>(1 + rnd(200));
    return p;
}

static void run(uint32_t n, uint32_t seed, int n_steps)
{
    lcg_state = seed;
    GateBook b;
    b.init(n);
    // what the harness knows: who is on, with which parameters and record; and what the device would hold after the last flush
    std::vector<uint8_t> on(n, 0);
    std::vector<aidax_gate_params> params(n);
    std::vector<GateRec> rec(n, GateRec{}), device(n, GateRec{});
    EXPECT(b.n_on == 0 && b.dirty.empty() && b.h_rec.size() == n && b.params.size() == n);
    for (int step = 0; step < n_steps; ++step, ++steps) {
        const uint32_t op = rnd(8);
        if (op == 7) {                                                          // a flush, as GateStage::before_pass does it while a gate is on
            if (b.n_on != 0 && !b.dirty.empty()) {
                std::copy(b.h_rec.begin() + b.dirty.lo, b.h_rec.begin() + b.dirty.hi + 1, device.begin() + b.dirty.lo);
                b.dirty.clear();
            }
        } else {
            const bool all = rnd(4) == 0, set = rnd(3) != 0;
            const uint32_t lo = all ? 0u : rnd(n), hi = all ? n : lo + 1u;
            aidax_gate_params p = some_params();
            aidax_gate_rec designed{};
            if (set) EXPECT(aidax_gate_design(&p, 48000.0, &designed) == AIDAX_OK && designed.on == 1u);
            // the restatement: the maximal runs of streams in [lo, hi) that are off now and on afterwards
            std::vector<std::pair<uint32_t, uint32_t>> want;
            for (uint32_t s = lo; s < hi; ++s) {
                if (set && !on[s]) {
                    if (!want.empty() && want.back().second == s) want.back().second = s + 1;
                    else want.push_back({ s, s + 1 });
                }
                on[s] = set ? 1 : 0;
                if (set) { params[s] = p; std::memcpy(&rec[s], &designed, sizeof(GateRec)); }
                else rec[s].on = 0u;
            }
            const std::vector<GateBook::Run>& got = b.apply(lo, hi, set ? &designed : nullptr, set ? &p : nullptr);
            EXPECT(got == want);
            EXPECT(!b.dirty.empty() && b.dirty.lo <= lo && hi - 1 <= b.dirty.hi && b.dirty.hi < n);      // dirty covers [lo, hi)
        }
        uint32_t count = 0;
        for (uint32_t s = 0; s < n; ++s) {
            count += on[s];
            EXPECT((b.h_rec[s].on != 0) == (on[s] != 0));
            EXPECT(std::memcmp(&b.h_rec[s], &rec[s], sizeof(GateRec)) == 0);
            if (on[s]) EXPECT(same(b.params[s], params[s]));                    // params is kept for enabled streams
            // what differs from the device's copy lies inside the dirty range
            if (std::memcmp(&b.h_rec[s], &device[s], sizeof(GateRec)) != 0) EXPECT(!b.dirty.empty() && b.dirty.lo <= s && s <= b.dirty.hi);
        }
        EXPECT(b.n_on == count);                                                // n_on equals the count of `on` records
    }
}

// the off-to-on rule's fixed case (asan_on_runs_case.h)
static void the_runs_that_restart()
{
    lcg_state = 5u;
    aidax_gate_params p = some_params();
    aidax_gate_rec designed{};
    EXPECT(aidax_gate_design(&p, 48000.0, &designed) == AIDAX_OK && designed.on == 1u);
    GateBook seven;
    seven.init(7);
    failures += on_runs_case("asan_gate_harness", seven, [&](uint32_t lo, uint32_t hi, bool on) -> const std::vector<GateBook::Run>& {
        return seven.apply(lo, hi, on ? &designed : nullptr, on ? &p : nullptr);
    });
    ++steps;
}

int main()
{
    the_runs_that_restart();
    for (uint32_t n : { 1u, 2u, 7u, 70u })
        for (uint32_t seed : { 1u, 77u, 2024u }) run(n, seed * 2654435761u + n, 400);
    std::printf("asan_gate_harness: %d steps, %d failures\n", steps, failures);
    return failures ? 1 : 0;
}
