// The stream tuners' host half under AddressSanitizer + UndefinedBehaviorSanitizer (`make asan_tuner`, tests/test_asan_tuner.py):
// TunerBook (aidax_tuner_book.h — a header without HIP: which tuners are on, the mirror of every stream's frame count, the "does this
// pass analyse" decision, the dirty range of `on` words and the runs of streams that restart) held against a direct restatement of the
// count and of the boundary rule over seeded random on / off / reset / pass sequences. CPU only: no device half is built.
#include <cstdint>
#include <cstdio>
#include <utility>
#include <vector>

#include "aidax.h"
#include "../aidadsp-lv2_amd/csrc/aidax_tuner_book.h"
#include "asan_on_runs_case.h"

static int failures = 0, steps = 0;
#define EXPECT(c) do { if (!(c)) { std::fprintf(stderr, "asan_tuner_harness: %s failed at line %d\n", #c, __LINE__); ++failures; } } while (0)

using aidax::TunerBook;

static uint32_t lcg_state = 88172645u;
static uint32_t rnd(uint32_t n) { lcg_state = lcg_state * 1664525u + 1013904223u; return (lcg_state >> 8) % n; }

// the boundary rule, the slow way: is there a multiple of `hop` in (p0, p1] that is at least `window`; the last one
static bool crosses_slowly(uint64_t p0, uint64_t p1, uint32_t window, uint32_t hop, uint64_t* last)
{
    bool any = false;
    for (uint64_t f = p0 + 1; f <= p1; ++f)
        if (f % hop == 0 && f >= window) { any = true; *last = f; }
    return any;
}

static void run(uint32_t n, uint32_t seed, int n_steps, uint32_t window, uint32_t hop, uint32_t max_frames)
{
    lcg_state = seed;
    aidax_tuner_rec rec{};
    rec.window = window; rec.hop = hop; rec.tmin = 2; rec.tmax = window / 2 - 1;
    TunerBook b;
    b.init(n, rec);
    // what the harness knows: who is on, every count, and the `on` words the device would hold after the last flush
    std::vector<uint8_t> on(n, 0);
    std::vector<uint64_t> pos(n, 0);
    std::vector<uint32_t> device(n, 0u);
    EXPECT(b.n_on == 0 && b.dirty.empty() && b.h_on.size() == n && b.pos.size() == n && b.runs.capacity() >= (n + 1u) / 2u);
    const size_t runs_capacity = b.runs.capacity();
    for (int step = 0; step < n_steps; ++step, ++steps) {
        const uint32_t op = rnd(10);
        if (op < 3) {                                                           // aidax_pool_set_tuner: one stream or all, on or off
            const bool all = rnd(4) == 0, set = rnd(3) != 0;
            const uint32_t lo = all ? 0u : rnd(n), hi = all ? n : lo + 1u;
            const aidax::DirtyRange dirty_before = b.dirty;
            const std::vector<TunerBook::Run>& runs = b.apply(lo, hi, set);
            // the runs: maximal, ascending, exactly the streams that were off and are on now
            std::vector<uint8_t> restarted(n, 0);
            uint32_t prev_end = 0;
            bool first = true;
            for (const TunerBook::Run& r : runs) {
                EXPECT(r.first < r.second && r.second <= hi && r.first >= lo);
                EXPECT(first || r.first > prev_end);                            // (maximal: two runs never touch)
                for (uint32_t s = r.first; s < r.second && s < n; ++s) restarted[s] = 1;
                prev_end = r.second; first = false;
            }
            bool changed = false;
            for (uint32_t s = lo; s < hi; ++s) {
                EXPECT((restarted[s] != 0) == (set && !on[s]));
                changed = changed || (on[s] != 0) != set;
                if (set && !on[s]) pos[s] = 0;
                on[s] = set ? 1 : 0;
            }
            for (uint32_t s = 0; s < n; ++s)
                if (s < lo || s >= hi) EXPECT(!restarted[s]);
            if (changed) EXPECT(!b.dirty.empty() && b.dirty.lo <= lo && b.dirty.hi >= hi - 1u);
            else EXPECT(b.dirty.lo == dirty_before.lo && b.dirty.hi == dirty_before.hi);      // (no word changed: nothing more to upload)
            EXPECT(b.runs.capacity() == runs_capacity);                         // (a change allocates nothing)
        } else if (op == 3) {                                                   // aidax_pool_reset_stream
            const uint32_t s = rnd(n);
            b.restart(s);
            pos[s] = 0;
        } else if (op == 4) {                                                   // a flush, as TunerStage::before_pass does it
            if (!b.dirty.empty()) {
                EXPECT(b.dirty.hi < n);
                for (uint32_t s = b.dirty.lo; s <= b.dirty.hi && s < n; ++s) device[s] = b.h_on[s];
                b.dirty.clear();
            }
            for (uint32_t s = 0; s < n; ++s) EXPECT(device[s] == (on[s] ? 1u : 0u));
        } else {                                                                // a pass over a prefix, or over the whole pool
            const uint32_t n_active = rnd(3) == 0 ? 1u + rnd(n) : n;
            const uint32_t n_frames = rnd(8) == 0 ? 0u : 1u + rnd(max_frames);
            bool want = false;
            for (uint32_t s = 0; s < n_active; ++s) {
                if (!on[s]) continue;
                uint64_t last = 0, got = 0;
                const bool w = crosses_slowly(pos[s], pos[s] + n_frames, window, hop, &last);
                EXPECT(TunerBook::crosses(pos[s], pos[s] + n_frames, window, hop, &got) == w);
                if (w) EXPECT(got == last);
                want = want || w;
                pos[s] += n_frames;
            }
            EXPECT(b.advance(n_active, n_frames) == want);
        }
        uint32_t n_on = 0;
        for (uint32_t s = 0; s < n; ++s) {
            n_on += on[s] ? 1u : 0u;
            EXPECT(b.h_on[s] == (on[s] ? 1u : 0u) && b.pos[s] == pos[s]);      // (the streams behind a prefix and the ones that are off stand)
        }
        EXPECT(b.n_on == n_on);
    }
}

int main()
{
    const uint32_t pools[] = { 1u, 2u, 7u, 70u };
    uint32_t seed = 1234567u;
    for (const uint32_t n : pools) {
        run(n, seed++, 600, 1024u, 64u, 300u);                                  // a hop shorter than most blocks: several boundaries in a pass
        run(n, seed++, 600, 2048u, 1024u, 256u);
        run(n, seed++, 400, 4096u, 65536u, 4096u);
    }
    {                                                                           // the off-to-on rule's fixed case (asan_on_runs_case.h)
        aidax_tuner_rec rec{};
        rec.window = 1024u; rec.hop = 64u; rec.tmin = 2; rec.tmax = 511;
        TunerBook seven;
        seven.init(7, rec);
        failures += on_runs_case("asan_tuner_harness", seven, [&](uint32_t lo, uint32_t hi, bool on) -> const std::vector<TunerBook::Run>& { return seven.apply(lo, hi, on); });
        ++steps;
    }
    // counts beyond 2^32 frames: the rule is 64-bit arithmetic
    uint64_t b = 0;
    EXPECT(TunerBook::crosses((1ull << 32) - 10u, (1ull << 32) + 10u, 1024u, 1024u, &b) && b == (1ull << 32));
    EXPECT(!TunerBook::crosses((1ull << 32) + 10u, (1ull << 32) + 20u, 1024u, 1024u, &b) && b == (1ull << 32));
    std::printf("asan_tuner_harness: %d steps, %d failures\n", steps, failures);
    return failures ? 1 : 0;
}
