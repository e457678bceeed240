// The stream delays' host half under AddressSanitizer + UndefinedBehaviorSanitizer (`make asan_delay`, tests/test_asan_delay.py):
// DelayBook (aidax_delay_book.h: the capacity and what fits it, the records and parameters, which delays are on, the runs of streams that
// restart, the dirty range) held against a direct restatement of its rules over seeded random sets by parameters and by records, offs,
// records beyond the capacity and flushes, of one stream or of all. CPU only: the header has no device half.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <utility>
#include <vector>

#include "aidax.h"
#include "../aidadsp-lv2_amd/csrc/aidax_delay_book.h"
#include "asan_on_runs_case.h"

static int failures = 0, steps = 0;
#define EXPECT(c) do { if (!(c)) { std::fprintf(stderr, "asan_delay_harness: %s failed at line %d\n", #c, __LINE__); ++failures; } } while (0)

using aidax::DelayBook;

static uint32_t lcg_state = 88172645u;
static uint32_t rnd(uint32_t n) { lcg_state = lcg_state * 1664525u + 1013904223u; return (lcg_state >> 8) % n; }

static bool same(const aidax_delay_params& a, const aidax_delay_params& b) { return std::memcmp(&a, &b, sizeof a) == 0; }
static bool same(const aidax_delay_rec& a, const aidax_delay_rec& b) { return std::memcmp(&a, &b, sizeof a) == 0; }

// a record of its own at every call, so that a kept record can be told from a replaced one; its reach lies on both sides of `cap`
static aidax_delay_rec some_rec(uint32_t cap, aidax_delay_params* p)
{
    aidax_delay_rec r{};
    r.m = AIDAX_DELAY_MIN + rnd(cap + 8u - AIDAX_DELAY_MIN);
    r.depth_q16 = rnd(3) == 0 ? 0u : rnd(40u << 16);
    r.lfo_step = rnd(1u << 20);
    r.fade = rnd(5000);
    r.fb = 0.98f - 0.01f * static_cast<float>(rnd(190));
    r.damp = 0.01f * static_cast<float>(rnd(51));
    r.wet = 0.1f * static_cast<float>(rnd(40));
    r.dry = 1.f;
    r.on = rnd(2);                                                              // (the book ignores it)
    r.reserved[1] = rnd(2) ? 0xdeadbeefu : 0u;                                  // (... and clears these)
    *p = aidax_delay_params{};
    p->time_ms = static_cast<float>(r.m);
    p->feedback = r.fb;
    return r;
}

static void run(uint32_t n, uint32_t cap, uint32_t seed, int n_steps)
{
    lcg_state = seed;
    DelayBook b;
    b.init(n, cap);
    // what the harness knows: who is on, with which parameters and record; and what the device would hold after the last flush
    std::vector<uint8_t> on(n, 0);
    std::vector<aidax_delay_params> params(n);
    std::vector<aidax_delay_rec> rec(n, aidax_delay_rec{}), device(n, aidax_delay_rec{});
    EXPECT(b.n_on == 0 && b.dirty.empty() && b.h_rec.size() == n && b.params.size() == n && b.cap == cap);
    EXPECT(DelayBook::ring_row(cap, 257) >= cap + 3u + 257u && DelayBook::ring_row(cap, 257) / 2u < cap + 3u + 257u);
    for (int step = 0; step < n_steps; ++step, ++steps) {
        const uint32_t op = rnd(8);
        if (op == 7) {                                                          // a flush, as DelayStage::after_pass does it while a delay is on
            if (b.n_on != 0 && !b.dirty.empty()) {
                std::copy(b.h_rec.begin() + b.dirty.lo, b.h_rec.begin() + b.dirty.hi + 1, device.begin() + b.dirty.lo);
                b.dirty.clear();
            }
        } else {
            const bool all = rnd(4) == 0, set = rnd(3) != 0, by_params = rnd(2) != 0;
            const uint32_t lo = all ? 0u : rnd(n), hi = all ? n : lo + 1u;
            aidax_delay_params p{};
            aidax_delay_rec r = some_rec(cap, &p);
            EXPECT(DelayBook::valid(r));
            // the restatement: does the record's reach fit, and the maximal runs of streams in [lo, hi) that are off now and on afterwards
            const uint64_t reach = static_cast<uint64_t>(r.m) + (r.depth_q16 >> 16) + ((r.depth_q16 & 0xffffu) ? 1u : 0u);
            const bool fits = !set || reach <= cap;
            const std::vector<aidax_delay_rec> before = b.h_rec;
            const uint32_t dirty_lo = b.dirty.lo, dirty_hi = b.dirty.hi, n_on = b.n_on;
            std::vector<std::pair<uint32_t, uint32_t>> want;
            if (fits)
                for (uint32_t s = lo; s < hi; ++s) {
                    if (set && !on[s]) {
                        if (!want.empty() && want.back().second == s) want.back().second = s + 1;
                        else want.push_back({ s, s + 1 });
                    }
                    on[s] = set ? 1 : 0;
                    if (set) {
                        params[s] = by_params ? p : aidax_delay_params{};
                        rec[s] = r;
                        rec[s].on = 1u;
                        rec[s].reserved[0] = rec[s].reserved[1] = rec[s].reserved[2] = 0u;
                    } else {
                        rec[s].on = 0u;
                    }
                }
            bool ok = !fits;
            const std::vector<DelayBook::Run>& got = b.set(lo, hi, set ? &r : nullptr, set && by_params ? &p : nullptr, &ok);
            EXPECT(ok == fits && got == want);
            if (fits) {
                EXPECT(!b.dirty.empty() && b.dirty.lo <= lo && hi - 1 <= b.dirty.hi && b.dirty.hi < n);      // dirty covers [lo, hi)
            } else {                                                            // a refused record changes nothing
                EXPECT(b.dirty.lo == dirty_lo && b.dirty.hi == dirty_hi && b.n_on == n_on);
                for (uint32_t s = 0; s < n; ++s) EXPECT(same(b.h_rec[s], before[s]));
            }
        }
        uint32_t count = 0;
        for (uint32_t s = 0; s < n; ++s) {
            count += on[s];
            EXPECT((b.h_rec[s].on != 0) == (on[s] != 0));
            EXPECT(same(b.h_rec[s], rec[s]));
            if (on[s]) EXPECT(same(b.params[s], params[s]) && b.fits(b.h_rec[s]));
            // what differs from the device's copy lies inside the dirty range
            if (!same(b.h_rec[s], device[s])) EXPECT(!b.dirty.empty() && b.dirty.lo <= s && s <= b.dirty.hi);
        }
        EXPECT(b.n_on == count);                                                // n_on equals the count of `on` records
    }
}

static void the_records_own_conditions()
{
    aidax_delay_params p{};
    lcg_state = 5u;
    const aidax_delay_rec good = some_rec(300, &p);
    EXPECT(DelayBook::valid(good));
    auto bad = [&](auto&& change) { aidax_delay_rec r = good; change(r); return !DelayBook::valid(r); };
    const float nan = __builtin_nanf(""), inf = __builtin_inff();
    EXPECT(bad([](aidax_delay_rec& r) { r.m = 63; }) && bad([](aidax_delay_rec& r) { r.m = AIDAX_DELAY_MAX + 1; }) && bad([](aidax_delay_rec& r) { r.m = 0xffffffffu; }));
    EXPECT(bad([](aidax_delay_rec& r) { r.depth_q16 = (AIDAX_DELAY_MAX_DEPTH << 16) + 1u; }) && bad([](aidax_delay_rec& r) { r.fade = AIDAX_DELAY_MAX_FADE + 1; }));
    EXPECT(bad([](aidax_delay_rec& r) { r.fb = 0.99f; }) && bad([](aidax_delay_rec& r) { r.fb = -0.99f; }) && bad([&](aidax_delay_rec& r) { r.fb = nan; }));
    EXPECT(bad([](aidax_delay_rec& r) { r.damp = -0.01f; }) && bad([](aidax_delay_rec& r) { r.damp = 0.51f; }) && bad([&](aidax_delay_rec& r) { r.damp = nan; }));
    EXPECT(bad([](aidax_delay_rec& r) { r.wet = 4.5f; }) && bad([&](aidax_delay_rec& r) { r.wet = nan; }) && bad([&](aidax_delay_rec& r) { r.dry = -inf; }));
    // the capacity's edge: m + ceil(depth) == cap fits, one Q16 step more does not; nothing wraps at the largest values
    DelayBook b;
    b.init(1, 300);
    aidax_delay_rec r = good;
    r.m = 290; r.depth_q16 = 10u << 16;
    EXPECT(b.fits(r));
    r.depth_q16 += 1u;
    EXPECT(!b.fits(r));
    r.m = 0xffffffffu; r.depth_q16 = 0xffffffffu;
    EXPECT(!b.fits(r));
    ++steps;
}

// the off-to-on rule's fixed case (asan_on_runs_case.h), with a record that fits
static void the_runs_that_restart()
{
    aidax_delay_params p{};
    lcg_state = 5u;
    aidax_delay_rec r = some_rec(300, &p);
    r.m = 100; r.depth_q16 = 0;
    DelayBook seven;
    seven.init(7, 300);
    failures += on_runs_case("asan_delay_harness", seven, [&](uint32_t lo, uint32_t hi, bool on) -> const std::vector<DelayBook::Run>& {
        bool ok = false;
        const std::vector<DelayBook::Run>& runs = seven.set(lo, hi, on ? &r : nullptr, on ? &p : nullptr, &ok);
        EXPECT(ok);
        return runs;
    });
    ++steps;
}

int main()
{
    the_records_own_conditions();
    the_runs_that_restart();
    for (uint32_t n : { 1u, 2u, 7u, 70u })
        for (uint32_t seed : { 1u, 77u, 2024u }) run(n, n == 7u ? 64u : 300u, seed * 2654435761u + n, 400);
    std::printf("asan_delay_harness: %d steps, %d failures\n", steps, failures);
    return failures ? 1 : 0;
}
