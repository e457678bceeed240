// The bus limiters' host half under AddressSanitizer + UndefinedBehaviorSanitizer (`make asan_limit`, tests/test_asan_limit.py): LimitBook
// (aidax_limit_stage.h: the buses' records and parameters, the capacities, the dirty range, the ring position and the ring row's length)
// held against a direct restatement of the rules of include/aidax.h ("Bus limiters") over seeded random steps: limiters set for one bus
// and for all, switched off, records beyond the capacities (refused: nothing changes), passes of ragged lengths, passes of no frames and
// prefix passes (the limiters run over every bus whatever the pass's streams, so a prefix pass moves the position like any other). The
// records are uploaded as LimitStage::after_mix does it — only what the dirty range names — and every pass checks the device's copy
// against the restatement, and, on a ring row of the book's own length that holds frame numbers, that the history the widest admitted
// record reads (2 L + H - 1 frames behind the pass) is still there after the pass's frames have been appended. CPU only.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "aidax.h"
#include "../aidadsp-lv2_amd/csrc/aidax_limit_stage.h"

namespace aidax {
// (aidax_model.cpp, linked for fail() and aidax_last_error(), asks the pool which models have a kernel: no model is loaded here)
bool model_supported(const aidax_model&) { return true; }
}  // namespace aidax

static int failures = 0, steps = 0;
#define EXPECT(c) do { if (!(c)) { std::fprintf(stderr, "asan_limit_harness: %s failed at line %d (%s)\n", #c, __LINE__, aidax_last_error()); ++failures; } } while (0)

using aidax::LimitBook;
using aidax::LimitRec;

static uint32_t lcg_state = 88172645u;
static uint32_t rnd(uint32_t n) { lcg_state = lcg_state * 1664525u + 1013904223u; return (lcg_state >> 8) % n; }

static bool same(const aidax_bus_limit_params& a, const aidax_bus_limit_params& b) { return std::memcmp(&a, &b, sizeof a) == 0; }
static bool same(const LimitRec& a, const LimitRec& b) { return std::memcmp(&a, &b, sizeof a) == 0; }

static const uint32_t kBlocks[] = { 1, 3, 0, 63, 64, 65, 257, 4, 8192 };

// parameters that design to `look` and `hold` frames at 48 kHz, with a ceiling of their own at every call
static aidax_bus_limit_params some_params(uint32_t look, uint32_t hold)
{
    aidax_bus_limit_params p{};
    p.ceiling_db = -60.f + 0.5f * static_cast<float>(rnd(145));
    p.lookahead_ms = static_cast<float>(look * 1000.0 / 48000.0);
    p.hold_ms = static_cast<float>(hold * 1000.0 / 48000.0);
    return p;
}

static void run(uint32_t n, uint32_t cap_look, uint32_t cap_hold, uint32_t max_frames, uint32_t seed, int n_steps)
{
    lcg_state = seed;
    LimitBook b;
    b.init(n, cap_look, cap_hold);
    const uint32_t row = LimitBook::ring_row(cap_look, cap_hold, max_frames), reach = 2u * cap_look + cap_hold - 1u;
    EXPECT(row >= reach + max_frames && (row & (row - 1u)) == 0u && (row / 2u < reach + max_frames || row == 1u));
    EXPECT(b.dirty.empty() && b.pos == 0u && b.h_rec.size() == n && b.params.size() == n && b.n_buses == n);
    // what the harness knows: who is on, with which parameters and record; what the device would hold after the last upload; the frames issued
    std::vector<uint8_t> on(n, 0);
    std::vector<aidax_bus_limit_params> params(n);
    std::vector<LimitRec> rec(n, LimitRec{}), device(n, LimitRec{});
    std::vector<int64_t> ring(row, -1);                                         // the frame number each slot of one bus's ring row holds
    uint64_t issued = 0;
    for (int step = 0; step < n_steps; ++step, ++steps) {
        const uint32_t op = rnd(8);
        if (op >= 5) {                                                          // a pass (op 7: a prefix pass), as LimitStage::after_mix issues it
            const uint32_t frames = std::min(kBlocks[rnd(sizeof kBlocks / sizeof kBlocks[0])], max_frames);
            const uint32_t n_active = op == 7 ? rnd(n + 1u) : n;
            (void)n_active;                                                     // (k_mix's business: the limiters take every bus)
            if (frames == 0) continue;                                          // a pass of no frames uploads nothing and moves nothing
            if (!b.dirty.empty()) {
                EXPECT(b.dirty.lo <= b.dirty.hi && b.dirty.hi < n);
                std::copy(b.h_rec.begin() + b.dirty.lo, b.h_rec.begin() + b.dirty.hi + 1, device.begin() + b.dirty.lo);
                b.dirty.clear();
            }
            for (uint32_t i = 0; i < n; ++i) EXPECT(same(device[i], rec[i]));    // the pass plays under the records in force
            EXPECT(b.pos == static_cast<uint32_t>(issued));
            const uint32_t mask = row - 1u, pos = b.pos;
            for (uint32_t t = 0; t < frames; ++t) ring[(pos + t) & mask] = static_cast<int64_t>(issued + t);      // the append
            for (uint32_t back = 1; back <= reach; ++back) {                   // ... has left the widest record's history in place
                const int64_t frame = static_cast<int64_t>(issued) - back;
                if (frame >= 0) EXPECT(ring[(pos - back) & mask] == frame);
            }
            b.advance(frames);
            issued += frames;
            EXPECT(b.pos == static_cast<uint32_t>(issued));
        } else {
            const bool all = rnd(4) == 0, set = op != 0;
            const uint32_t lo = all ? 0u : rnd(n), hi = all ? n : lo + 1u;
            // one call in four asks for more than the capacities admit (where the header's own bounds leave room for that)
            const bool beyond = set && rnd(4) == 0;
            uint32_t look = 1u + rnd(cap_look), hold = rnd(cap_hold + 1u);
            if (beyond) {
                if (rnd(2) && cap_look < AIDAX_BUS_LOOKAHEAD_MAX) look = cap_look + 1u + rnd(AIDAX_BUS_LOOKAHEAD_MAX - cap_look);
                else if (cap_hold < AIDAX_BUS_HOLD_MAX) hold = cap_hold + 1u + rnd(AIDAX_BUS_HOLD_MAX - cap_hold);
            }
            const bool fits = look <= cap_look && hold <= cap_hold;
            aidax_bus_limit_params p = some_params(look, hold);
            aidax_bus_limit_rec designed{};
            if (set) EXPECT(aidax_bus_limit_design(&p, 48000.0, &designed) == AIDAX_OK && designed.on == 1u && designed.lookahead == look && designed.hold == hold && designed.ceiling > 0.f);
            const aidax::DirtyRange was = b.dirty;
            const bool took = b.set(lo, hi, set ? &designed : nullptr, set ? &p : nullptr);
            EXPECT(took == (!set || fits));
            if (!took) {
                EXPECT(b.dirty.lo == was.lo && b.dirty.hi == was.hi);           // a refused record changes nothing (the records are compared below)
            } else {
                for (uint32_t i = lo; i < hi; ++i) {
                    on[i] = set ? 1 : 0;
                    if (set) { params[i] = p; std::memcpy(&rec[i], &designed, sizeof(LimitRec)); }
                    else rec[i].on = 0u;
                }
                EXPECT(!b.dirty.empty() && b.dirty.lo <= lo && hi - 1 <= b.dirty.hi && b.dirty.hi < n);      // dirty covers [lo, hi)
            }
        }
        for (uint32_t i = 0; i < n; ++i) {
            EXPECT(same(b.h_rec[i], rec[i]) && (b.h_rec[i].on != 0u) == (on[i] != 0));
            EXPECT(b.latency(i) == (on[i] ? rec[i].lookahead : 0u));
            if (on[i]) EXPECT(same(b.params[i], params[i]) && b.fits(aidax_bus_limit_rec{ rec[i].ceiling, rec[i].lookahead, rec[i].hold, 1u }));
            // what differs from the device's copy lies inside the dirty range
            if (!same(b.h_rec[i], device[i])) EXPECT(!b.dirty.empty() && b.dirty.lo <= i && i <= b.dirty.hi);
        }
    }
}

int main()
{
    // the ring position wraps at 2^32 like any other step: a book started just below it
    {
        LimitBook b;
        b.init(1, 1, 0);
        b.pos = 0xFFFFFF00u;
        b.advance(257);
        EXPECT(b.pos == 1u);
        EXPECT(LimitBook::ring_row(1, 0, 1) == 2u && LimitBook::ring_row(512, 4096, 8192) == 16384u && LimitBook::ring_row(512, 4096, 257) == 8192u);
    }
    const uint32_t caps[][3] = { { 1, 0, 1 }, { 64, 0, 257 }, { 64, 100, 64 }, { 512, 4096, 257 }, { 512, 4096, 8192 }, { 7, 4096, 100 } };
    for (const auto& c : caps)
        for (uint32_t n : { 1u, 3u, 70u })
            run(n, c[0], c[1], c[2], c[0] * 2654435761u + n + c[1], 120);
    std::printf("asan_limit_harness: %d steps, %d failures\n", steps, failures);
    return failures ? 1 : 0;
}
