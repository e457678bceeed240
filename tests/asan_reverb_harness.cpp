// The bus reverbs' host half under AddressSanitizer + UndefinedBehaviorSanitizer (`make asan_reverb`, tests/test_asan_reverb.py):
// ReverbBook (aidax_reverb_stage.h: the buses' records and parameters, the delay capacity, the dirty range, the frame position, the
// epochs and their refresh, the ring row's length) held against a direct restatement of the rules of include/aidax.h ("Bus reverbs")
// over seeded random steps: reverbs set by parameters and by records, for one bus and for all, switched off, reset, records with a
// delay beyond the capacity (refused: nothing changes), passes of ragged lengths, passes of no frames and prefix passes (the reverbs
// run over every bus whatever the pass's streams, so a prefix pass moves the position like any other). The records are uploaded as
// ReverbStage::after_mix does it — the refresh, then only what the dirty range names — and every pass checks the device's copy against
// the restatement, the epoch the device compares with against the bus's epoch in 64-bit frames for every read the kernel can make
// (back to the capacity + 1 frames behind the pass), and, on a ring row of the book's own length that holds frame numbers, that this
// history is still there after the pass's frames have been appended. The same steps run from positions just below 2^31 and 2^32, and
// a book whose refresh is switched off must fail there. CPU only.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "aidax.h"
#include "../aidadsp-lv2_amd/csrc/aidax_reverb_stage.h"

namespace aidax {
// (aidax_model.cpp, linked for fail() and aidax_last_error(), asks the pool which models have a kernel: no model is loaded here)
bool model_supported(const aidax_model&) { return true; }
}  // namespace aidax

static int failures = 0, steps = 0;
static bool quiet = false;                     // (the run that must fail counts its failures without printing them)
#define EXPECT(c) do { if (!(c)) { if (!quiet) std::fprintf(stderr, "asan_reverb_harness: %s failed at line %d (%s)\n", #c, __LINE__, aidax_last_error()); ++failures; } } while (0)

using aidax::ReverbBook;
using aidax::ReverbRec;

static uint32_t lcg_state = 88172645u;
static uint32_t rnd(uint32_t n) { lcg_state = lcg_state * 1664525u + 1013904223u; return (lcg_state >> 8) % n; }

static bool same(const aidax_bus_reverb_params& a, const aidax_bus_reverb_params& b) { return std::memcmp(&a, &b, sizeof a) == 0; }
// everything of a record but its epoch, which is compared by what it classifies
static bool same_but_epoch(ReverbRec a, ReverbRec b) { a.epoch = b.epoch = 0u; return std::memcmp(&a, &b, sizeof a) == 0; }

static const uint32_t kBlocks[] = { 1, 3, 0, 63, 64, 65, 257, 4, 8192 };

// a record of the harness's own with its delays in [64, top]
static aidax_bus_reverb_rec some_rec(uint32_t top)
{
    aidax_bus_reverb_rec r{};
    for (uint32_t i = 0; i < 8; ++i) {
        r.m[i] = 64u + rnd(top - 63u);
        r.gq[i] = 0.35f * static_cast<float>(rnd(1000)) / 1000.f;
    }
    r.a = 0.5f * static_cast<float>(rnd(101)) / 100.f;
    r.wet = -4.f + 0.08f * static_cast<float>(rnd(101));
    r.dry = 4.f - 0.08f * static_cast<float>(rnd(101));
    r.on = rnd(2); r.epoch = rnd(1000);                                        // (not the caller's to set: ignored)
    return r;
}

// the book against the restatement over n_steps random steps from the frame position `start`; returns nothing: EXPECT counts
static void run(uint32_t n, uint32_t cap, uint32_t max_frames, uint64_t start, uint32_t seed, int n_steps, bool refreshes)
{
    lcg_state = seed;
    ReverbBook b;
    b.init(n, cap);
    b.refreshes = refreshes;
    const uint32_t row = ReverbBook::ring_row(cap, max_frames), reach = cap + 1u;
    EXPECT(row >= reach + max_frames && (row & (row - 1u)) == 0u && row / 2u < reach + max_frames);
    EXPECT(b.dirty.empty() && b.pos() == 0u && b.h_rec.size() == n && b.params.size() == n && b.n_buses == n && b.max_delay == cap);
    // what the harness knows: who is on, with which parameters and record, since which frame (64 bits); what the device would hold
    // after the last upload; the frames issued
    std::vector<uint8_t> on(n, 0), by_params(n, 0);
    std::vector<aidax_bus_reverb_params> params(n);
    std::vector<ReverbRec> rec(n, ReverbRec{}), device(n, ReverbRec{});
    std::vector<uint64_t> epoch(n, 0);
    std::vector<int64_t> ring(row, -1);                                         // the frame number each slot of one line's ring row holds
    uint64_t issued = 0, ring_from = 0;                                         // (ring_from: the first frame the harness's ring row has seen)
    bool moved = false;
    for (int step = 0; step < n_steps; ++step, ++steps) {
        bool pass_now = false;
        if (!moved && step == n_steps / 4) {
            // a long time passes: `start` frames of reverberated passes, which the book is told of in one piece. Every reverb that is on
            // keeps its epoch (nothing cut its tail), so an epoch of the first quarter is now `start` frames old.
            moved = true;
            if (start > issued) {                                              // (start 0: no time passes)
                if (!on[n - 1u]) {                                             // one reverb is on across it for certain: the last bus's
                    const aidax_bus_reverb_rec r = some_rec(cap);
                    EXPECT(b.set(n - 1u, n, &r, nullptr));
                    on[n - 1u] = 1; by_params[n - 1u] = 0; epoch[n - 1u] = issued;
                    std::memcpy(&rec[n - 1u], &r, sizeof(ReverbRec));
                    rec[n - 1u].on = 1u;
                }
                pass_now = true;                                               // ... and the first step behind it is a pass
                b.frames = issued = ring_from = start;
                b.next_scan = start;                                           // (the look at the epochs is due, as it has been many times on the way)
                std::fill(ring.begin(), ring.end(), -1);
            }
        }
        const uint32_t op = pass_now ? 6u : rnd(9);
        if (op >= 6) {                                                          // a pass (op 8: a prefix pass), as ReverbStage::after_mix issues it
            const uint32_t frames = pass_now ? 1u : std::min(kBlocks[rnd(sizeof kBlocks / sizeof kBlocks[0])], max_frames);
            const uint32_t n_active = op == 8 ? rnd(n + 1u) : n;
            (void)n_active;                                                     // (k_mix's business: the reverbs take every bus)
            if (frames == 0) continue;                                          // a pass of no frames uploads nothing and moves nothing
            b.refresh();
            if (!b.dirty.empty()) {
                EXPECT(b.dirty.lo <= b.dirty.hi && b.dirty.hi < n);
                std::copy(b.h_rec.begin() + b.dirty.lo, b.h_rec.begin() + b.dirty.hi + 1, device.begin() + b.dirty.lo);
                b.dirty.clear();
            }
            EXPECT(b.pos() == static_cast<uint32_t>(issued) && b.frames == issued);
            const uint32_t mask = row - 1u, pos = b.pos();
            for (uint32_t i = 0; i < n; ++i) {                                  // the pass plays under the records in force
                EXPECT(same_but_epoch(device[i], rec[i]));
                if (!on[i]) continue;
                // every frame the kernel can read: the pass's own and the capacity + 1 behind it (the oldest, the youngest, around the epoch)
                const uint64_t first = issued >= reach ? issued - reach : 0u, last = issued + frames - 1u;
                const uint64_t probes[] = { first, first + 1u, (first + last) / 2u, last, epoch[i], epoch[i] ? epoch[i] - 1u : 0u, epoch[i] + 1u };
                for (uint64_t j : probes) {
                    if (j < first || j > last) continue;
                    const bool kept = static_cast<int32_t>(static_cast<uint32_t>(j) - device[i].epoch) >= 0;
                    EXPECT(kept == (j >= epoch[i]));
                }
                // frames that lie before frame 0 of the book's life read as 0 through the epoch as well
                if (issued < reach) EXPECT(static_cast<int32_t>(static_cast<uint32_t>(issued - reach) - device[i].epoch) < 0);
            }
            for (uint32_t t = 0; t < frames; ++t) ring[(pos + t) & mask] = static_cast<int64_t>(issued + t);      // the append
            for (uint32_t back = 1; back <= reach; ++back) {                   // ... has left the longest delay's history in place
                const int64_t frame = static_cast<int64_t>(issued) - back;
                if (frame >= 0 && static_cast<uint64_t>(frame) >= ring_from) EXPECT(ring[(pos - back) & mask] == frame);
            }
            b.advance(frames);
            issued += frames;
            EXPECT(b.pos() == static_cast<uint32_t>(issued));
        } else if (op == 5) {                                                   // a reset: a new epoch, on or off
            const bool all = rnd(4) == 0;
            const uint32_t lo = all ? 0u : rnd(n), hi = all ? n : lo + 1u;
            b.reset(lo, hi);
            for (uint32_t i = lo; i < hi; ++i) epoch[i] = issued;
            EXPECT(!b.dirty.empty() && b.dirty.lo <= lo && hi - 1 <= b.dirty.hi && b.dirty.hi < n);
        } else {
            const bool all = rnd(4) == 0, set = op != 0, designed = set && rnd(2) == 0, keep_delays = set && !designed && rnd(3) == 0;
            const uint32_t lo = all ? 0u : rnd(n), hi = all ? n : lo + 1u;
            // one call in four asks for more than the capacity admits (where the header's own bound leaves room for that)
            const bool beyond = set && !keep_delays && rnd(4) == 0 && cap < AIDAX_BUS_REVERB_MAX_DELAY;
            aidax_bus_reverb_rec r{};
            aidax_bus_reverb_params p{};
            if (designed) {
                // at 48 kHz the longest line is 2999 * size frames (rounded, made odd and distinct: a few frames more)
                const double top = beyond ? std::min(2.0, (cap + 40.0) / 2999.0 * 1.5) : std::min(2.0, (cap - 20.0) / 2999.0);
                p.rt60_s = 0.1f + 0.1f * static_cast<float>(rnd(100));
                p.size = static_cast<float>(std::max(0.05, top));
                p.damping = 0.01f * static_cast<float>(rnd(101));
                p.wet = 0.5f; p.dry = 1.f; p.variant = rnd(4);
                EXPECT(aidax_bus_reverb_design(&p, 48000.0, &r) == AIDAX_OK && r.on == 1u && ReverbBook::valid(r));
            } else if (set) {
                r = some_rec(cap);
                if (keep_delays && on[lo]) std::memcpy(r.m, rec[lo].m, sizeof r.m);      // only gq, a, wet and dry change (for bus lo at least)
                if (beyond) r.m[rnd(8)] = cap + 1u + rnd(AIDAX_BUS_REVERB_MAX_DELAY - cap);
                EXPECT(ReverbBook::valid(r));
            }
            bool fits = true;
            for (uint32_t i = 0; i < 8; ++i) fits = fits && (!set || r.m[i] <= cap);
            EXPECT(!beyond || !fits || designed);                               // (a designed record beyond a large capacity may still fit: size ends at 2)
            const aidax::DirtyRange was = b.dirty;
            const std::vector<ReverbRec> before = b.h_rec;
            const bool took = b.set(lo, hi, set ? &r : nullptr, designed ? &p : nullptr);
            EXPECT(took == (!set || fits) && b.fits(r) == fits);
            if (!took) {
                EXPECT(b.dirty.lo == was.lo && b.dirty.hi == was.hi);           // a refused record changes nothing
                for (uint32_t i = 0; i < n; ++i) EXPECT(std::memcmp(&before[i], &b.h_rec[i], sizeof(ReverbRec)) == 0);
            } else {
                for (uint32_t i = lo; i < hi; ++i) {
                    if (!set) { on[i] = 0; rec[i].on = 0u; continue; }
                    // off -> on and other delays start a new epoch; other gains, damping and levels alone do not
                    if (!on[i] || std::memcmp(rec[i].m, r.m, sizeof r.m) != 0) epoch[i] = issued;
                    on[i] = 1; by_params[i] = designed ? 1 : 0;
                    params[i] = p;
                    std::memcpy(&rec[i], &r, sizeof(ReverbRec));
                    rec[i].on = 1u;
                }
                EXPECT(!b.dirty.empty() && b.dirty.lo <= lo && hi - 1 <= b.dirty.hi && b.dirty.hi < n);      // dirty covers [lo, hi)
            }
        }
        for (uint32_t i = 0; i < n; ++i) {
            EXPECT(same_but_epoch(b.h_rec[i], rec[i]) && (b.h_rec[i].on != 0u) == (on[i] != 0));
            if (on[i]) {
                EXPECT(b.since_epoch(i) == issued - epoch[i]);
                EXPECT(same(b.params[i], by_params[i] ? params[i] : aidax_bus_reverb_params{}));
            }
            // what differs from the device's copy lies inside the dirty range
            if (std::memcmp(&b.h_rec[i], &device[i], sizeof(ReverbRec)) != 0) EXPECT(!b.dirty.empty() && b.dirty.lo <= i && i <= b.dirty.hi);
        }
    }
}

int main()
{
    {
        ReverbBook b;
        b.init(1, 64);
        b.frames = 0xFFFFFF00u;
        b.advance(257);
        EXPECT(b.pos() == 1u && b.frames == 0x100000001ull);
        EXPECT(ReverbBook::ring_row(64, 1) == 128u && ReverbBook::ring_row(128, 257) == 512u && ReverbBook::ring_row(4096, 257) == 8192u && ReverbBook::ring_row(32768, 8192) == 65536u);
        // the record's own conditions
        aidax_bus_reverb_rec r = some_rec(100);
        EXPECT(ReverbBook::valid(r));
        aidax_bus_reverb_rec bad = r; bad.m[3] = 63u; EXPECT(!ReverbBook::valid(bad));
        bad = r; bad.m[7] = 32769u; EXPECT(!ReverbBook::valid(bad));
        bad = r; bad.gq[0] = 0.35355341f; EXPECT(!ReverbBook::valid(bad));      // (the float next above 1 / sqrt(8))
        bad = r; bad.gq[0] = 0.35355338f; EXPECT(ReverbBook::valid(bad));       // (the float next below it)
        bad = r; bad.gq[5] = -0.01f; EXPECT(!ReverbBook::valid(bad));
        bad = r; bad.gq[5] = std::nanf(""); EXPECT(!ReverbBook::valid(bad));
        bad = r; bad.a = 0.51f; EXPECT(!ReverbBook::valid(bad));
        bad = r; bad.a = -0.01f; EXPECT(!ReverbBook::valid(bad));
        bad = r; bad.a = std::nanf(""); EXPECT(!ReverbBook::valid(bad));
        bad = r; bad.wet = 4.01f; EXPECT(!ReverbBook::valid(bad));
        bad = r; bad.dry = -4.01f; EXPECT(!ReverbBook::valid(bad));
        bad = r; bad.wet = std::nanf(""); EXPECT(!ReverbBook::valid(bad));
        bad = r; bad.dry = std::numeric_limits<float>::infinity(); EXPECT(!ReverbBook::valid(bad));
    }
    const uint32_t caps[][2] = { { 64, 1 }, { 128, 257 }, { 512, 64 }, { 4096, 257 }, { 32768, 8192 }, { 100, 100 } };
    // from frame 0, and from just below 2^31 and 2^32 (an epoch of the first quarter of the steps is that old when the rest runs)
    const uint64_t starts[] = { 0u, (1ull << 31) - 300u, (1ull << 32) - 300u, (1ull << 33) + (1ull << 31) - 100u };
    for (const auto& c : caps)
        for (uint32_t n : { 1u, 3u, 70u })
            for (uint64_t start : starts)
                run(n, c[0], c[1], start, c[0] * 2654435761u + n + c[1] + static_cast<uint32_t>(start >> 20), 100, true);
    // ... and a book without the refresh must fail this step: the same runs from the two wraps, counted apart
    const int good = failures;
    quiet = true;
    for (uint64_t start : { (1ull << 31) - 300u, (1ull << 32) - 300u })
        run(3, 128, 257, start, 7u + static_cast<uint32_t>(start >> 20), 100, false);
    quiet = false;
    const int without = failures - good;
    failures = good;
    if (without == 0) { std::fprintf(stderr, "asan_reverb_harness: a book without the epoch refresh passed the wrap\n"); ++failures; }
    std::printf("asan_reverb_harness: %d steps, %d failures\n(a book without the epoch refresh fails %d checks at the wraps)\n", steps, failures, without);
    return failures ? 1 : 0;
}
