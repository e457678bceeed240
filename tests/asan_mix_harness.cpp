// The mix buses' host half under AddressSanitizer + UndefinedBehaviorSanitizer (`make asan_mix`, tests/test_asan_mix.py): MixBook
// (aidax_mix_stage.h: the sends, their ramps, the CSR plan, the dirty state, the advance per pass and per prefix) held against a direct
// restatement of the rules of include/aidax.h ("Mix buses") over seeded random steps: sends set, moved and removed for one stream and
// for all, several calls between two passes, passes of ragged lengths and prefix passes (n_active < n_streams: no public call reaches
// one without the hub, so this is where the prefix rule is tested). The plan is uploaded as MixStage::after_pass does it — only when the
// book says so — and every pass checks what k_mix would compute from the device's copy: the entries of every bus and their order, and
// each active entry's gain at the pass's first, last and a middle frame, against the restatement's own frame counters. CPU only.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <utility>
#include <vector>

#include "aidax.h"
#include "../aidadsp-lv2_amd/csrc/aidax_mix_stage.h"

namespace aidax {
// (aidax_model.cpp, linked for fail() and aidax_last_error(), asks the pool which models have a kernel: no model is loaded here)
bool model_supported(const aidax_model&) { return true; }
}  // namespace aidax

static int failures = 0, steps = 0;
#define EXPECT(c) do { if (!(c)) { std::fprintf(stderr, "asan_mix_harness: %s failed at line %d (%s)\n", #c, __LINE__, aidax_last_error()); ++failures; } } while (0)

using aidax::MixBook;
using aidax::MixEntry;

static uint32_t lcg_state = 88172645u;
static uint32_t rnd(uint32_t n) { lcg_state = lcg_state * 1664525u + 1013904223u; return (lcg_state >> 8) % n; }

static float gain_at(float g0, float g1, uint32_t ramp, uint32_t k)
{
    float g = -99.f;
    EXPECT(aidax_mix_gain(g0, g1, ramp, k, &g) == AIDAX_OK);
    return g;
}
static bool same_bits(float a, float b) { return std::memcmp(&a, &b, sizeof a) == 0; }

// the restatement's send: where it is set to, where it last played and at which gain, its ramp and the frames issued of it
struct RefSend {
    int32_t bus = AIDAX_BUS_NONE, played = AIDAX_BUS_NONE;
    float g0 = 0.f, g1 = 0.f, now = 0.f;
    uint32_t len = 0;
    uint64_t k = 0;                                                             // frames issued since the ramp was set (not saturating)
    bool ended_at_set = true;
    float g_now() const { return bus != AIDAX_BUS_NONE && bus == played ? now : 0.f; }
    float frame(uint64_t t) const { return ended_at_set ? g1 : gain_at(g0, g1, len, static_cast<uint32_t>(std::min<uint64_t>(k + t, 1u << 30))); }
    uint32_t left() const
    {
        if (ended_at_set) return 0;
        const uint64_t total = std::max(len, 1u);
        return k >= total ? 0u : static_cast<uint32_t>(total - k);
    }
};

static const uint32_t kRamps[] = { 0, 1, 2, 3, 7, 64, 100, 257, 1000, 48000, 1u << 24 };
static const uint32_t kBlocks[] = { 1, 3, 63, 64, 65, 257, 4, 8192 };

static void run(uint32_t n, uint32_t n_buses, uint32_t seed, int n_steps)
{
    lcg_state = seed;
    MixBook b;
    b.init(n, n_buses);
    std::vector<RefSend> ref(static_cast<size_t>(n) * AIDAX_SENDS);
    // the device's copy of the plan: what the last upload left there
    std::vector<uint8_t> device(b.plan_bytes(), 0xEE), snapshot(b.plan_bytes());
    uint32_t uploads = 0, passes_since_change = 0;
    EXPECT(b.dirty && b.n_entries == 0 && b.sends.size() == ref.size() && b.bus_start.size() == n_buses + 1u);

    for (int step = 0; step < n_steps; ++step, ++steps) {
        const uint32_t op = rnd(10);
        if (op < 6) {
            // one to three calls between two passes: the last one on a send wins, from the same g0
            const uint32_t calls = 1u + rnd(3);
            for (uint32_t c = 0; c < calls; ++c) {
                const bool all = rnd(5) == 0;
                const uint32_t lo = all ? 0u : rnd(n), hi = all ? n : lo + 1u, send = rnd(AIDAX_SENDS);
                const uint32_t kind = rnd(6);                                   // 0: remove; 1, 2: the bus it is on (a new ramp); else: any bus
                const float gain = rnd(8) == 0 ? 0.f : (static_cast<float>(rnd(4097)) - 2048.f) / 1024.f;
                const uint32_t len = kRamps[rnd(sizeof kRamps / sizeof *kRamps)];
                for (uint32_t s = lo; s < hi; ++s) {
                    RefSend& x = ref[static_cast<size_t>(s) * AIDAX_SENDS + send];
                    const int32_t bus = kind == 0 ? AIDAX_BUS_NONE : (kind <= 2 && x.bus != AIDAX_BUS_NONE) ? x.bus : static_cast<int32_t>(rnd(n_buses));
                    b.set(s, send, bus, gain, len);
                    x.bus = bus;
                    x.g0 = x.g_now();
                    x.g1 = bus == AIDAX_BUS_NONE ? 0.f : gain + 0.f;
                    x.len = len;
                    x.k = 0;
                    x.ended_at_set = x.g0 == x.g1;
                }
                EXPECT(b.dirty);
            }
            passes_since_change = 0;
        } else {
            // a pass: whole or a prefix, of a ragged length (op 9: of no frames — nothing moves, nothing is uploaded)
            const uint32_t n_active = rnd(3) == 0 ? 1u + rnd(n) : n;
            const uint32_t frames = op == 9 ? 0u : kBlocks[rnd(sizeof kBlocks / sizeof *kBlocks)];
            if (frames != 0) {
                const uint32_t before = uploads;
                if (b.dirty) {
                    b.rebuild();
                    std::fill(snapshot.begin(), snapshot.end(), 0xEE);
                    const size_t bytes = b.serialise(snapshot.data());
                    EXPECT(bytes <= device.size() && bytes == b.entries_off() + sizeof(MixEntry) * b.n_entries);
                    std::memcpy(device.data(), snapshot.data(), bytes);
                    ++uploads;
                }
                if (n_active == n && passes_since_change >= 1) EXPECT(uploads == before);      // whole passes without a change upload nothing, ramps or not
                const uint32_t* bus_start = reinterpret_cast<const uint32_t*>(device.data());
                std::vector<MixEntry> entries(b.n_entries);
                if (b.n_entries) std::memcpy(entries.data(), device.data() + b.entries_off(), sizeof(MixEntry) * b.n_entries);
                const uint32_t k_off = b.since_build;
                EXPECT(bus_start[0] == 0 && k_off <= aidax::kMixMaxRampOffset);
                uint32_t longest = 0;
                for (uint32_t bus = 0; bus < n_buses; ++bus) {
                    // the restatement's list of the bus: its sends in ascending (stream, send) order, over ALL streams (k_mix leaves out the ones beyond n_active)
                    std::vector<std::pair<uint32_t, uint32_t>> want;
                    for (uint32_t s = 0; s < n; ++s)
                        for (uint32_t j = 0; j < AIDAX_SENDS; ++j)
                            if (ref[static_cast<size_t>(s) * AIDAX_SENDS + j].bus == static_cast<int32_t>(bus)) want.push_back({ s, j });
                    const uint32_t lo = bus_start[bus], hi = bus_start[bus + 1u];
                    EXPECT(lo <= hi && hi <= b.n_entries && hi - lo == want.size());
                    longest = std::max<uint32_t>(longest, static_cast<uint32_t>(want.size()));
                    for (uint32_t i = lo; i < hi && i - lo < want.size(); ++i) {
                        const MixEntry& e = entries[i];
                        EXPECT(e.stream == want[i - lo].first && e.ramp <= (1u << 24) && e.k <= (1u << 24));
                        if (e.stream >= n_active) continue;                     // left out of this pass: its gain is not looked at
                        const RefSend& x = ref[static_cast<size_t>(e.stream) * AIDAX_SENDS + want[i - lo].second];
                        for (uint32_t t : { 0u, frames / 2u, frames - 1u }) {
                            const uint32_t k = e.k + k_off + t;                 // as k_mix forms it
                            EXPECT(same_bits(gain_at(e.g0, e.g1, e.ramp, k), x.frame(t)));
                        }
                    }
                }
                EXPECT(bus_start[n_buses] == b.n_entries && b.max_entries == longest);
                b.advance(n_active, frames);
                for (uint32_t s = 0; s < n_active; ++s)
                    for (uint32_t j = 0; j < AIDAX_SENDS; ++j) {
                        RefSend& x = ref[static_cast<size_t>(s) * AIDAX_SENDS + j];
                        x.played = x.bus;
                        x.now = x.bus == AIDAX_BUS_NONE ? 0.f : x.frame(frames - 1u);
                        x.k += frames;
                    }
                if (n_active == n) ++passes_since_change; else passes_since_change = 0;
            } else {
                const bool dirty = b.dirty;
                const uint32_t since = b.since_build;
                b.advance(n_active, 0);
                EXPECT(b.dirty == dirty && b.since_build == since);
            }
        }
        // aidax_pool_stream_send's answers, and the count of sends that have something left to do
        uint32_t unsettled = 0;
        for (uint32_t s = 0; s < n; ++s)
            for (uint32_t j = 0; j < AIDAX_SENDS; ++j) {
                const MixBook::Send& got = b.at(s, j);
                const RefSend& x = ref[static_cast<size_t>(s) * AIDAX_SENDS + j];
                EXPECT(got.bus == x.bus && same_bits(MixBook::gain_now(got), x.g_now()) && same_bits(got.g1, x.g1) && MixBook::frames_left(got) == x.left());
                unsettled += (x.bus != x.played || x.left() != 0) ? 1u : 0u;
            }
        EXPECT(b.n_unsettled == unsettled);
    }
    EXPECT(uploads > 0);
}

// a prefix pass asks for another plan only while an entry of a stream it leaves out may still be moving
static void prefix_uploads()
{
    MixBook b;
    b.init(4, 2);
    b.set(0, 0, 0, 1.f, 0);
    b.set(3, 0, 1, 0.5f, 10);
    b.rebuild();
    b.advance(4, 8);
    EXPECT(!b.dirty);
    b.advance(2, 1);                                    // frame 8 of stream 3's 10: it is where it was, the plan's offset is not
    EXPECT(b.dirty && MixBook::frames_left(b.at(3, 0)) == 2);
    b.rebuild();
    b.advance(4, 64);                                   // the ramp has ended, with no rebuild since
    EXPECT(!b.dirty && MixBook::frames_left(b.at(3, 0)) == 0);
    for (int i = 0; i < 3; ++i) {
        b.advance(2, 8);
        EXPECT(!b.dirty);                               // left out at rest: nothing to upload, prefix pass after prefix pass
    }
    ++steps;
}

int main()
{
    prefix_uploads();
    float g = 0.f;
    EXPECT(aidax_mix_gain(0.f, 1.f, 4, 1, &g) == AIDAX_OK && g == 0.5f);
    EXPECT(aidax_mix_gain(0.f, 17.f, 4, 1, &g) == AIDAX_ERR_ARG && aidax_mix_gain(0.f, 1.f, (1u << 24) + 1u, 1, &g) == AIDAX_ERR_ARG && aidax_mix_gain(0.f, 1.f, 4, 1, nullptr) == AIDAX_ERR_ARG);
    const uint32_t buses[] = { 1, 3, 5, 64 };
    int i = 0;
    for (uint32_t n : { 1u, 2u, 7u, 70u }) {
        for (uint32_t seed : { 1u, 77u, 2024u }) run(n, buses[i], seed * 2654435761u + n, 120);
        ++i;
    }
    std::printf("asan_mix_harness: %d steps, %d failures\n", steps, failures);
    return failures ? 1 : 0;
}
