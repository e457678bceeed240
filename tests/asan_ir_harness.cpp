// The host side of the cabinet IR stage under AddressSanitizer + UndefinedBehaviorSanitizer (`make asan_ir`, tests/test_asan_ir.py):
// aidax_ir_resample over rate pairs, leads, caps and refused arguments, with every output buffer allocated at exactly the size the call
// may write, the fragment packer at the longest IR a pool takes, and IrPlan (the stage's plan builder) held against a direct
// restatement of its rules over seeded random assignments, commits and passes. CPU only: device pointers are made-up numbers.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "aidax.h"
#include "../aidadsp-lv2_amd/csrc/aidax_ir_stage.h"

namespace aidax {
// (the library defines this next to the kernel, in aidax_ir_mfma.hip, which is no host source)
uint32_t ir_diagonals(uint32_t n_taps) { return (n_taps + 30u) / 16u + 1u; }
// (aidax_model.cpp, linked for fail() and aidax_last_error(), asks the pool which models have a kernel: no model is loaded here)
bool model_supported(const aidax_model&) { return true; }
}  // namespace aidax

static int failures = 0;
#define EXPECT(c) do { if (!(c)) { std::fprintf(stderr, "asan_ir_harness: %s failed at line %d (%s)\n", #c, __LINE__, aidax_last_error()); ++failures; } } while (0)

using aidax::IrItem;
using aidax::IrPlan;
using aidax::IrSection;
using aidax::IrSlot;
constexpr int kKeys = AIDAX_IR_SLOTS + 1;

static uint32_t lcg_state = 2463534242u;
static uint32_t rnd(uint32_t n) { lcg_state = lcg_state * 1664525u + 1013904223u; return (lcg_state >> 8) % n; }

// what the harness knows of one IR's content, and a staged slot made from it (never dereferenced)
struct Content { uint32_t* frag = nullptr; uint32_t n_diag = 0; uint64_t gen = 0; };
static Content fresh_content()
{
    static uintptr_t next = 0x10000;
    next += 0x1000;
    return Content{ reinterpret_cast<uint32_t*>(next), 3 + rnd(4000), 0 };
}

// A section as the rules state it: for each source in order, the streams whose source it is in ascending order, cut into runs of 64
struct Want {
    std::vector<IrItem> items;
    std::vector<uint32_t> streams;
    uint32_t max_diag = 0;
};
static Want restate(const std::vector<int>& source_of, const std::vector<Content>& sources)
{
    Want w;
    for (size_t k = 0; k < sources.size(); ++k) {
        std::vector<uint32_t> mine;
        for (size_t s = 0; s < source_of.size(); ++s)
            if (source_of[s] == static_cast<int>(k)) mine.push_back(static_cast<uint32_t>(s));
        for (size_t c = 0; c < mine.size(); c += 64)
            w.items.push_back(IrItem{ sources[k].frag, sources[k].n_diag, static_cast<uint32_t>(std::min<size_t>(64, mine.size() - c)),
                                      static_cast<uint32_t>(w.streams.size() + c), 0u });
        if (!mine.empty()) w.max_diag = std::max(w.max_diag, sources[k].n_diag);
        w.streams.insert(w.streams.end(), mine.begin(), mine.end());
    }
    return w;
}
static void expect_section(const IrSection& sec, const Want& w)
{
    EXPECT(sec.n_items == w.items.size() && sec.n_listed == w.streams.size() && sec.max_diag == w.max_diag);
    if (sec.n_items != w.items.size() || sec.n_listed != w.streams.size()) return;
    for (size_t i = 0; i < w.items.size(); ++i)
        EXPECT(sec.items[i].frag == w.items[i].frag && sec.items[i].n_diag == w.items[i].n_diag && sec.items[i].count == w.items[i].count &&
               sec.items[i].first == w.items[i].first);
    EXPECT(std::equal(w.streams.begin(), w.streams.end(), sec.streams.begin()));
}

// serialise() into a snapshot of exactly plan_bytes(): the sections at the documented offsets, nothing else written
static void expect_snapshot(const IrPlan& plan)
{
    const size_t n = plan.n_streams, runs = (n + 63) / 64;
    const size_t streams_off = (runs + kKeys) * sizeof(IrItem), fade_items = (streams_off + 4 * n + 7) / 8 * 8;
    const size_t fade_streams = fade_items + (runs + 2 * kKeys) * sizeof(IrItem), fade_mix = fade_streams + 4 * n, total = fade_mix + 4 * n;
    EXPECT(plan.plan_items_bytes() == streams_off && plan.fade_items_off() == fade_items && plan.fade_streams_off() == fade_streams &&
           plan.fade_mix_off() == fade_mix && plan.plan_bytes() == total);
    std::vector<uint8_t> snap(plan.plan_bytes(), 0xEE), want(plan.plan_bytes(), 0xEE);
    const size_t bytes = plan.serialise(snap.data());
    std::memcpy(want.data(), plan.main.items.data(), plan.main.n_items * sizeof(IrItem));
    std::memcpy(want.data() + streams_off, plan.main.streams.data(), plan.main.n_listed * 4);
    size_t end = streams_off + plan.main.n_listed * 4;
    if (plan.n_mix) {
        std::memcpy(want.data() + fade_items, plan.fade_out.items.data(), plan.fade_out.n_items * sizeof(IrItem));
        std::memcpy(want.data() + fade_streams, plan.fade_out.streams.data(), plan.fade_out.n_listed * 4);
        std::memcpy(want.data() + fade_mix, plan.mix.data(), plan.n_mix * 4);
        end = fade_mix + plan.n_mix * 4;
    }
    EXPECT(bytes == end && bytes <= total && snap == want);
}

static int key_of(int32_t a) { return a == AIDAX_IR_POOL ? 0 : a >= 0 ? 1 + a : -1; }

static int plan_rebuilds = 0;

// The main section: pool sizes around the item size, 0 .. 64 live bank slots with and without a pool IR, streams on AIDAX_IR_NONE and
// on empty slots, and the layouts that make (or just miss) the identity plan
static void main_section_cases()
{
    for (uint32_t n : { 1u, 63u, 64u, 65u, 1000u, 4096u })
        for (int n_live : { 0, 1, 5, 64 })
            for (int pool_ir = 0; pool_ir < 2; ++pool_ir) {
                IrPlan plan;
                plan.init(n);
                std::vector<Content> live(kKeys);
                for (int k = 0; k < kKeys; ++k) {
                    const bool on = k == 0 ? pool_ir != 0 : n_live == 64 || (n_live == 5 && k % 13 == 2) || (n_live == 1 && k == 40);
                    if (!on) continue;
                    live[k] = fresh_content();
                    IrSlot sg{ live[k].frag, 16 * live[k].n_diag, live[k].n_diag, 0 };
                    plan.commit(k, sg);
                    EXPECT(sg.d_frag == nullptr);
                }
                for (int round = 0; round < 6; ++round) {
                    const int32_t one = round == 2 ? AIDAX_IR_POOL : static_cast<int32_t>(rnd(AIDAX_IR_SLOTS));
                    for (uint32_t s = 0; s < n; ++s) {
                        const uint32_t r = rnd(100);
                        plan.assign[s] = round >= 2 && round <= 4 ? one : r < 10 ? AIDAX_IR_NONE : r < 30 ? AIDAX_IR_POOL : static_cast<int32_t>(rnd(AIDAX_IR_SLOTS));
                    }
                    if (round == 4) plan.assign[rnd(n)] = AIDAX_IR_NONE;            // all but one stream on one IR
                    plan.dirty = true;
                    plan.rebuild(false);
                    ++plan_rebuilds;
                    std::vector<int> source_of(n);
                    std::vector<uint32_t> per_key(kKeys, 0);
                    for (uint32_t s = 0; s < n; ++s) {
                        const int k = key_of(plan.assign[s]);
                        source_of[s] = k >= 0 && live[k].frag ? k : -1;
                        EXPECT(plan.key(s) == source_of[s]);
                        if (source_of[s] >= 0) ++per_key[source_of[s]];
                    }
                    expect_section(plan.main, restate(source_of, live));
                    EXPECT(plan.identity == (std::count(per_key.begin(), per_key.end(), n) == 1));
                    EXPECT(!plan.dirty && plan.n_mix == 0 && plan.fade_out.n_items == 0);
                    expect_snapshot(plan);
                }
            }
}

// The fade-out section: commits, assignments and passes in random order against a model of the rules (include/aidax.h, aidax_ir_stage.h).
// fade_mode 0: no fade length; 1: one set throughout; 2: set and cleared at random (how an old IR comes to be held nowhere)
static void fade_section_cases(uint32_t n, int fade_mode)
{
    IrPlan plan;
    plan.init(n);
    plan.fade = fade_mode == 1 ? 256 : 0;
    std::vector<Content> live(kKeys), parked(kKeys);
    std::vector<bool> pass_since_commit(kKeys, false);
    std::vector<int> played_key(n, -1);
    std::vector<uint64_t> played_gen(n, 0);
    uint64_t gen_next = 1;
    bool any_pass = false;
    const int keys[] = { 0, 1, 2, 7, 64 };
    for (int step = 0; step < 600; ++step) {
        const uint32_t op = rnd(10);
        if (fade_mode == 2 && rnd(8) == 0) plan.fade = plan.fade ? 0 : 256;
        if (op < 3) {                                                           // a commit: new content, or none, for one key
            const int k = keys[rnd(5)];
            Content c = rnd(5) == 0 ? Content{} : fresh_content();
            if (c.frag) c.gen = gen_next++;
            IrSlot sg{ c.frag, 16 * c.n_diag, c.n_diag, 0 };
            plan.commit(k, sg);
            // played content is parked and what was parked comes back to be freed; content no pass has played comes back itself
            Content back = live[k];
            if (plan.fade != 0 && pass_since_commit[k]) std::swap(back, parked[k]);
            live[k] = c;
            pass_since_commit[k] = false;
            EXPECT(sg.d_frag == back.frag && (!back.frag || sg.gen == back.gen) && plan.dirty);
            EXPECT(plan.live[k].d_frag == c.frag && plan.live[k].gen == c.gen && plan.parked[k].d_frag == parked[k].frag);
        } else if (op < 6) {                                                    // an assignment
            const int32_t slot = rnd(4) == 0 ? AIDAX_IR_NONE : keys[rnd(5)] - 1;
            if (rnd(6) == 0) std::fill(plan.assign.begin(), plan.assign.end(), slot);
            else plan.assign[rnd(n)] = slot;
            plan.dirty = true;
        } else {                                                                // a pass, as IrStage::begin_pass and issue drive the plan
            const bool rebuilt = plan.dirty;
            plan.spend_fade();
            if (rebuilt) { plan.rebuild(any_pass); ++plan_rebuilds; }
            std::vector<int> main_of(n, -1), fade_of(n, -1);
            std::vector<uint32_t> mix;
            for (uint32_t s = 0; s < n; ++s) {
                const int k = key_of(plan.assign[s]);
                const int nk = k >= 0 && live[k].frag ? k : -1;
                const uint64_t ng = nk >= 0 ? live[nk].gen : 0;
                main_of[s] = nk;
                if (!rebuilt) continue;
                const int ok = played_key[s];
                const uint64_t og = played_gen[s];
                played_key[s] = nk;
                played_gen[s] = ng;
                if (!any_pass || plan.fade == 0 || (nk == ok && ng == og)) continue;
                if (ok < 0) mix.push_back(s | aidax::kIrFadeDry);
                else if (live[ok].frag && live[ok].gen == og) { fade_of[s] = ok; mix.push_back(s); }
                else if (parked[ok].frag && parked[ok].gen == og) { fade_of[s] = kKeys + ok; mix.push_back(s); }
            }
            expect_section(plan.main, restate(main_of, live));
            std::vector<Content> sources(live);
            sources.insert(sources.end(), parked.begin(), parked.end());
            expect_section(plan.fade_out, restate(fade_of, sources));
            EXPECT(plan.n_mix == mix.size() && std::equal(mix.begin(), mix.end(), plan.mix.begin()));
            expect_snapshot(plan);
            if (rnd(12) == 0) continue;                                         // the pass failed on its way: the next one must not find the section
            plan.pass_issued();
            EXPECT(plan.fade_out.n_items == 0 && plan.fade_out.n_listed == 0 && plan.n_mix == 0);
            any_pass = true;
            pass_since_commit.assign(kKeys, true);
        }
    }
}

int main()
{
    std::vector<float> in(3000);
    uint32_t seed = 12345u;
    for (size_t k = 0; k < in.size(); ++k) {
        seed = seed * 1664525u + 1013904223u;
        in[k] = (static_cast<float>(seed >> 8) / 8388608.f - 1.f) * std::exp(-static_cast<float>(k) / 400.f);
    }
    const double pairs[][2] = { { 48000, 44100 }, { 48000, 96000 }, { 48000, 192000 }, { 48000, 32000 }, { 44100, 48000 }, { 48000, 48000 },
                                { 1, 16777216 }, { 16777216, 1 }, { 48000, 44101 }, { 7, 3 } };
    const uint32_t leads[] = { 0, 1, 33, 1024 };
    const uint32_t lengths[] = { 1, 2, 37, 3000 };
    int calls = 0;
    double sum = 0.0;
    for (const auto& pr : pairs)
        for (uint32_t lead : leads)
            for (uint32_t n_in : lengths) {
                const bool huge = pr[1] > 1e6;                                           // 1 -> 2^24: lengths in the billions, queried only
                uint32_t n_full = 0;
                const int rc = aidax_ir_resample(in.data(), n_in, pr[0], pr[1], lead, nullptr, 0, &n_full);
                if (huge && n_in > 37) { EXPECT(rc == AIDAX_ERR_ARG && n_full == 0); continue; }
                EXPECT(rc == AIDAX_OK && n_full > lead);
                for (uint32_t cap : { n_full, n_full / 2 + 1, 1u, n_full + 5 }) {
                    if (huge && cap > 4096) cap = 4096;
                    std::vector<float> out(cap);                                         // exactly cap floats: a write past it is a finding
                    uint32_t n2 = 0;
                    EXPECT(aidax_ir_resample(in.data(), n_in, pr[0], pr[1], lead, out.data(), cap, &n2) == AIDAX_OK && n2 == n_full);
                    for (uint32_t i = 0; i < cap && i < n_full; ++i) {
                        EXPECT(std::isfinite(out[i]));
                        sum += out[i];
                    }
                    ++calls;
                }
            }
    // refused arguments write nothing and report a length of 0
    std::vector<float> out(16, 7.f);
    uint32_t n = 99;
    EXPECT(aidax_ir_resample(nullptr, 4, 48000, 44100, 0, out.data(), 16, &n) == AIDAX_ERR_ARG);
    EXPECT(aidax_ir_resample(in.data(), 4, 48000, 44100, 0, out.data(), 16, nullptr) == AIDAX_ERR_ARG);
    EXPECT(aidax_ir_resample(in.data(), 4, 48000, 44100, 0, nullptr, 16, &n) == AIDAX_ERR_ARG && n == 0);
    EXPECT(aidax_ir_resample(in.data(), 0, 48000, 44100, 0, out.data(), 16, &n) == AIDAX_ERR_ARG);
    EXPECT(aidax_ir_resample(in.data(), 4, 48000.5, 44100, 0, out.data(), 16, &n) == AIDAX_ERR_ARG);
    EXPECT(aidax_ir_resample(in.data(), 4, 48000, -1, 0, out.data(), 16, &n) == AIDAX_ERR_ARG);
    EXPECT(aidax_ir_resample(in.data(), 4, std::numeric_limits<double>::quiet_NaN(), 44100, 0, out.data(), 16, &n) == AIDAX_ERR_ARG);
    EXPECT(aidax_ir_resample(in.data(), 4, 48000, std::numeric_limits<double>::infinity(), 0, out.data(), 16, &n) == AIDAX_ERR_ARG);
    EXPECT(aidax_ir_resample(in.data(), 4, 1e300, 44100, 0, out.data(), 16, &n) == AIDAX_ERR_ARG);
    EXPECT(aidax_ir_resample(in.data(), 4, 48000, 44100, 1025, out.data(), 16, &n) == AIDAX_ERR_ARG);
    std::vector<float> bad(in.begin(), in.begin() + 8);
    bad[5] = std::numeric_limits<float>::infinity();
    EXPECT(aidax_ir_resample(bad.data(), 8, 48000, 44100, 0, out.data(), 16, &n) == AIDAX_ERR_ARG && n == 0);
    for (float v : out) EXPECT(v == 7.f);
    // the packer at 65536 taps: 4098 diagonals, 12.6 MB of fragments
    std::vector<float> h(65536);
    for (size_t k = 0; k < h.size(); ++k) h[k] = in[k % in.size()];
    uint32_t n_diag = 0;
    const std::vector<uint32_t> frag = aidax::pack_ir_fragments(h.data(), 65536, &n_diag);
    EXPECT(n_diag == 4098 && frag.size() == size_t(4098) * 3 * 64 * 4);
    uint32_t n_diag2 = 0;
    const size_t words = aidax::pack_ir_fragments(h.data(), 8193, &n_diag2).size();
    EXPECT(n_diag2 == 514 && words == size_t(514) * 768);
    main_section_cases();
    for (uint32_t pool : { 1u, 65u, 300u })
        for (int fade_mode = 0; fade_mode < 3; ++fade_mode) fade_section_cases(pool, fade_mode);
    EXPECT(plan_rebuilds > 1000);
    std::printf("asan_ir_harness: %d resample calls, checksum %.9g, %d plan rebuilds, %d failures\n", calls, sum, plan_rebuilds, failures);
    return failures ? 1 : 0;
}
