// The IR blend's host side under AddressSanitizer + UndefinedBehaviorSanitizer (`make asan_ir_blend`, tests/test_asan_ir_blend.py): IrPlan
// driven as IrStage drives it (begin_pass: spend_fade, stale, rebuild; issue: pass_issued with the pass's streams and frames) over seeded
// random sequences of assignments of A and B, mixes, commits, fade-length changes and passes of 0, 1, 17, 64 and 256 frames, whole and
// prefix, against a direct restatement of the rules of include/aidax.h, "IR blend" and "IR fade". CPU only: device pointers are made-up
// numbers, nothing is dereferenced.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "aidax.h"
#include "../aidadsp-lv2_amd/csrc/aidax_ir_stage.h"

namespace aidax {
uint32_t ir_diagonals(uint32_t n_taps) { return (n_taps + 30u) / 16u + 1u; }
bool model_supported(const aidax_model&) { return true; }
}  // namespace aidax

static int failures = 0;
#define EXPECT(c) do { if (!(c)) { if (failures < 40) std::fprintf(stderr, "asan_ir_blend_harness: %s failed at line %d\n", #c, __LINE__); ++failures; } } while (0)

using aidax::IrBlendEntry;
using aidax::IrItem;
using aidax::IrPlan;
using aidax::IrSection;
using aidax::IrSlot;
constexpr int kKeys = AIDAX_IR_SLOTS + 1;

static uint32_t lcg_state = 88172645u;
static uint32_t rnd(uint32_t n) { lcg_state = lcg_state * 1664525u + 1013904223u; return (lcg_state >> 8) % n; }

struct Content { uint32_t* frag = nullptr; uint32_t n_diag = 0; uint64_t gen = 0; };
static Content fresh_content()
{
    static uintptr_t next = 0x10000;
    next += 0x1000;
    return Content{ reinterpret_cast<uint32_t*>(next), 3 + rnd(4000), 0 };
}

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

// serialise() into a snapshot of exactly total_bytes(): today's bytes at today's offsets, the blend's behind plan_bytes(), nothing else
static std::vector<uint8_t> expect_snapshot(const IrPlan& plan, size_t* length)
{
    const size_t n = plan.n_streams, runs = (n + 63) / 64;
    const size_t streams_off = (runs + kKeys) * sizeof(IrItem), fade_items = (streams_off + 4 * n + 7) / 8 * 8;
    const size_t fade_streams = fade_items + (runs + 2 * kKeys) * sizeof(IrItem), fade_mix = fade_streams + 4 * n, old_total = fade_mix + 4 * n;
    const size_t blend_items = (old_total + 7) / 8 * 8, blend_streams = blend_items + (runs + kKeys) * sizeof(IrItem), blend_list = blend_streams + 4 * n;
    const size_t total = blend_list + sizeof(IrBlendEntry) * n;
    EXPECT(plan.plan_bytes() == old_total && plan.blend_items_off() == blend_items && plan.blend_streams_off() == blend_streams &&
           plan.blend_list_off() == blend_list && plan.total_bytes() == total);
    std::vector<uint8_t> snap(plan.total_bytes(), 0xEE), want(plan.total_bytes(), 0xEE);
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
    if (plan.n_blend) {
        std::memcpy(want.data() + blend_items, plan.blend.items.data(), plan.blend.n_items * sizeof(IrItem));
        std::memcpy(want.data() + blend_streams, plan.blend.streams.data(), plan.blend.n_listed * 4);
        std::memcpy(want.data() + blend_list, plan.blend_list.data(), plan.n_blend * sizeof(IrBlendEntry));
        end = blend_list + plan.n_blend * sizeof(IrBlendEntry);
    } else {
        EXPECT(bytes <= old_total);
    }
    EXPECT(bytes == end && bytes <= total && snap == want);
    *length = bytes;
    return snap;
}

static int key_of(int32_t a) { return a == AIDAX_IR_POOL ? 0 : a >= 0 ? 1 + a : -1; }

// a stream's mix as the rules state it: `issued` frames since the ramp was set, never clipped
struct Mix {
    float m0 = 0.f, m1 = 0.f, now = 0.f;
    uint32_t R = 0;
    uint64_t issued = 1;
    uint64_t span() const { return R > 1 ? R : 1; }
    uint64_t left() const { return span() > issued ? span() - issued : 0; }
    int rest() const { return left() > 1 ? -1 : m1 == 0.f ? 0 : m1 == 1.f ? 1 : -1; }
    float weight(uint64_t k) const
    {
        if (k + 1 >= R) return m1;
        const double wd = (double)m0 + ((double)m1 - (double)m0) * (double)(k + 1) / (double)R;
        return (float)wd;
    }
    void set(float mix, uint32_t ramp)
    {
        m0 = now; m1 = mix; R = ramp; issued = 0;
        if (m0 == m1) { R = 0; issued = 1; }
    }
    void advance(uint32_t n)
    {
        if (n == 0 || left() == 0) return;
        issued += n;
        now = weight(std::min<uint64_t>(issued, span()) - 1);
    }
};

static int plan_rebuilds = 0, clean_ramp_passes = 0, rests = 0, prefix_rebuilds = 0, blended_fade_passes = 0;

// blend_mode 0: no blend call at all, and a second plan driven through the members of before the blend only must serialise the same bytes;
// 1: every operation
static void sequence(uint32_t n, int blend_mode, int steps)
{
    IrPlan plan, twin;
    plan.init(n);
    twin.init(n);
    std::vector<Content> live(kKeys), parked(kKeys);
    std::vector<bool> pass_since_commit(kKeys, false);
    std::vector<int> played_key(n, -1);
    std::vector<uint64_t> played_gen(n, 0);
    std::vector<bool> was_blended(n, false);
    std::vector<int32_t> A(n, AIDAX_IR_POOL), B(n, AIDAX_IR_NONE);
    std::vector<Mix> mix(n);
    std::vector<uint32_t> listed;                // the blended streams of the plan in force
    uint64_t gen_next = 1;
    bool any_pass = false, touched = true, left_out = false;
    const int keys[] = { 0, 1, 2, 7, 64 };
    const float mixes[] = { 0.f, 1.f, 0.25f, 0.5f, 0.3f, 1.f, 0.f };
    const uint32_t ramps[] = { 0, 1, 2, 17, 100, 700, 3000 };
    const uint32_t lengths[] = { 0, 1, 17, 64, 256 };
    for (int step = 0; step < steps; ++step) {
        const uint32_t op = rnd(16);
        if (rnd(16) == 0) plan.fade = twin.fade = plan.fade ? 0 : 256;
        if (op < 2) {                                                           // a commit: new content, or none, for one key
            const int k = keys[rnd(5)];
            Content c = rnd(5) == 0 ? Content{} : fresh_content();
            if (c.frag) c.gen = gen_next++;
            IrSlot sg{ c.frag, 16 * c.n_diag, c.n_diag, 0 }, sg2 = sg;
            plan.commit(k, sg);
            twin.commit(k, sg2);
            Content back = live[k];
            if (plan.fade != 0 && pass_since_commit[k]) std::swap(back, parked[k]);
            live[k] = c;
            pass_since_commit[k] = false;
            EXPECT(sg.d_frag == back.frag && (!back.frag || sg.gen == back.gen) && plan.dirty);
            touched = true;
        } else if (op < 4) {                                                    // an assignment of A
            const int32_t slot = rnd(4) == 0 ? AIDAX_IR_NONE : keys[rnd(5)] - 1;
            if (rnd(8) == 0) { std::fill(plan.assign.begin(), plan.assign.end(), slot); std::fill(A.begin(), A.end(), slot); }
            else { const uint32_t s = rnd(n); plan.assign[s] = A[s] = slot; }
            twin.assign = plan.assign;
            plan.dirty = twin.dirty = true;
            touched = true;
        } else if (op < 6 && blend_mode) {                                      // ... of B (aidax_pool_assign_ir_b's host half)
            const int32_t slot = rnd(4) == 0 ? AIDAX_IR_NONE : keys[rnd(5)] - 1;
            const uint32_t s = rnd(n);
            if (plan.assign_b[s] != slot) {
                plan.assign_b[s] = B[s] = slot;
                if (plan.rest(s) != 0) plan.dirty = true;
                touched = true;
            }
        } else if (op < 9 && blend_mode) {                                      // a mix, for one stream or for all
            const float m = mixes[rnd(7)];
            const uint32_t R = ramps[rnd(7)];
            const uint32_t lo = rnd(6) == 0 ? 0 : rnd(n), hi = lo == 0 && rnd(3) == 0 ? n : lo + 1;
            for (uint32_t s = lo; s < hi; ++s) {
                plan.set_mix(s, m, R);
                mix[s].set(m, R);
                EXPECT(plan.ramp[s].m0 == mix[s].m0 && plan.ramp[s].m1 == m && plan.ramp[s].now == mix[s].now && plan.frames_left(s) == mix[s].left());
            }
            touched = true;
        } else {                                                                // a pass, as IrStage::begin_pass and issue drive the plan
            const uint32_t frames = lengths[rnd(5)];
            const uint32_t n_active = blend_mode && rnd(10) == 0 ? 1 + rnd(n) : n;
            if (frames == 0) {                                                  // (the pool does not enter the stage; the plan's own guard)
                plan.advance(n_active, 0);
                for (uint32_t s = 0; s < n; ++s) EXPECT(plan.frames_left(s) == mix[s].left() && plan.ramp[s].now == mix[s].now);
                continue;
            }
            plan.spend_fade();
            twin.spend_fade();
            if (plan.stale()) plan.dirty = true;
            const bool rebuilt = plan.dirty;
            if (rebuilt) { plan.rebuild(any_pass); ++plan_rebuilds; }
            if (twin.dirty) twin.rebuild(any_pass);
            // the blended streams by the rules; a plan that was not rebuilt must still hold exactly them
            std::vector<uint32_t> blended;
            for (uint32_t s = 0; s < n; ++s)
                if (mix[s].rest() < 0) blended.push_back(s);
            if (!touched && !left_out && blended == listed) { EXPECT(!rebuilt); if (!blended.empty() && plan.n_moving) ++clean_ramp_passes; }
            if (!rebuilt) EXPECT(blended == listed);
            if (rebuilt && !touched && !left_out) { EXPECT(blended.size() < listed.size()); ++rests; }
            if (rebuilt && left_out) ++prefix_rebuilds;
            std::vector<int> main_of(n, -1), fade_of(n, -1), blend_of(n, -1);
            std::vector<uint32_t> fmix;
            std::vector<bool> in_fade(n, false), in_blend(n, false);
            size_t at = 0;
            for (uint32_t s = 0; s < n; ++s) {
                const int ka = key_of(A[s]), kb = key_of(B[s]);
                const int la = ka >= 0 && live[ka].frag ? ka : -1, lb = kb >= 0 && live[kb].frag ? kb : -1;
                const int r = mix[s].rest();
                const int nk = r == 1 ? lb : la;
                const uint64_t ng = nk >= 0 ? live[nk].gen : 0;
                main_of[s] = nk;
                if (r < 0) {
                    blend_of[s] = lb;
                    in_blend[s] = true;
                    // the list entry: the ramp as the rebuild found it; with the frames issued since, where the stream is now
                    EXPECT(at < plan.n_blend);
                    if (at < plan.n_blend) {
                        const IrBlendEntry& e = plan.blend_list[at++];
                        EXPECT(e.stream == (s | (lb < 0 ? aidax::kIrBlendDry : 0u)) && e.m0 == mix[s].m0 && e.m1 == mix[s].m1 && e.ramp == mix[s].R);
                        EXPECT(std::min<uint64_t>(uint64_t(e.k) + plan.since_build, mix[s].span()) == std::min<uint64_t>(mix[s].issued, mix[s].span()));
                    }
                } else {
                    // at rest on 0 or 1: once in main under the right key (restated below), in no other section
                    EXPECT(plan.eff_key(s) == nk);
                }
                if (!rebuilt) continue;
                const int ok = played_key[s];
                const uint64_t og = played_gen[s];
                const bool hand_over = r < 0 || was_blended[s];
                played_key[s] = nk;
                played_gen[s] = ng;
                was_blended[s] = r < 0;
                if (!any_pass || plan.fade == 0 || hand_over || (nk == ok && ng == og)) continue;
                if (ok < 0) { fmix.push_back(s | aidax::kIrFadeDry); in_fade[s] = true; }
                else if (live[ok].frag && live[ok].gen == og) { fade_of[s] = ok; fmix.push_back(s); in_fade[s] = true; }
                else if (parked[ok].frag && parked[ok].gen == og) { fade_of[s] = kKeys + ok; fmix.push_back(s); in_fade[s] = true; }
            }
            EXPECT(at == plan.n_blend && plan.n_blend == blended.size());
            expect_section(plan.main, restate(main_of, live));
            expect_section(plan.blend, restate(blend_of, live));
            std::vector<Content> sources(live);
            sources.insert(sources.end(), parked.begin(), parked.end());
            expect_section(plan.fade_out, restate(fade_of, sources));
            EXPECT(plan.n_mix == fmix.size() && std::equal(fmix.begin(), fmix.end(), plan.mix.begin()));
            for (uint32_t i = 0; i < plan.n_mix; ++i) EXPECT(!in_blend[plan.mix[i] & ~aidax::kIrFadeDry]);
            for (uint32_t s = 0; s < n; ++s) EXPECT(!(in_fade[s] && in_blend[s]));
            if (plan.n_mix && plan.n_blend) ++blended_fade_passes;
            size_t bytes = 0, twin_bytes = 0;
            const std::vector<uint8_t> snap = expect_snapshot(plan, &bytes);
            if (!blend_mode) {
                const std::vector<uint8_t> other = expect_snapshot(twin, &twin_bytes);
                EXPECT(bytes == twin_bytes && snap == other && bytes <= plan.plan_bytes());
            }
            listed = blended;
            touched = false;
            if (rebuilt) left_out = false;
            if (rnd(12) == 0) {                                                 // the pass failed on its way: nothing moves
                for (uint32_t s = 0; s < n; ++s) EXPECT(plan.frames_left(s) == mix[s].left() && plan.ramp[s].now == mix[s].now);
                continue;
            }
            plan.pass_issued(n_active, frames);
            twin.pass_issued();
            for (uint32_t s = 0; s < n_active; ++s) mix[s].advance(frames);
            for (uint32_t s = 0; s < n; ++s) EXPECT(plan.frames_left(s) == mix[s].left() && plan.ramp[s].now == mix[s].now);
            // a prefix pass that left a blended stream out: the plan's common frame offset no longer holds for it
            if (!blended.empty() && blended.back() >= n_active) { left_out = true; EXPECT(plan.dirty); }
            EXPECT(plan.fade_out.n_items == 0 && plan.fade_out.n_listed == 0 && plan.n_mix == 0);
            any_pass = true;
            pass_since_commit.assign(kKeys, true);
        }
    }
}

int main()
{
    // the weights by hand: 0 -> 1 over 4 frames, cut 2 + 4; a jump; the state a stream starts in
    {
        IrPlan plan;
        plan.init(3);
        EXPECT(plan.rest(0) == 0 && plan.frames_left(0) == 0 && plan.ramp[0].now == 0.f && plan.n_moving == 0);
        plan.dirty = false;
        plan.set_mix(0, 0.f, 100);                                              // between equal weights: ended, and at rest as before
        EXPECT(!plan.dirty && plan.frames_left(0) == 0);
        plan.set_mix(0, 1.f, 4);
        EXPECT(plan.dirty && plan.frames_left(0) == 4 && plan.rest(0) == -1 && plan.ramp[0].now == 0.f);
        plan.advance(3, 2);
        EXPECT(plan.ramp[0].now == 0.5f && plan.frames_left(0) == 2);
        plan.advance(3, 1);
        EXPECT(plan.ramp[0].now == 0.75f && plan.frames_left(0) == 1 && plan.rest(0) == 1);      // the one frame to come carries 1
        plan.advance(3, 4);
        EXPECT(plan.ramp[0].now == 1.f && plan.frames_left(0) == 0 && plan.n_moving == 0);
        plan.set_mix(1, 0.3f, 0);                                               // a jump: in force from the next frame, reported until then
        EXPECT(plan.frames_left(1) == 1 && plan.ramp[1].now == 0.f && plan.rest(1) == -1);
        plan.set_mix(1, 1.f, 0);                                                // the last call wins, from the same m0
        EXPECT(plan.ramp[1].m0 == 0.f && plan.rest(1) == 1);
        plan.advance(3, 0);
        EXPECT(plan.frames_left(1) == 1);
        plan.advance(3, 1);
        EXPECT(plan.frames_left(1) == 0 && plan.ramp[1].now == 1.f);
    }
    for (uint32_t pool : { 1u, 7u, 65u, 200u })
        for (int mode = 0; mode < 2; ++mode) sequence(pool, mode, 3000);
    EXPECT(plan_rebuilds > 1000);
    EXPECT(clean_ramp_passes > 100 && rests > 20 && prefix_rebuilds > 5 && blended_fade_passes > 5);
    std::printf("asan_ir_blend_harness: %d plan rebuilds, %d clean passes of running ramps, %d rests, %d prefix rebuilds, %d passes with fade-out and blend, %d failures\n",
                plan_rebuilds, clean_ramp_passes, rests, prefix_rebuilds, blended_fade_passes, failures);
    return failures ? 1 : 0;
}
