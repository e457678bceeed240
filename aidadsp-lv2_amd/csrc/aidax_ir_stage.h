// aidax_ir_stage.h — the cabinet IR stage of a pool: IrPlan, its host-only half (aidax_ir.cpp: which stream goes through which IR, and
// the work items k_ir_conv runs for that), and IrStage, the device half around it (aidax_ir_stage.cpp: the history, the uploads, the launches).
#pragma once

#include <algorithm>
#include <atomic>
#include <cstdint>
#include <vector>

#include "aidax_internal.h"
#include "aidax_kernels.h"

namespace aidax {

// One IR's content on the device (aidax_pool_prepare_ir / aidax_pool_commit_ir): its A fragments for k_ir_conv, swapped in and out like a model.
struct IrSlot {
    uint32_t* d_frag = nullptr;      // nullptr: no IR
    uint32_t n_taps = 0, n_diag = 0;
    uint64_t gen = 0;                // which committed content this is (a number per commit, given by the commit; 0: none): the IR fade's identity of an IR
};

// One section of the plan: IRs with the streams that go through them, as items of up to kIrItemStreams streams — the IRs in source
// order, each IR's streams in stream order (items[i] lists streams[first .. first + count - 1]). Host memory sized at creation.
struct IrSection {
    std::vector<IrItem> items;
    std::vector<uint32_t> streams;       // [n_streams]
    uint32_t n_items = 0, n_listed = 0, max_diag = 0;
    void clear() { n_items = n_listed = max_diag = 0; }
};

// Which IR each stream's output goes through (AIDAX_IR_POOL, AIDAX_IR_NONE or a bank slot), and the plan built from it on the audio
// side whenever an assignment or a commit has changed it. An IR's key: 0 the pool IR, 1 + j bank slot j. One IR for every stream gives
// the identity plan (item i: streams 64 i ..). No HIP call in here.
//
// The IR fade (`fade` frames; 0: off). Every commit gives its content a generation number, and a stream records the (key, generation)
// of the IR it went through in the last pass issued (-1 / 0: none). A rebuild that finds another one in force for a stream adds the
// stream to the fade-out section: the old IRs (still live, or parked, see commit) with the streams fading from them, and to the mix list
// (k_ir_fade: stream index, kIrFadeDry set where the old side is the dry block). That section serves the one pass it was built for:
// pass_issued() ends it, and so does spend_fade() for a pass that failed on its way.
//
// The blend (include/aidax.h, "IR blend"). A stream has a second assignment B and a mix, the weight of B, that ramps over the frames
// issued for the stream (Ramp). A stream whose coming frames all carry a weight of exactly 0 or 1 is at rest: it is listed once, in the
// main section, under A or under B (eff_key), like any one-IR stream. Every other stream is blended: in `main` under A, in the `blend`
// section under B (live slots only; either side may be nothing: the dry block) and in blend_list with its ramp as the rebuild found it.
// The plan is NOT rebuilt as a ramp moves on: the frames issued since the rebuild travel as k_ir_mix's k_off (since_build, the same for
// every blended stream, since a pass advances them all). It is rebuilt when a blended stream comes to rest on 0 or 1 (stale()), after
// set_mix and assignments of B, and after a prefix pass that left a blended stream out (advance). A stream that is blended in the last
// pass issued or in this one never joins the fade-out section.
struct IrPlan {
    static constexpr int kKeys = AIDAX_IR_SLOTS + 1;
    uint32_t n_streams = 0;
    std::vector<int32_t> assign;             // [n_streams]
    IrSlot live[kKeys];                      // d_frag == nullptr: empty
    IrSlot parked[kKeys];                    // per key: the content retired last, kept for the streams that still fade from it
    uint64_t gen_next = 1;
    uint64_t pass_seq = 0;                   // passes issued through the stage
    uint64_t commit_seq[kKeys] = {};         // ... when the key's content was committed: smaller than pass_seq = it has been played
    std::vector<int8_t> played_key;          // [n_streams]
    std::vector<uint64_t> played_gen;        // [n_streams]
    uint32_t fade = 0;
    IrSection main, fade_out;                // items: [ceil(n_streams / 64) + 65] and [ceil(n_streams / 64) + 2 * 65]
    std::vector<uint32_t> mix;               // [n_streams]
    uint32_t n_mix = 0;
    bool identity = false, dirty = true;
    // a ramp m0 -> m1 over `len` frames, `k` of which have been issued (saturating at max(len, 1): frames_left() == 0); `now` is the
    // weight of the last frame issued. Ramp frame k carries m1 once k + 1 >= len, so a ramp of 0 or 1 frames is a jump at the boundary.
    struct Ramp { float m0 = 0.f, m1 = 0.f, now = 0.f; uint32_t len = 0, k = 1; };
    std::vector<int32_t> assign_b;           // [n_streams]
    std::vector<Ramp> ramp;                  // [n_streams]
    std::vector<uint8_t> was_blended;        // [n_streams]: blended in the plan of the last rebuild
    IrSection blend;                         // items: [ceil(n_streams / 64) + 65]
    std::vector<IrBlendEntry> blend_list;    // [n_streams]
    uint32_t n_blend = 0;
    uint32_t since_build = 0;                // frames issued since the rebuild, while streams are blended (saturating at kIrMaxRampOffset)
    uint32_t rest_in = 0;                    // ... at which the first blended stream comes to rest on 0 or 1 (0: none will)
    uint32_t blend_hi = 0;                   // the last blended stream
    uint32_t n_moving = 0;                   // streams with frames_left() != 0

    void init(uint32_t n);
    int key(uint32_t s) const                // the key of the IR stream s goes through; -1: none (also an empty slot)
    {
        static_assert(AIDAX_IR_POOL == -1 && AIDAX_IR_NONE == -2, "an assignment is its key - 1");
        const int k = 1 + assign[s];
        return k >= 0 && live[k].d_frag ? k : -1;
    }
    int key_b(uint32_t s) const
    {
        const int k = 1 + assign_b[s];
        return k >= 0 && live[k].d_frag ? k : -1;
    }
    uint32_t frames_left(uint32_t s) const { return std::max(ramp[s].len, 1u) - ramp[s].k; }
    // 0 / 1: every coming frame of the stream has exactly that weight (at rest on A / on B); -1: the stream is blended
    int rest(uint32_t s) const
    {
        const Ramp& r = ramp[s];
        if (frames_left(s) > 1u) return -1;
        return r.m1 == 0.f ? 0 : r.m1 == 1.f ? 1 : -1;
    }
    int eff_key(uint32_t s) const { return rest(s) == 1 ? key_b(s) : key(s); }       // a stream at rest: its effective IR
    // the weight of ramp frame k (ramp_value, aidax_kernels.h: the statement k_ir_mix computes with)
    static float weight(const Ramp& r, uint32_t k)
    {
        return static_cast<float>(ramp_value(r.m0, r.m1, r.len, k));
    }
    // aidax_pool_set_ir_mix for one stream: a ramp from the weight of the last frame issued; between equal weights it has ended already
    void set_mix(uint32_t s, float mix, uint32_t len);
    // the sections for the pass about to be issued, and every stream's played record brought up to that pass
    void rebuild(bool any_pass);
    // has a blended stream of the plan come to rest on 0 or 1 with the frames issued since the rebuild?
    bool stale() const { return n_blend != 0 && rest_in != 0 && since_build >= rest_in; }
    void pass_issued() { ++pass_seq; spend_fade(); }
    // ... of n_frames for the first n_active streams: their ramps move on
    void pass_issued(uint32_t n_active, uint32_t n_frames) { pass_issued(); advance(n_active, n_frames); }
    void advance(uint32_t n_active, uint32_t n_frames);
    void spend_fade() { fade_out.clear(); n_mix = 0; }
    // the host half of aidax_pool_commit_ir: `staged` becomes the content of `key` and gets back what is to be freed
    void commit(int key, IrSlot& staged);

    // The plan's bytes on the device and in a snapshot: the main section's items and stream list, then (8-byte aligned) the fade-out
    // section's, then the mix list. serialise() writes what the sections hold and returns the length to upload from the snapshot's start.
    size_t plan_items_bytes() const { return main.items.size() * sizeof(IrItem); }
    size_t fade_items_off() const { return (plan_items_bytes() + sizeof(uint32_t) * n_streams + 7u) & ~size_t(7); }
    size_t fade_streams_off() const { return fade_items_off() + fade_out.items.size() * sizeof(IrItem); }
    size_t fade_mix_off() const { return fade_streams_off() + sizeof(uint32_t) * n_streams; }
    size_t plan_bytes() const { return fade_mix_off() + sizeof(uint32_t) * n_streams; }
    // ... and behind them, in a plan with blended streams only, the blend section's items and stream list and the blend list
    size_t blend_items_off() const { return (plan_bytes() + 7u) & ~size_t(7); }
    size_t blend_streams_off() const { return blend_items_off() + blend.items.size() * sizeof(IrItem); }
    size_t blend_list_off() const { return blend_streams_off() + sizeof(uint32_t) * n_streams; }
    size_t total_bytes() const { return blend_list_off() + sizeof(IrBlendEntry) * n_streams; }
    size_t serialise(uint8_t* snapshot) const;

  private:
    std::vector<int16_t> src;                // [n_streams]: scratch of rebuild, each stream's source in the section being grouped
    // source k of a section: live[k] for k < kKeys, parked[k - kKeys] behind them
    const IrSlot& source(int k) const { return k < kKeys ? live[k] : parked[k - kKeys]; }
    uint32_t group(IrSection& sec, int n_sources);
};

struct IrHistory;

// The device half. The history (per stream a ring of dry samples, the K split's partial sums, the fade's side buffer, the device copy
// of the plan and the pinned snapshots it is uploaded from) is allocated by the first prepare and published ONCE by the worker side;
// the audio side picks it up at its next call (adopt) and owns everything else in here. Every function but prepare, capacity and
// has_history is the audio side's; HIP failures leave as HipFail.
struct IrStage {
    IrPlan plan;

    void init(uint32_t n_streams, uint32_t max_frames, int cus, hipStream_t worker)
    {
        max_frames_ = max_frames; cus_ = cus; wq_ = worker;
        plan.init(n_streams);
    }
    ~IrStage();                                              // (aidax_ir_stage.cpp: the history and the fragments go back)
    // the longest IR the stage takes (aidax_pool_set_ir_capacity, set-up side: fixed once the first prepare has sized the history with it)
    std::atomic<uint32_t> capacity{kIrMaxTaps};
    bool has_history() const { return pub_.load(std::memory_order_acquire) != nullptr; }
    // worker side: the history on first use (allocated, zeroed, published), then the IR's fragments packed and uploaded (taps == nullptr: none)
    void prepare(const float* taps, uint32_t n_taps, IrSlot& out);
    // a swap of host records behind `fence`, recorded on q: no allocation, no free, no wait
    void commit(int32_t slot, IrSlot& staged, hipEvent_t fence, hipStream_t q);
    // is there a history (from now on every pass of n_frames > 0 goes through begin_pass and issue)?
    bool adopt() { return hist_ || (hist_ = pub_.load(std::memory_order_acquire)); }
    // ahead of the pass's model launch: a dirty plan rebuilt and uploaded, stream-ordered with the passes that follow. A fade-out
    // section that a failed pass left behind is dropped here (a later pass, with another n_frames and ring position, must not run it)
    void begin_pass(hipStream_t s, bool any_pass)
    {
        plan.spend_fade();
        if (plan.stale()) plan.dirty = true;                 // a ramp has ended on 0 or 1: that stream is a one-IR stream from this pass on
        if (plan.dirty) flush_plan(s, any_pass);
    }
    // behind it: the block's dry samples into the history, the convolution in place on d_out, the fade-out section and its mix, the
    // blend section and its mix; the ramps of the pass's streams move on by n_frames
    void issue(hipStream_t s, float* d_out, uint32_t n_active, uint32_t n_frames);
    void clear_stream(uint32_t stream, hipStream_t q);       // one stream's past, if there is a history
    void clear_all(hipStream_t q);                           // every stream's (errors ignored: the k_mfma_lp give-up path)

  private:
    uint32_t max_frames_ = 0;
    int cus_ = 0;
    hipStream_t wq_ = nullptr;
    std::atomic<IrHistory*> pub_{nullptr};
    IrHistory* hist_ = nullptr;
    uint32_t pos_ = 0;                       // the ring slot of the next pass's first frame
    void flush_plan(hipStream_t s, bool any_pass);
    IrArgs conv_args(const IrSection& sec, size_t items_off, size_t streams_off, float* out, uint32_t n_active, uint32_t n_frames) const;
};

}  // namespace aidax
