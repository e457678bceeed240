// aidax_pool.h — the stream pool's own types, shared by its four sources: aidax_pool.cpp (the core: launch — the
// executor of a PassForm —, the pass and the order of its stages, create / destroy, controls and stream state), aidax_pool_stages.cpp (the
// C ABI of the opt-in stages: meters, gate, tuners, buses, bus limiters, bus reverbs, stream delays), aidax_pool_model.cpp (everything that
// builds or commits an aidax_staged) and aidax_pool_io.cpp (the host-buffer entry points). Which kernels serve a pass is decided in ONE
// place, the HIP-free aidax_pass_form.h: a slot carries the SlotForm that choose_form gave it, aidax_pool::pass_form gathers the facts (and
// reads the per-call hooks), and launch, aidax_pool_kernel_name and aidax_pool_process all read the PassForm it returns. Private to the four sources.
// Issues HIP calls: include it last, like aidax_model_bank.h.
#pragma once

#include <algorithm>
#include <atomic>
#include <cstdlib>
#include <memory>
#include <mutex>

#include "aidax_ir_stage.h"
#include "aidax_model_bank.h"
#include "aidax_stream_stages.h"
#include "aidax_mix_stage.h"
#include "aidax_limit_stage.h"
#include "aidax_reverb_stage.h"
#include "aidax_delay_stage.h"

namespace aidax {

constexpr uint32_t kWarmupFrames = 2048;        // rt-neural-generic.cpp:1077
constexpr uint32_t kMaxFrames = 8192;           // LDS block buffer bound (32 KiB)
bool model_supported(const aidax_model& m);      // which models have a device path (aidax_pool.cpp)

// the streams or buses [lo, hi) of n that a call names by one index or by AIDAX_ALL_STREAMS / AIDAX_ALL_BUSES; false: out of range
static_assert(static_cast<int>(AIDAX_ALL_STREAMS) == static_cast<int>(AIDAX_ALL_BUSES), "one 'all' value for both");
inline bool named_range(int32_t index, uint32_t n, uint32_t* lo, uint32_t* hi)
{
    if (index != AIDAX_ALL_STREAMS && (index < 0 || static_cast<uint32_t>(index) >= n)) return false;
    *lo = index == AIDAX_ALL_STREAMS ? 0u : static_cast<uint32_t>(index);
    *hi = index == AIDAX_ALL_STREAMS ? n : *lo + 1u;
    return true;
}

// a flag written on the launch path and read by other threads (aidax_pool_kernel_name, lp_in_use from the worker): an atomic that
// a struct assignment of its owner (a model swap is one) may copy
struct RelaxedFlag {
    std::atomic<bool> v{false};
    RelaxedFlag() = default;
    RelaxedFlag(const RelaxedFlag& o) : v(o.v.load(std::memory_order_relaxed)) {}
    RelaxedFlag& operator=(const RelaxedFlag& o) { v.store(o.v.load(std::memory_order_relaxed), std::memory_order_relaxed); return *this; }
    RelaxedFlag& operator=(bool b) { v.store(b, std::memory_order_relaxed); return *this; }
    operator bool() const { return v.load(std::memory_order_relaxed); }
};

// k_mfma_lp needs every workgroup of its grid resident at once, which the pool can promise only for ONE grid on the
// device: one pool per device holds the right to use the kernel (a pool's staged model shares its own pool's hold), the
// others serve their stacked models with k_mfma. Process-wide; another process on the same GPU is beyond its reach
// and ends in a reported give-up (aidax_mfmalp.hip, aidax_mfmals.h).
struct LpGate {
    std::mutex mu;
    // `off`: the owner's "I have stopped using the kernel" flag (a pool whose hand-over gave up serves its model with
    // k_mfma from then on): a hold whose owner has raised it is void, the next pool that asks takes the device over
    struct Hold { const void* owner = nullptr; int refs = 0; const std::atomic<bool>* off = nullptr; } dev[64];
    bool acquire(int device, const void* owner, const std::atomic<bool>* off = nullptr)
    {
        if (device < 0 || device >= 64) return false;
        std::lock_guard<std::mutex> g(mu);
        Hold& h = dev[device];
        if (h.refs != 0 && h.owner != owner) {
            if (!(h.off && h.off->load(std::memory_order_relaxed))) return false;
            h.refs = 0;                                    // (the old owner's later release() no longer matches and is ignored)
        }
        h.owner = owner;
        h.off = off;
        ++h.refs;
        return true;
    }
    void release(int device, const void* owner)
    {
        if (device < 0 || device >= 64) return;
        std::lock_guard<std::mutex> g(mu);
        Hold& h = dev[device];
        if (h.owner == owner && h.refs > 0 && --h.refs == 0) { h.owner = nullptr; h.off = nullptr; }
    }
};
LpGate& lp_gate();                     // (the one instance: aidax_pool.cpp)

// The device side of one loaded model: what the reference keeps in a DynamicModel (rt-neural-generic.h:115-129)
// minus the per-stream members. A pool plays `cur`; aidax_pool_prepare_model builds the next one on the worker
// thread and aidax_pool_commit_model swaps the two on the audio thread (moves of host fields and owners: no HIP call). Move-only.
struct ModelSlot {
    bool has_model = false;
    enum Kind { TABLE = 0, STACK = 1, CONV = 2, MFMA = 3, QUAD = 4 } kind = TABLE;
    QuadDesc qdesc{};
    StackDesc sdesc{};
    MfmaDesc mdesc{};
    ConvDesc cdesc{};
    SlotForm form;                   // how the model's passes are served (aidax_pass_form.h; choose_form decides it, nothing changes it afterwards)
    const KernelEntry* kernel = nullptr;
    int cell = 0, input_size = 1, input_skip = 0, hidden = 0;
    float in_gain = 1.f, out_gain = 1.f, model_sr = 48000.f;
    uint32_t nn_stride = 0;
    DevBuf<float> d_wq4;             // k_lstm_q4's weight record (LSTM-32 snapshot models), next to the table kernels' d_wpack
    DevBuf<float> d_wpack;           // weights in the kernel's layout
    DevBuf<float> d_nn;              // recurrent state [n_streams][nn_stride]
    DevBuf<float> d_ring;            // k_mfma_lp: h of layer l-1 on its way to layer l, per stream group
    DevBuf<uint32_t> d_counters;     // k_mfma_lp: frames produced / consumed per (group, layer boundary)
    mutable const void* lp_owner = nullptr;  // the pool whose hold on the device's LpGate this slot shares (it has a d_ring); given up on the launch path when the grid is refused
    mutable RelaxedFlag lp_refused;  // the runtime refused this model's chained grid (cooperative launch: not co-resident on this device): k_mfma serves it — this
                                     // model only; another model of the pool, with a smaller grid, may still fit (set on the launch path, hence mutable)

    float p_den() const { return 0.1f * model_sr; }      // LinearValueSmoother tau * sampleRate (:1053-1054)
    ModelRec rec() const { return model_rec(d_wpack.get(), in_gain, out_gain, input_skip); }      // what a banked stream on this model reads of it
    BankArch arch() const { return { cell, hidden, input_size, model_sr, has_model && kind == TABLE && kernel && kernel->fn_pipe_bank }; }
};

// The end markers of a pass, handed down to the launch that can carry them: the pipelined host path's "pass done" event, the blocking path's completion
// word and the number to write. A launch that takes one clears it and raises its *_taken flag; the caller issues what was not taken behind the pass.
struct PassEnd { hipEvent_t done = nullptr; uint32_t* word = nullptr; uint32_t seq = 0; bool done_taken = false, word_taken = false; };

// The blocking host-buffer path's buffers (aidax_pool_process; alloc: aidax_pool_io.cpp)
struct BlockingIo {
    DevBuf<float> d_in;              // staging for the host-buffer entry point
    DevBuf<float> d_out;
    PinnedBuf<float> h_in;           // pinned host staging (empty: blocks too large, pageable copies)
    PinnedBuf<float> h_out;
    float* hd_in = nullptr;          // device view of h_in / h_out (zero-copy passes)
    float* hd_out = nullptr;
    bool zero_copy = false;
    // completion word of a pass in pinned host memory: the stream writes the pass number behind its last launch and the
    // caller of aidax_pool_process polls it — no interrupt, no wake-up of a blocked thread (small pools: the plugin case)
    PinnedBuf<uint32_t> h_done;
    uint32_t* hd_done = nullptr;
    uint32_t done_seq = 0;
    bool spin_wait = false;
    bool kernel_word = true;         // a one-workgroup pass (k_*_pipe / k_*_pipe4 of a one-stream pool) writes the completion word itself, behind its block:
                                     // no packet follows the pass on its queue — 1.7 us of the LV2 instance's 23 us round trip at 64 frames
                                     // (profiles/r06_host_pipeline.txt). AIDAX_KERNEL_WORD=0: the queue writes it (hipStreamWriteValue32), as in round 5
    void alloc(size_t block_floats, int device);     // (set-up side; reads AIDAX_ZEROCOPY, AIDAX_SPIN_WAIT, AIDAX_KERNEL_WORD)
};

// aidax_pool_submit / aidax_pool_collect: kPipeSets staging sets and two copy streams, so that the upload of the blocks behind
// block k and the download of the blocks in front of it run under the pass of block k (allocated by the first submit).
// THREE sets since round 6: with two, submit(k) has to wait for collect(k - 2), which returns a cross-stream hop and a download
// after pass k - 2 has ended; the upload of k and its own hop then end ~110 us after that — later than pass k - 1 (65 us for a
// cfg2 block) does, and the GPU idles for the difference every block (88 us per block predicted, 83.8 measured in round 3).
// A third set takes the host's round trip off the GPU's critical path: the pass is what is left.
constexpr int kPipeSets = 3;
struct Pipeline {
    Stream q_up, q_down;             // (declared first, destroyed last: behind the sets' blocks and events)
    bool ready = false;
    PinnedBuf<float> h_in[kPipeSets], h_out[kPipeSets];
    DevBuf<float> d_in[kPipeSets], d_out[kPipeSets];
    Event ev_up[kPipeSets], ev_pass[kPipeSets], ev_down[kPipeSets];
    uint32_t frames[kPipeSets] = {};
    float* direct_out[kPipeSets] = {};      // the block's download went straight to this caller buffer (registered): collect() only waits
    uint64_t submitted = 0, collected = 0;
    void alloc(size_t cap_floats);   // (the first submit: not a real-time call) all of it or nothing
};

}  // namespace aidax
using namespace aidax;               // (a private header of four sources that say the same)

// A model on its way into (or out of) a pool. Built by aidax_pool_prepare_model on the worker thread; after
// aidax_pool_commit_model the same object carries what the swap retired, for aidax_staged_free on the worker.
struct aidax_staged {
    int device = 0;
    uint32_t n_streams = 0;
    ModelSlot slot;
    DevBuf<StreamState> d_pst;       // per-stream DynamicModel members of the new model (PARAM smoothers, paramFirstRun), installed by the commit
    Event fence;                     // recorded by the commit: everything that may still touch the retired buffers precedes it
    bool fenced = false;
    enum Payload { MODEL, IR, BANK_SLOT } payload = MODEL;      // what is on its way: `slot`, `ir` (aidax_pool_prepare_ir / _slot) or `bank` (aidax_pool_prepare_model_slot)
    int32_t ir_slot = AIDAX_IR_POOL; // IR: for the pool IR or for this bank slot
    IrSlot ir;                       // (ir.d_frag and bank.d_wpack are the staged object's: records that the books swap, freed by staged_release)
    uint32_t bank_slot = 0;
    BankSlot bank;
};

struct aidax_pool {
    // The two streams are declared first, so they are destroyed last: every block, event and stage below goes back ahead of them, as the
    // hand-written release did it. ~aidax_pool does what is not memory; the members then free themselves in reverse order.
    Stream q;                        // the audio side's stream
    Stream wq;                       // the worker side's stream (prepare)
    int device = 0;
    uint32_t n_streams = 0, max_frames = 0;
    double host_sr = 48000.0;
    float gain_coef = 0.f;
    Event ev_x;                      // edge between two streams that carry passes one after the other
    Event ev_adopt;                  // "everything this pool has issued so far": what a stream of ANOTHER pool waits for before it adopts one of ours
    hipStream_t last_stream = nullptr;

    DevBuf<StreamCtl> d_ctl;
    DevBuf<StreamState> d_st;
    BlockingIo io;                   // aidax_pool_process: staging, zero-copy views and the completion word
    Pipeline pipe;                   // aidax_pool_submit / _collect (allocated by the first submit)
    bool spin_collect = true;        // aidax_pool_collect polls the download's event instead of sleeping on it (AIDAX_SPIN_WAIT=0: off)
    bool keep_warm = false;          // this pool holds a reference on its device's keep-warm thread (AIDAX_KEEP_WARM_US)
    // k_mfma_lp: a word in pinned host memory that a workgroup bumps when a layer hand-over timed out. The pass that did
    // so is wrong; whoever notices reports it, and the pool serves the model with k_mfma from then on (lp_off).
    PinnedBuf<uint32_t> h_lp_fault;
    uint32_t* hd_lp_fault = nullptr;
    mutable std::atomic<bool> lp_off{false};      // (mutable: set from the launch path, a const member function)
    std::atomic<uint32_t> lp_faults{0};
    mutable std::atomic<uint32_t> lp_refusals{0}; // chained grids the runtime refused (the text is in aidax_last_error(); kernel_name says k_mfma from then on)
    bool take_lp_fault()
    {
        if (!h_lp_fault) return false;
        // read-and-clear in ONE atomic step: workgroups bump the word with system-scope atomic adds while we look, and a
        // give-up that landed between a read and a separate store of 0 would go unreported
        if (__atomic_load_n(h_lp_fault.get(), __ATOMIC_RELAXED) == 0) return false;
        if (__atomic_exchange_n(h_lp_fault.get(), 0u, __ATOMIC_ACQ_REL) == 0) return false;
        lp_off.store(true, std::memory_order_relaxed);
        lp_faults.fetch_add(1, std::memory_order_relaxed);
        // the wrong block is in the IR history: clear it, so that it does not sound through the IR's tail (behind every pass issued so far)
        if (ir.adopt()) {
            if (last_stream && last_stream != q && hipEventRecord(ev_x.get(), last_stream) == hipSuccess) (void)hipStreamWaitEvent(q, ev_x.get(), 0);
            last_stream = q;
            ir.clear_all(q);
        }
        return true;
    }

    IrStage ir;                      // the cabinet IR stage behind every pass (aidax_ir_stage.h)
    bool any_pass = false;           // the pool has issued a pass of n_frames > 0 (its first one has nothing for an IR change to fade from)
    MeterStage meter;                // the stream meters on both sides of a pass (aidax_stream_stages.h; nothing until the first aidax_pool_set_metering(1))
    GateStage gate;                  // the noise gate ahead of the model (nothing until the first aidax_pool_set_gate that enables one)
    TunerStage tuner;                // the stream tuners ahead of the model (nothing until the first aidax_pool_set_tuning with parameters)
    DelayStage delay;                // the stream delays behind the IR stage (aidax_delay_stage.h; nothing until the first aidax_pool_set_delays(1, ..))
    MixStage mix;                    // the mix buses behind the last stage (aidax_mix_stage.h; nothing until the first aidax_pool_set_buses with a count)
    ReverbStage reverb;              // the bus reverbs between k_mix and k_bus_limit (aidax_reverb_stage.h; nothing until the first aidax_pool_set_bus_reverbs(1, ..))
    LimitStage limit;                // the bus limiters and bus meters behind k_mix (aidax_limit_stage.h; nothing until the first aidax_pool_set_bus_limiting(1, ..))
    // aidax_pool_register_host: page-locked ranges of the caller's memory (copies to and from them need no staging)
    struct HostRange { char* base; size_t bytes; };
    std::vector<HostRange> host_ranges;
    bool host_registered(const void* ptr, size_t bytes) const
    {
        const char* c = static_cast<const char*>(ptr);
        for (const HostRange& r : host_ranges)
            if (c >= r.base && c + bytes <= r.base + r.bytes) return true;
        return false;
    }

    std::vector<aidax_controls> controls;
    std::vector<uint8_t> loading;
    std::vector<uint8_t> forced_off;                     // the hub parks a stream (raw copy, state does not move) without touching its controls
    std::vector<StreamCtl> h_ctl;
    DirtyRange ctl_dirty;                                // control records to upload
    SnapshotRing ctl_ring;

    ModelSlot cur;
    ModelBankStage bank;             // the model bank (aidax_model_bank.h; nothing until the first aidax_pool_prepare_model_slot)
    int tune = 0;                    // AIDAX_TUNE (measurement switches, see LaunchArgs)
    int cus = 0;                     // compute units of the device (form selection)
    bool packed_fits = false;        // the packed chains' eight rows of max_frames fit their LDS (chain_lds_bytes: set by aidax_pool_create)
    Force force = Force::None;       // AIDAX_KERNEL (test build) overrides the heuristics (A/B testing)

    bool lp_in_use(const ModelSlot& m) const { return chained_usable(m.d_ring && !m.lp_refused, m.mdesc.n_layers >= 2, lp_off.load(std::memory_order_relaxed)); }
    static size_t lds_bytes(const ModelSlot& m, uint32_t n_frames)
    {
        return (static_cast<size_t>((n_frames + 3) & ~3u) + static_cast<size_t>(m.hidden > 0 ? m.hidden + 4 : 4)) * sizeof(float);   // block + h row + spare slot
    }

    // The form of one pass (or warm-up, or bare-model run) of slot m over n_pass_streams streams: the facts resolve_pass decides on. bank_pass:
    // a pass of the playing slot with the model bank in force. (The two hooks are read per call: tests switch forms within one process.)
    PassForm pass_form(const ModelSlot& m, int mode, uint32_t n_frames, uint32_t n_pass_streams, bool bank_pass) const
    {
        const char* p4 = AIDAX_HOOK_ENV("AIDAX_PIPE4");
        const char* p4_min = AIDAX_HOOK_ENV("AIDAX_PIPE4_MIN");
        const bool table = m.has_model && m.kernel;
        PoolFacts pool{};
        pool.n_streams = n_streams; pool.max_frames = max_frames; pool.cus = cus; pool.force = force;
        pool.pipe4_off = p4 && p4[0] == '0'; pool.pipe4_min = p4_min ? atoi(p4_min) : -1;
        pool.bank = bank_pass; pool.lp_off = lp_off.load(std::memory_order_relaxed); pool.packed_fits = packed_fits;
        PassFacts pass{};
        pass.slot = m.form; pass.has = table ? &m.kernel->has : nullptr;
        pass.mode = mode; pass.n_frames = n_frames; pass.n_streams = n_pass_streams; pass.input_size = m.input_size;
        pass.pipe4_lds_ok = table && pipe4_lds_bytes(m.hidden, n_frames, m.input_size) <= 160 * 1024;      // (a CU's LDS)
        pass.ring_ready = m.d_ring && !m.lp_refused; pass.hand_over = m.mdesc.n_layers >= 2;
        pass.conv_st = m.cdesc.st_ok != 0;
        return resolve_pass(pool, pass);
    }
    // ... and of a MODE_CHAIN pass of the playing slot over the whole pool: what aidax_pool_kernel_name names (at max_frames) and aidax_pool_process asks
    PassForm playing_form(uint32_t n_frames) const { return pass_form(cur, MODE_CHAIN, n_frames, n_streams, bank.in_force()); }
    // A give-up of an earlier pass that nobody has collected yet: no further k_mfma_lp / k_mfma_ls launch of a stacked model (its counters are
    // out of step); the word stays for whoever reports it (aidax_pool_sync, the hub). AHEAD of every resolution of a form that launch executes.
    void note_lp_give_up() const { if (h_lp_fault && *static_cast<volatile uint32_t*>(h_lp_fault.get()) != 0) lp_off.store(true, std::memory_order_relaxed); }
    // ... so the form a caller resolves ahead of pool_process_prefix, to hand it in: the one launch would resolve itself
    PassForm resolved_playing_form(uint32_t n_frames) const { note_lp_give_up(); return playing_form(n_frames); }
    void refresh_ctl(uint32_t s)
    {
        build_stream_ctl(controls[s], host_sr, cur.has_model, loading[s] != 0, gain_coef, cur.p_den(), &h_ctl[s]);
        if (forced_off[s]) h_ctl[s].flags &= ~static_cast<uint32_t>(CTL_ENABLED);
        ctl_dirty.mark(s, s);
    }
    void refresh_all()
    {
        // identical controls are the common case: design once, then copy
        for (uint32_t s = 0; s < n_streams; ++s) {
            if (s > 0 && std::memcmp(&controls[s], &controls[s - 1], sizeof(aidax_controls)) == 0 &&
                loading[s] == loading[s - 1]) {
                h_ctl[s] = h_ctl[s - 1];
            } else {
                build_stream_ctl(controls[s], host_sr, cur.has_model, loading[s] != 0, gain_coef, cur.p_den(), &h_ctl[s]);
            }
        }
        for (uint32_t s = 0; s < n_streams; ++s)
            if (forced_off[s]) h_ctl[s].flags &= ~static_cast<uint32_t>(CTL_ENABLED);
        ctl_dirty.mark(0, n_streams - 1);
    }
    // the fields of a control record that depend on the model and on `loading`, without redesigning the filters
    void patch_model_fields(uint32_t s)
    {
        StreamCtl& o = h_ctl[s];
        const aidax_controls& c = controls[s];
        o.master_target = loading[s] ? 0.f : db_to_coeff(c.master_db);                   // :490, :654
        o.p_den = cur.p_den();
        if (cur.has_model && !(c.net_bypass > 0.5f)) o.flags |= CTL_NET_ON;              // :631-632
        else o.flags &= ~static_cast<uint32_t>(CTL_NET_ON);
    }
    // Upload the changed control records, stream-ordered with the pass that follows. The records leave from a
    // ring of pinned snapshots, so the copy is asynchronous and a later set_controls cannot overtake it.
    void flush_ctl(hipStream_t s) { ctl_ring.upload_dirty(d_ctl.get(), h_ctl.data(), ctl_dirty, s); }
    // Passes and control pokes are issued in program order by the audio side but may sit on two streams (the pool's
    // own and one handed to aidax_pool_process_device): moving from one to the other puts an event edge between them.
    void enter_stream(hipStream_t s)
    {
        if (last_stream && last_stream != s) {
            HIP_TRY(hipEventRecord(ev_x.get(), last_stream));
            HIP_TRY(hipStreamWaitEvent(s, ev_x.get(), 0));
        }
        last_stream = s;
    }
    // host side: wait for what the pool has issued on a caller's stream (its own stream is the caller's next wait)
    void sync_issued() { if (last_stream && last_stream != q) HIP_TRY(hipStreamSynchronize(last_stream)); }
    LaunchArgs args(const ModelSlot& m, StreamState* st, const float* in, float* out, uint32_t n_frames, int mode) const
    {
        LaunchArgs a{};
        a.ctl = d_ctl.get(); a.st = st; a.nn = m.d_nn.get();
        a.in = in; a.out = out;
        a.n_streams = n_streams; a.n_frames = n_frames; a.nn_stride = m.nn_stride;
        a.mode = mode; a.input_size = m.input_size;
        apply_model_rec(a, m.rec());
        a.tune = tune;
        return a;
    }
    // frames one launch of the extension kernels may carry (their LDS planes grow with n)
    uint32_t ext_chunk() const { return max_frames < 256 ? max_frames : 256; }
    uint32_t launch_chunk(const ModelSlot& m, uint32_t n) const
    {
        // (MFMA: k_mfma takes any length, but a 2048-frame warm-up launch would hold its CUs for ~10 ms next to the passes)
        return (m.kind == ModelSlot::STACK || m.kind == ModelSlot::CONV || m.kind == ModelSlot::MFMA) ? std::min(ext_chunk(), n) : n;
    }
    // one pass (or warm-up, or bare-model run) of slot m in the form the pool chose for it; `end`: the pass's end markers, for a launch that can carry them (aidax_pool.cpp)
    hipError_t launch(const ModelSlot& m, const LaunchArgs& a, hipStream_t s, PassEnd* end = nullptr, const PassForm* known = nullptr) const;
    // A fresh DynamicModel for stream s alone (:1035, :1053-1061), with START_WARMUP 2048 zeros through applyModel (:1077-1078): the launch
    // arguments view the pool as one stream, which plays the model of `rec` (m's own, or a bank slot's weights, gains and skip)
    void fresh_stream_model(const ModelSlot& m, uint32_t s, int start_mode, const ModelRec& rec, hipStream_t on) const
    {
        HIP_TRY(launch_reset_for_model(d_st.get() + s, m.d_nn.get() + static_cast<size_t>(s) * m.nn_stride, 1, m.nn_stride, m.p_den(), on));
        const uint32_t chunk = launch_chunk(m, kWarmupFrames);
        for (uint32_t done = 0; start_mode == AIDAX_START_WARMUP && done < kWarmupFrames; done += chunk) {
            LaunchArgs a = args(m, d_st.get(), nullptr, nullptr, std::min(chunk, kWarmupFrames - done), MODE_WARMUP);
            apply_model_rec(a, rec);
            a.ctl += s; a.st += s; a.nn += static_cast<size_t>(s) * m.nn_stride;
            a.n_streams = 1;
            HIP_TRY(launch(m, a, on));
        }
    }
    // an audio-side call that issues work on the pool's own stream, behind everything issued so far
    template <class F> int on_own_stream(F&& f) { return guarded([&]() -> int { HIP_TRY(hipSetDevice(device)); enter_stream(q); return f(); }); }
    // What is not memory (aidax_pool_destroy has set the device and waited for the streams; a failed aidax_pool_create comes here on its device)
    ~aidax_pool()
    {
        if (cur.lp_owner) lp_gate().release(device, cur.lp_owner);
        if (h_lp_fault)                                      // (measurement builds / AIDAX_TUNE bit 4096: the stamps behind the fault word, while it is alive)
            if (const char* f = AIDAX_HOOK_ENV("AIDAX_LP_TRACE_FILE"))
                if (FILE* fp = std::fopen(f, "wb")) { std::fwrite(h_lp_fault.get() + 16, 4, 1536, fp); std::fclose(fp); }
        for (const HostRange& r : host_ranges) (void)hipHostUnregister(r.base);
    }
};

namespace aidax {
// worker side (aidax_pool_model.cpp): a staged object goes back, behind its fence; an empty staged object of pool p, with the fence its commit will record
void staged_release(aidax_staged* s);
using StagedPtr = std::unique_ptr<aidax_staged, void (*)(aidax_staged*)>;
StagedPtr new_staged(const aidax_pool& p, aidax_staged::Payload payload);
}  // namespace aidax
