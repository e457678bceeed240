// aidax_pool.cpp — one of the stream pool's four sources behind the C ABI (aidax_pool.h): which models have a device path, launch (the
// executor of a PassForm), the pass itself with its stages in their order (pool_process_prefix), create / destroy, control latching and
// the streams' state. The opt-in stages' own calls: aidax_pool_stages.cpp; models and IRs on their way in: aidax_pool_model.cpp; host
// buffers: aidax_pool_io.cpp. Host logic only; the kernels are in the .hip sources. No CPU fallback: any HIP failure is AIDAX_ERR_DEVICE.
#include <hip/hip_runtime_api.h>

#include <chrono>
#include <cstdio>
#include <cmath>
#include <thread>

#include "aidax_pool.h"

namespace aidax {

// Which models have a device path: the reference's 54 variants (18 register-resident kernels; k_quad /
// k_mfma for many streams), stacked or wider recurrent layers (k_mfma, k_stack) and conv1d stacks
// (k_conv_mfma, k_conv) as extensions.
bool model_supported(const aidax_model& m)
{
    if (is_conv_model(m)) {
        if (m.input_size != 1 || m.hidden > 16 || m.n_rnn > kMaxConvLayers) return false;
        for (int l = 0; l < m.n_rnn; ++l)
            if (m.layers[l].out_size != m.hidden || m.layers[l].ksize > 8) return false;
        return true;
    }
    if (is_stack_model(m)) return m.n_rnn <= kMaxStackLayers && m.hidden <= 128 && m.hidden % 4 == 0;
    return m.n_rnn == 1 && find_kernel(m.cell, m.hidden) != nullptr;
}

LpGate& lp_gate() { static LpGate g; return g; }

// AIDAX_KEEP_WARM_US=<period in us> (off unless set): a host calls run() once per audio period (rt-neural-generic.cpp:484) — 1.3 to 5.3 ms
// apart — and a GPU that has idled for that long serves the next launch slower than one that is kept busy (bench.py realtime_paced: the
// same pass 8 - 13 % longer, the call's tail several times longer). With the variable set, ONE thread per device launches an empty grid
// (a wave per CU) on a stream of the lowest priority every <period>, while any pool on that device exists. Never on the audio thread;
// what it buys on a box is measured by bench.py (realtime_paced.keep_warm) and stated in INTEGRATION.md §3.
struct KeepWarm {
    std::mutex mu;
    struct Dev { int refs = 0; std::thread th; std::atomic<bool> stop{false}; } dev[64];
    ~KeepWarm()
    {
        for (Dev& d : dev) { d.stop.store(true); if (d.th.joinable()) d.th.detach(); }      // (a pool that outlived main(): no join at exit)
    }
    static long period_us()
    {
        const char* e = std::getenv("AIDAX_KEEP_WARM_US");
        const long v = e ? std::strtol(e, nullptr, 10) : 0;
        return v >= 50 && v <= 1000000 ? v : 0;
    }
    bool acquire(int device)
    {
        const long us = period_us();
        if (us == 0 || device < 0 || device >= 64) return false;
        std::lock_guard<std::mutex> g(mu);
        Dev& d = dev[device];
        if (d.refs++ == 0) {
            d.stop.store(false);
            d.th = std::thread([device, us, &d] {
                if (hipSetDevice(device) != hipSuccess) return;
                int least = 0, greatest = 0, cus = 0;
                hipStream_t q = nullptr;
                (void)hipDeviceGetStreamPriorityRange(&least, &greatest);
                if (hipStreamCreateWithPriority(&q, hipStreamNonBlocking, least) != hipSuccess) return;
                (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device);
                auto next = std::chrono::steady_clock::now();
                while (!d.stop.load(std::memory_order_relaxed)) {
                    (void)launch_keep_warm_kernel(cus > 0 ? cus : 1, q);
                    next += std::chrono::microseconds(us);
                    const auto now = std::chrono::steady_clock::now();
                    if (next < now) next = now;
                    std::this_thread::sleep_until(next);
                }
                (void)hipStreamSynchronize(q);
                (void)hipStreamDestroy(q);
            });
        }
        return true;
    }
    void release(int device)
    {
        std::thread done;
        {
            std::lock_guard<std::mutex> g(mu);
            Dev& d = dev[device];
            if (d.refs > 0 && --d.refs == 0) { d.stop.store(true); done = std::move(d.th); }
        }
        if (done.joinable()) done.join();
    }
};
static KeepWarm& keep_warm() { static KeepWarm k; return k; }

}  // namespace aidax

// The executor of a PassForm (aidax_pass_form.h decides it): one arm per kernel family; the packed chains around a kernel that does not run
// them itself, the time slices and stream ranges, the end markers and the refusal of a chained grid are what only the launch path can do.
hipError_t aidax_pool::launch(const ModelSlot& m, const LaunchArgs& a, hipStream_t s, PassEnd* end, const PassForm* known) const
{
    // A one-launch pass takes its end markers with it (PassForm::carries_event / carries_word)
    auto take_end_markers = [&](const PassForm& f, LaunchArgs& b) -> hipEvent_t {
        if (!end || !f.carries_event) return nullptr;
        hipEvent_t done = end->done;
        end->done = nullptr;
        end->done_taken = done != nullptr;
        if (end->word && f.carries_word) {
            b.done_word = end->word; b.done_seq = end->seq;
            end->word = nullptr;
            end->word_taken = true;
        }
        return done;
    };
    // a block longer than the extension kernels' 256 frames: time slices, each the whole run() of its slice (the rows keep the block's pitch)
    auto time_slices = [&](auto&& one) {
        const uint32_t chunk = ext_chunk();
        hipError_t e = hipSuccess;
        for (uint32_t done = 0; done < a.n_frames && e == hipSuccess; done += chunk) {
            LaunchArgs b = a;
            b.in = a.in + done; b.out = a.out + done;
            b.n_frames = std::min(chunk, a.n_frames - done);
            b.row_stride = a.n_frames;
            e = one(b);
        }
        return e;
    };
    // a pass over more streams than one resident grid of k_mfma_ls holds: one launch per range (every range a resident grid)
    auto stream_ranges = [&](auto&& one) {
        const uint32_t step = m.form.round_streams();
        hipError_t e = hipSuccess;      // (a refusal can only come from the first range: the ranges are one size or smaller)
        for (uint32_t s0 = 0; s0 < a.n_streams && e == hipSuccess; s0 += step) {
            LaunchArgs b = a;
            b.n_streams = std::min(step, a.n_streams - s0);
            b.ctl = a.ctl + s0; b.st = a.st + s0; b.nn = a.nn + static_cast<size_t>(s0) * a.nn_stride;
            if (a.in) b.in = a.in + static_cast<size_t>(s0) * a.n_frames;
            b.out = a.out + static_cast<size_t>(s0) * a.n_frames;
            e = one(b);
        }
        return e;
    };
    auto in_pieces = [&](const PassForm& f, auto&& one) {
        return f.pieces == PassForm::TIME_SLICES ? time_slices(one) : f.pieces == PassForm::STREAM_RANGES ? stream_ranges(one) : one(a);
    };
    auto kernel = [&](const PassForm& f) -> hipError_t {
        const bool whole_run = a.mode == MODE_CHAIN && !f.chains;      // the kernel runs the DSP chain too
        const KernelEntry* table = m.has_model ? m.kernel : nullptr;
        switch (f.kern) {
        case PassKern::NoModel:
        case PassKern::Wave: return launch_stream_kernel(table, a, lds_bytes(m, a.mode == MODE_CHAIN ? a.n_frames : 0), s);
        case PassKern::Pipe: { LaunchArgs b = a; hipEvent_t done = take_end_markers(f, b); return launch_pipe_kernel(table, b, s, done); }
        case PassKern::Pipe4: { LaunchArgs b = a; hipEvent_t done = take_end_markers(f, b); return launch_pipe4_kernel(table, b, s, done); }
        // (the model bank in force — pool_process_prefix set the records)
        case PassKern::PipeBank: { LaunchArgs b = a; hipEvent_t done = take_end_markers(f, b); return launch_pipe_bank_kernel(table, b, s, done); }
        case PassKern::Q4: { LaunchArgs b = a; b.wpack = m.d_wq4.get(); return launch_q4_kernel(m.hidden, b, s); }
        case PassKern::Nn: return launch_nn_kernel(table, a, s);
        case PassKern::Quad: return launch_quad_kernel(m.cell, m.hidden, a, m.qdesc, s);
        case PassKern::Mfma: return launch_mfma_kernel(a, m.mdesc, s);
        case PassKern::MfmaLp: return launch_mfma_lp_kernel(a, m.mdesc, m.d_ring.get(), m.d_counters.get(), hd_lp_fault, s, whole_run);
        case PassKern::MfmaLs:
            return in_pieces(f, [&](const LaunchArgs& r) { return launch_mfma_ls_kernel(r, m.mdesc, m.d_ring.get(), m.d_counters.get(), hd_lp_fault, m.form.products(), s, whole_run); });
        case PassKern::GruGm: return launch_gru_gm_kernel(a, m.mdesc, s);
        case PassKern::GruGs: return launch_gru_gs_kernel(a, m.mdesc, m.form.products(), s);
        case PassKern::LstmGs: return launch_lstm_gs_kernel(a, m.mdesc, m.form.products(), s);
        case PassKern::Stack: return launch_stack_kernel(a, m.sdesc, s);
        case PassKern::Conv: return launch_conv_kernel(a, m.cdesc, s);
        case PassKern::ConvMfma: return in_pieces(f, [&](const LaunchArgs& r) { return launch_conv_mfma_kernel(r, m.cdesc, whole_run, s); });
        case PassKern::ConvMs: return in_pieces(f, [&](const LaunchArgs& r) { return launch_conv_ms_kernel(r, m.cdesc, whole_run, s); });
        }
        return hipErrorInvalidValue;
    };
    // the packed chains in -> out ahead of a kernel that works in place between them (once per pass), and the kernel — none for a block of no frames
    bool pre_issued = false;
    auto issue = [&](const PassForm& f) {
        hipError_t e = hipSuccess;
        if (f.chains && !pre_issued) { e = launch_chain_pass(true, a, s); pre_issued = true; }
        if (e == hipSuccess && !(f.chains && a.n_frames == 0)) e = kernel(f);
        return e;
    };
    // (a form resolved by the caller stands unless it names a chained kernel that a give-up or a refusal has retired since)
    const bool chained_known = known && (known->kern == PassKern::MfmaLp || known->kern == PassKern::MfmaLs);
    PassForm f = known && !(chained_known && !lp_in_use(m)) ? *known : pass_form(m, a.mode, a.n_frames, a.n_streams, a.bank != nullptr);
    hipError_t e = issue(f);
    if (e == hipErrorCooperativeLaunchTooLarge && (f.kern == PassKern::MfmaLp || f.kern == PassKern::MfmaLs)) {
        // A chained grid the runtime refuses (cooperative launch: it cannot be co-resident on this device — a partitioned GPU, a pool forced
        // onto the kernel) is no error of the pass: the model is served by k_mfma from here on, and the form is resolved again
        (void)hipGetLastError();
        m.lp_refused = true;                          // this model's grid; a pool-wide lp_off is for give-ups (co-tenants)
        // ... and this slot's share of the pool's hold on the device's gate goes back: a pool that cannot use the chained kernels
        // must not keep every other pool of the device off them (advisor, round 5)
        if (m.lp_owner) { lp_gate().release(device, m.lp_owner); m.lp_owner = nullptr; }
        lp_refusals.fetch_add(1, std::memory_order_relaxed);
        set_error("a chained grid cannot be co-resident on this device (cooperative launch refused): the model is served by k_mfma");
        f = pass_form(m, a.mode, a.n_frames, a.n_streams, a.bank != nullptr);
        e = issue(f);
    }
    if (e == hipSuccess && f.chains) e = launch_chain_pass(false, a, s);
    return e;
}

namespace aidax {

// aidax_pool_process_device over the first `n_active` streams only (rows of the others are neither read nor
// written, their state does not move): the hub launches what can be attached, not the pool's capacity.
int pool_process_prefix(aidax_pool* p, const float* d_in, float* d_out, uint32_t n_frames, void* hip_stream, uint32_t n_active, PassEnd* end, const PassForm* form)
{
    if (n_frames > p->max_frames) return fail(AIDAX_ERR_ARG, "n_frames exceeds the pool's max_frames");
    if (n_frames != 0 && (!d_in || !d_out)) return fail(AIDAX_ERR_ARG, "null buffer");
    if (n_active > p->n_streams) return fail(AIDAX_ERR_ARG, "n_active exceeds the pool's streams");
    if (n_active == 0) return AIDAX_OK;
    return guarded([&]() -> int {
        HIP_TRY(hipSetDevice(p->device));
        hipStream_t s = hip_stream ? static_cast<hipStream_t>(hip_stream) : p->q;
        p->enter_stream(s);
        p->flush_ctl(s);
        p->note_lp_give_up();                                          // (ahead of the form's resolution in launch)
        LaunchArgs a = p->args(p->cur, p->d_st.get(), d_in, d_out, n_frames, MODE_CHAIN);
        a.n_streams = n_active;
        if (p->bank.in_force()) a.bank = p->bank.flush(s);           // the records this pass plays, ahead of it on its stream
        // with an IR history the pass ends behind the IR stage: its end markers (the submit path's event, the blocking path's completion
        // word) are not handed down to the model's launch but issued after the stage by the caller
        const bool ir_on = n_frames != 0 && p->ir.adopt();
        // ... and a metered pass behind k_meter's reading of the block it returns: the same rule, so that a pass that has ended for the host
        // (aidax_pool_process has returned, the submit path's download may start) has also been metered
        const bool meter_on = n_frames != 0 && p->meter.on;
        // ... and a pass with the mix buses on behind k_mix: a pass that has ended for the host has been mixed
        const bool mix_on = n_frames != 0 && p->mix.on;
        // ... and a pass with a stream delay on behind k_delay, which works in place on the block the pass returns
        const bool delay_on = n_frames != 0 && p->delay.plays();
        if (ir_on || meter_on || mix_on || delay_on) end = nullptr;    // (the markers are not handed down: nullptr to launch)
        if (ir_on) p->ir.begin_pass(s, p->any_pass);                   // the plan this pass is issued with, ahead of it
        if (meter_on) p->meter.launch_in(d_in, n_active, n_frames, s);  // (ahead of the pass: it may work in place)
        p->tuner.before_pass(d_in, n_active, n_frames, s);            // the tuners read the same block: the DI signal, ahead of the gate
        a.in = p->gate.before_pass(d_in, p->d_ctl.get(), n_active, n_frames, s);      // the gated block, where a gate is on
        HIP_TRY(p->launch(p->cur, a, s, end, form));
        if (ir_on) p->ir.issue(s, d_out, n_active, n_frames);
        else p->ir.plan.advance(n_active, n_frames);                   // (no history yet: both sides of a blend are the dry block, its ramps run on)
        if (delay_on) p->delay.after_pass(d_out, p->d_ctl.get(), n_active, n_frames, s);      // the stream delays, in place: the meters and the buses see the delayed block
        if (meter_on) p->meter.launch_out(d_out, n_active, n_frames, s);
        const bool limit_on = mix_on && p->limit.on;                   // the bus limiters: k_mix writes their raw side block, k_bus_limit the bus block
        if (mix_on) p->mix.after_pass(d_out, n_active, n_frames, s, limit_on ? p->limit.d_raw.get() : nullptr);      // the buses: a gather over the block the pass returns
        if (mix_on && p->reverb.on) p->reverb.after_mix(limit_on ? p->limit.d_raw.get() : p->mix.d_bus.get(), n_frames, s);      // the bus reverbs, in place on the block k_mix wrote
        if (limit_on) p->limit.after_mix(p->mix.d_bus.get(), n_frames, s);
        if (n_frames != 0) p->any_pass = true;
        return AIDAX_OK;
    });
}

// Park / unpark one stream for the coming passes: while parked it behaves like a disabled plugin (raw copy, no state
// moves) whatever its own `enabled` control says. One flag flip in the host record — no filter redesign: the hub
// does this for every stream that is not part of the pass it launches.
int pool_park_stream(aidax_pool* p, uint32_t s, bool parked)
{
    if (s >= p->n_streams) return fail(AIDAX_ERR_ARG, "stream out of range");
    if ((p->forced_off[s] != 0) == parked) return AIDAX_OK;
    p->forced_off[s] = parked ? 1 : 0;
    StreamCtl& o = p->h_ctl[s];
    if (!parked && p->controls[s].enabled > 0.5f) o.flags |= CTL_ENABLED;
    else o.flags &= ~static_cast<uint32_t>(CTL_ENABLED);
    p->ctl_dirty.mark(s, s);
    return AIDAX_OK;
}

// Did a k_mfma_lp pass since the last call give up a hand-over (its output is wrong)? Clears the report and retires the
// kernel for this pool. The hub asks after a pass's event has passed.
bool pool_take_lp_fault(aidax_pool* p) { return p->take_lp_fault(); }
bool pool_chained_kernel_in_use(aidax_pool* p) { return p->cur.has_model && p->cur.kind == ModelSlot::MFMA && p->cur.mdesc.n_layers >= 2 && p->lp_in_use(p->cur); }
bool pool_lp_in_use(const aidax_pool* p) { return p->cur.has_model && p->lp_in_use(p->cur); }

int pool_device(const aidax_pool* p) { return p->device; }
uint32_t pool_max_frames(const aidax_pool* p) { return p->max_frames; }
int pool_enter_own_stream(aidax_pool* p) { return p->on_own_stream([] { return AIDAX_OK; }); }

}  // namespace aidax

extern "C" {

AIDAX_API int aidax_device_count(int* count)
{
    if (!count) return fail(AIDAX_ERR_ARG, "null count");
    *count = 0;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return fail(AIDAX_ERR_DEVICE, "no usable HIP device (this library has no CPU fallback)");
    *count = n;
    return AIDAX_OK;
}

AIDAX_API int aidax_pool_create(uint32_t n_streams, uint32_t max_frames, double host_samplerate,
                                int device_id, aidax_pool** out)
{
    if (!out) return fail(AIDAX_ERR_ARG, "null argument");
    *out = nullptr;
    if (n_streams == 0 || max_frames == 0 || max_frames > kMaxFrames || !(host_samplerate > 0))
        return fail(AIDAX_ERR_ARG, "n_streams/max_frames/samplerate out of range");
    return guarded([&]() -> int {
        int n_dev = 0;
        if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev <= 0)
            return fail(AIDAX_ERR_DEVICE, "no HIP device: the MI355X path has no CPU fallback");
        if (device_id < 0 || device_id >= n_dev) return fail(AIDAX_ERR_ARG, "device_id out of range");
        auto p = std::make_unique<aidax_pool>();
        p->device = device_id;
        p->n_streams = n_streams;
        p->max_frames = max_frames;
        p->packed_fits = chain_lds_bytes(max_frames) <= kChainLdsLimit;
        p->host_sr = host_samplerate;
        p->gain_coef = exp_smoother_coef(static_cast<float>(host_samplerate), 0.1f);
        p->force = parse_force(AIDAX_HOOK_ENV("AIDAX_KERNEL"));
        if (const char* t = AIDAX_HOOK_ENV("AIDAX_TUNE")) p->tune = std::atoi(t);
        // (a failure from here on: ~aidax_pool and the owning members give back what was made, the streams last)
        HIP_TRY(hipSetDevice(device_id));
        HIP_TRY(hipDeviceGetAttribute(&p->cus, hipDeviceAttributeMultiprocessorCount, device_id));
        // the audio side's stream outranks the worker's: a pass must not queue behind a warm-up for its CUs
        int prio_least = 0, prio_greatest = 0;
        HIP_TRY(hipDeviceGetStreamPriorityRange(&prio_least, &prio_greatest));
        p->q.create(prio_greatest);
        p->wq.create(prio_least);
        { const char* sp = std::getenv("AIDAX_SPIN_WAIT"); p->spin_collect = !(sp && sp[0] == '0'); }
        p->keep_warm = keep_warm().acquire(device_id);
        p->h_lp_fault.alloc(2048);                              // (8192 bytes) the fault word + the time stamps of scratch/lp_trace.py, r05_modes.py
        p->hd_lp_fault = p->h_lp_fault.device();
        *p->h_lp_fault.get() = 0;
        p->ev_x.create();
        p->ev_adopt.create();
        p->d_ctl.alloc(n_streams);
        p->d_st.alloc(n_streams);
        p->io.alloc(n_streams * static_cast<size_t>(max_frames), device_id);
        p->ctl_ring.alloc(sizeof(StreamCtl) * n_streams);
        p->ir.init(n_streams, max_frames, p->cus, p->wq);
        p->controls.resize(n_streams);
        for (auto& c : p->controls) aidax_controls_default(&c);
        p->loading.assign(n_streams, 1);
        p->forced_off.assign(n_streams, 0);
        p->h_ctl.resize(n_streams);
        p->refresh_all();
        // instantiate(), rt-neural-generic.cpp:283-321: preGain target 1 cleared, masterGain target 0 cleared,
        // biquad z = 0, no model, loading = true
        HIP_TRY(launch_init_streams(p->d_st.get(), n_streams, p->q));
        HIP_TRY(hipStreamSynchronize(p->q));
        p->last_stream = p->q;
        *out = p.release();
        return AIDAX_OK;
    });
}

AIDAX_API void aidax_pool_destroy(aidax_pool* p)
{
    if (!p) return;
    (void)hipSetDevice(p->device);
    if (p->last_stream && p->last_stream != p->q) (void)hipStreamSynchronize(p->last_stream);
    if (p->q) (void)hipStreamSynchronize(p->q);
    if (p->wq) (void)hipStreamSynchronize(p->wq);
    if (p->pipe.q_up) (void)hipStreamSynchronize(p->pipe.q_up);
    if (p->pipe.q_down) (void)hipStreamSynchronize(p->pipe.q_down);
    const bool warm = p->keep_warm;
    const int device = p->device;
    delete p;
    if (warm) keep_warm().release(device);
}

AIDAX_API uint32_t aidax_pool_streams(const aidax_pool* p) { return p ? p->n_streams : 0; }
AIDAX_API double aidax_pool_samplerate(const aidax_pool* p) { return p ? p->host_sr : 0.0; }

AIDAX_API int aidax_pool_reset_stream(aidax_pool* p, uint32_t stream, int start_mode) { return aidax::pool_reset_stream_inherit(p, stream, start_mode, nullptr); }

#ifdef AIDAX_TEST_HOOKS
AIDAX_API int aidax_test_hip_calls(char* buf, uint32_t cap) { return read_hip_calls(buf, cap); }      // (test build only, not in include/aidax.h)
// (test build only: aidax_pool_process_device over the first n_active streams — the hub's prefix pass, which no public call reaches on a pool
// with buses: tests/test_gpu_bus_limit.py)
AIDAX_API int aidax_test_process_prefix(aidax_pool* p, const float* d_in, float* d_out, uint32_t n_frames, void* hip_stream, uint32_t n_active)
{
    if (!p) return fail(AIDAX_ERR_ARG, "null pool");
    return aidax::pool_process_prefix(p, d_in, d_out, n_frames, hip_stream, n_active);
}
// (test build only: one stream's whole record as the kernels left it — `pending`, and in `pad` the length of the post cascade that the last
// k_*_pipe4 launch ran for the stream, 1 where it skipped a transparent EQ: tests/test_gpu_eq_transparent.py)
AIDAX_API int aidax_test_stream_state(aidax_pool* p, uint32_t stream, void* out, uint32_t cap)
{
    if (!out || cap < sizeof(StreamState)) return fail(AIDAX_ERR_ARG, "buffer too small for a stream's record");
    StreamState st{};
    const int rc = aidax::pool_read_stream_state(p, stream, &st);
    if (rc != AIDAX_OK) return rc;
    std::memcpy(out, &st, sizeof(StreamState));
    return (int)sizeof(StreamState);
}
// (test build only: what choose_form decided for the playing slot, as one text line — tests/test_gpu_load_forms.py)
AIDAX_API int aidax_test_slot_form(aidax_pool* p, char* buf, uint32_t cap)
{
    if (!p || !buf || cap == 0) return fail(AIDAX_ERR_ARG, "null argument");
    static const char* const kinds[] = { "table", "stack", "conv", "mfma", "quad" };
    const ModelSlot& m = p->cur;
    const SlotForm& f = m.form;
    return std::snprintf(buf, cap, "kind=%s serve=%d fused=%d products=%d round_streams=%u pipe_capacity=%d split_pays=%d q4=%d nn_stride=%u ring=%d",
                         m.has_model ? kinds[m.kind] : "none", static_cast<int>(f.serve()), f.fused(), f.products(), f.round_streams(), f.pipe_capacity(), f.split_pays(), f.q4(),
                         m.nn_stride, m.d_ring ? 1 : 0);
}
#endif

}  // extern "C"

namespace aidax {

// aidax_pool_reset_stream for a stream that continues another plugin instance's life: the fresh DynamicModel is built
// around `p_targets` (the PARAM targets of the model that instance plays now, :822-825) instead of the 0 / 0 of a first load.
int pool_reset_stream_inherit(aidax_pool* p, uint32_t stream, int start_mode, const float* p_targets)
{
    if (!p) return fail(AIDAX_ERR_ARG, "null pool");
    if (stream >= p->n_streams) return fail(AIDAX_ERR_ARG, "stream out of range");
    if (start_mode != AIDAX_START_WARMUP && start_mode != AIDAX_START_RESET) return fail(AIDAX_ERR_ARG, "bad start_mode");
    return p->on_own_stream([&]() -> int {
        const ModelSlot& m = p->cur;
        HIP_TRY(launch_init_streams(p->d_st.get() + stream, 1, p->q));      // instantiate(), :283-321
        p->ir.clear_stream(stream, p->q);                              // a fresh instance has no past for the IR to sound
        p->gate.clear_states(stream, 1, p->q);                         // ... and its gate starts at unity gain, hold expired
        if (p->tuner.enabled()) { p->tuner.book.restart(stream); p->tuner.clear_streams(stream, 1, p->q); }      // ... and its tuner has heard nothing
        p->delay.clear_states(stream, 1, p->q);                        // ... and its delay line is empty
        if (p_targets) HIP_TRY(launch_set_param_targets(p->d_st.get() + stream, p_targets[0], p_targets[1], p->q));
        const ModelBank* b = p->bank.adopt();                         // (a stream on a bank slot keeps it: that slot's weights, gains and skip)
        if (m.has_model) p->fresh_stream_model(m, stream, start_mode, b && b->assign[stream] >= 0 ? ModelBank::rec_of(b->slot[b->assign[stream]]) : m.rec(), p->q);
        p->loading[stream] = m.has_model ? 0 : 1;
        p->refresh_ctl(stream);
        return AIDAX_OK;
    });
}

// Stream `ds` of `dst` takes over the plugin-owned DSP members (biquad states, gain smoothers) of stream `ss` of `src`,
// as they are once everything `src` has issued so far has run: an event on src's latest stream, a wait on dst's own,
// one tiny kernel. Nothing waits on the host: this is work_response() of an instance that moves between hubs. The
// caller serialises access to both pools (the hubs' locks).
int pool_adopt_stream_dsp(aidax_pool* dst, uint32_t ds, aidax_pool* src, uint32_t ss)
{
    if (!dst || !src || ds >= dst->n_streams || ss >= src->n_streams) return fail(AIDAX_ERR_ARG, "adopt: stream out of range");
    if (dst->device != src->device) return fail(AIDAX_ERR_ARG, "adopt: pools on different devices");
    return guarded([&]() -> int {
        HIP_TRY(hipSetDevice(dst->device));
        hipStream_t from = src->last_stream ? src->last_stream : src->q;
        HIP_TRY(hipEventRecord(src->ev_adopt.get(), from));
        dst->enter_stream(dst->q);
        HIP_TRY(hipStreamWaitEvent(dst->q, src->ev_adopt.get(), 0));
        HIP_TRY(launch_adopt_dsp(dst->d_st.get() + ds, src->d_st.get() + ss, dst->q));
        if (src != dst) {                                   // src must not overwrite the record before the copy has read it:
            HIP_TRY(hipEventRecord(dst->ev_adopt.get(), dst->q));  // its next operation waits for the copy (the stream is parked or
            src->enter_stream(src->q);                       // detached by then, but a later occupant of the seat is reset on src->q)
            HIP_TRY(hipStreamWaitEvent(src->q, dst->ev_adopt.get(), 0));
        }
        return AIDAX_OK;
    });
}

// One stream's record as it is once the pool's issued work has run (waits: worker / test side only).
int pool_read_stream_state(aidax_pool* p, uint32_t stream, StreamState* out)
{
    if (!p || !out || stream >= p->n_streams) return fail(AIDAX_ERR_ARG, "stream out of range");
    return guarded([&]() -> int {
        HIP_TRY(hipSetDevice(p->device));
        p->sync_issued();
        HIP_TRY(hipStreamSynchronize(p->q));
        HIP_TRY(hipMemcpy(out, p->d_st.get() + stream, sizeof(StreamState), hipMemcpyDeviceToHost));
        return AIDAX_OK;
    });
}

bool pool_has_model(const aidax_pool* p) { return p->cur.has_model; }

// The same read without a wait inside: the copy (into pinned memory of the caller) and `done` are put behind what the
// pool has issued so far; the caller waits for `done` wherever it may.
int pool_peek_stream_state(aidax_pool* p, uint32_t stream, StreamState* pinned_out, void* done_event)
{
    if (!p || !pinned_out || stream >= p->n_streams) return fail(AIDAX_ERR_ARG, "stream out of range");
    return p->on_own_stream([&]() -> int {
        HIP_TRY(hipMemcpyAsync(pinned_out, p->d_st.get() + stream, sizeof(StreamState), hipMemcpyDeviceToHost, p->q));
        HIP_TRY(hipEventRecord(static_cast<hipEvent_t>(done_event), p->q));
        return AIDAX_OK;
    });
}

}  // namespace aidax

extern "C" {

AIDAX_API int aidax_pool_export_stream_dsp(aidax_pool* p, uint32_t stream, aidax_stream_dsp* out)
{
    if (!p || !out) return fail(AIDAX_ERR_ARG, "null argument");
    StreamState st{};
    const int rc = aidax::pool_read_stream_state(p, stream, &st);
    if (rc != AIDAX_OK) return rc;
    std::memcpy(out->z, st.z, sizeof(out->z));
    out->pre_mem = st.pre_mem; out->master_mem = st.master_mem;
    out->pre_target = st.pre_tgt; out->master_target = st.master_tgt;
    out->param_target[0] = p->cur.has_model ? st.p_tgt[0] : 0.f;           // no model: work() passes 0 / 0 (:815-816)
    out->param_target[1] = p->cur.has_model ? st.p_tgt[1] : 0.f;
    return AIDAX_OK;
}

AIDAX_API int aidax_pool_import_stream_dsp(aidax_pool* p, uint32_t stream, const aidax_stream_dsp* in)
{
    if (!p || !in) return fail(AIDAX_ERR_ARG, "null argument");
    if (stream >= p->n_streams) return fail(AIDAX_ERR_ARG, "stream out of range");
    return guarded([&]() -> int {
        HIP_TRY(hipSetDevice(p->device));
        StreamState st{};
        const int rc = aidax::pool_read_stream_state(p, stream, &st);     // waits for the pool's passes: not an audio-thread call
        if (rc != AIDAX_OK) return rc;
        std::memcpy(st.z, in->z, sizeof(st.z));
        st.pre_mem = in->pre_mem; st.master_mem = in->master_mem;
        st.pre_tgt = in->pre_target; st.master_tgt = in->master_target;
        st.pending &= ~static_cast<uint32_t>(PEND_ACTIVATE);
        HIP_TRY(hipMemcpy(p->d_st.get() + stream, &st, sizeof(StreamState), hipMemcpyHostToDevice));
        return AIDAX_OK;
    });
}

AIDAX_API int aidax_pool_set_loading(aidax_pool* p, int32_t stream, int loading)
{
    if (!p) return fail(AIDAX_ERR_ARG, "null pool");
    uint32_t lo = 0, hi = 0;
    if (!named_range(stream, p->n_streams, &lo, &hi)) return fail(AIDAX_ERR_ARG, "stream out of range");
    for (uint32_t s = lo; s < hi; ++s) {
        p->loading[s] = loading ? 1 : 0;
        p->patch_model_fields(s);
    }
    p->ctl_dirty.mark(lo, hi - 1);
    return AIDAX_OK;
}

AIDAX_API int aidax_pool_set_controls(aidax_pool* p, int32_t stream, const aidax_controls* c)
{
    if (!p || !c) return fail(AIDAX_ERR_ARG, "null argument");
    uint32_t lo = 0, hi = 0;
    if (!named_range(stream, p->n_streams, &lo, &hi)) return fail(AIDAX_ERR_ARG, "stream out of range");
    for (uint32_t s = lo; s < hi; ++s) p->controls[s] = *c;
    if (stream == AIDAX_ALL_STREAMS) p->refresh_all();
    else p->refresh_ctl(lo);
    return AIDAX_OK;
}

AIDAX_API int aidax_pool_activate(aidax_pool* p, int32_t stream)
{
    if (!p) return fail(AIDAX_ERR_ARG, "null pool");
    uint32_t lo = 0, hi = 0;                                // (k_set_pending takes the index as the call names it)
    if (!named_range(stream, p->n_streams, &lo, &hi)) return fail(AIDAX_ERR_ARG, "stream out of range");
    return p->on_own_stream([&]() -> int {
        // paramFirstRun is only re-armed when a model exists (rt-neural-generic.cpp:344-351)
        const uint32_t bits = PEND_ACTIVATE | (p->cur.has_model ? PEND_PARAM_FIRST : 0u);
        HIP_TRY(launch_set_pending(p->d_st.get(), p->n_streams, stream, bits, p->q));
        return AIDAX_OK;
    });
}

AIDAX_API int aidax_pool_process_device(aidax_pool* p, const float* d_in, float* d_out, uint32_t n_frames, void* hip_stream)
{
    if (!p) return fail(AIDAX_ERR_ARG, "null pool");
    return pool_process_prefix(p, d_in, d_out, n_frames, hip_stream, p->n_streams);
}

AIDAX_API int aidax_pool_read_state(aidax_pool* p, uint32_t stream, int layer, float* h, float* c, uint32_t cap)
{
    if (!p || !h) return fail(AIDAX_ERR_ARG, "null argument");
    const ModelSlot& m = p->cur;
    if (!m.has_model || stream >= p->n_streams || m.kind == ModelSlot::CONV) return fail(AIDAX_ERR_STATE, "no such state");
    // TABLE and QUAD pools keep one layer as h[H] | c[H] (pack_quad shares the table kernels' state layout)
    const int n_layers = m.kind == ModelSlot::MFMA ? m.mdesc.n_layers : m.kind == ModelSlot::STACK ? m.sdesc.n_layers : 1;
    if (layer < 0 || layer >= n_layers) return fail(AIDAX_ERR_STATE, "no such layer");
    return guarded([&]() -> int {
        HIP_TRY(hipSetDevice(p->device));
        p->sync_issued();
        HIP_TRY(hipStreamSynchronize(p->q));
        uint32_t H = static_cast<uint32_t>(m.hidden), off = 0;
        bool lstm = false;
        if (m.kind == ModelSlot::STACK) {
            H = static_cast<uint32_t>(m.sdesc.L[layer].hidden); off = m.sdesc.L[layer].state_off; lstm = m.sdesc.L[layer].cell == 0;
        } else if (m.kind == ModelSlot::MFMA) {
            H = static_cast<uint32_t>(m.mdesc.hidden_true); off = m.mdesc.L[layer].state_off; lstm = m.mdesc.L[layer].cell == 0;
        } else {
            lstm = m.cell == AIDAX_CELL_LSTM;
        }
        const uint32_t n = H < cap ? H : cap;
        const float* base = m.d_nn.get() + static_cast<size_t>(stream) * m.nn_stride + off;
        HIP_TRY(hipMemcpy(h, base, n * sizeof(float), hipMemcpyDeviceToHost));
        if (c && lstm) HIP_TRY(hipMemcpy(c, base + H, n * sizeof(float), hipMemcpyDeviceToHost));
        return static_cast<int>(H);
    });
}

}  // extern "C"
