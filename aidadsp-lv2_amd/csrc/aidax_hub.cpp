// aidax_hub.cpp — host-side stream aggregator: many plugin instances of one process, one pool pass per
// audio period (include/aidax.h, "hub"). Pipelined by one period so that hosts that call their instances
// one after another never wait on each other; see the header for the contract.
//
// Who does what:
//   run() of an instance   stages its input row into pinned memory and counts itself in (a few hundred
//                          nanoseconds under the hub's mutex), then — outside the mutex — waits for the event of
//                          the PREVIOUS period's pass (normally long complete) and copies its output row out.
//                          It launches nothing unless it has to close a period itself (re-entry before the
//                          launcher got to it, change of block size).
//   the launcher thread    launches the pass of a period (H2D of the attached rows, the pool pass, D2H, event)
//                          as soon as every attached instance has submitted, or when the period's deadline
//                          passes — so one instance that stalls or stops calling cannot hold the others' audio.
//
// The bookkeeping of all that is HubBook's (aidax_hub_book.h, host only). Every ABI function here checks its arguments, takes the lock,
// asks the book, does the HIP and pool calls the answer requires, and tells the book.
#include <hip/hip_runtime_api.h>

#include <chrono>
#include <condition_variable>
#include <cstring>
#include <memory>
#include <mutex>
#include <thread>

#include "aidax_hub_book.h"
#include "aidax_hip_host.h"

using namespace aidax;
using Clock = std::chrono::steady_clock;

struct aidax_hub {
    // Members go in reverse declaration order, behind ~aidax_hub's join and wait: the pool first (before the stream it last ran on goes
    // away), then every block and event, the stream q last. So q is declared first and the pool behind everything it must not outlive.
    Stream q;
    DevBuf<float> d_in, d_out;
    PinnedBuf<float> h_in[kHubBuffers], h_out[kHubBuffers];      // pinned staging, rows packed at the period's block length
    Event done[kHubBuffers];                     // the pass a buffer holds has delivered its output
    PinnedBuf<StreamState> h_peek;               // one seat's record on its way to a worker thread (attach_successor)
    Event peek_ev;
    std::mutex peek_mu;                          // one reader at a time
    uint32_t max_frames = 0;
    int device = 0;
    double host_sr = 48000.0;
    HubBook book;                                // everything below `mu` that is bookkeeping
    std::mutex mu;
    std::condition_variable cv;
    std::thread launcher;
    bool stop = false;
    int64_t deadline_us = -1;                    // < 0: half the period; 0: no deadline
    Clock::time_point deadline{};
    struct PoolClose { void operator()(aidax_pool* p) const { aidax_pool_destroy(p); } };
    std::unique_ptr<aidax_pool, PoolClose> pool;

    // what is not memory
    ~aidax_hub()
    {
        {
            std::lock_guard<std::mutex> g(mu);
            stop = true;
        }
        cv.notify_all();
        if (launcher.joinable()) launcher.join();
        if (q) (void)hipStreamSynchronize(q);
    }
};

namespace {

// launch the period that is being collected (h.mu held): asynchronous, nothing in here waits for the GPU
int launch_period(aidax_hub& h)
{
    HubBook& b = h.book;
    const uint32_t n = b.period_frames;
    const uint32_t rows = b.hi_slot;
    for (uint32_t s = 0; s < rows; ++s) {
        bool off = false;
        if (!b.park_change(s, &off)) continue;
        const int rc = pool_park_stream(h.pool.get(), s, off);      // (its controls stay what the instance set)
        if (rc != AIDAX_OK) return rc;
        b.parked(s, off);
    }
    const int buf = b.cur;
    const size_t bytes = sizeof(float) * static_cast<size_t>(rows) * n;
    HIP_TRY(hipSetDevice(h.device));
    if (bytes != 0) HIP_TRY(hipMemcpyAsync(h.d_in.get(), h.h_in[buf].get(), bytes, hipMemcpyHostToDevice, h.q));
    const int rc = pool_process_prefix(h.pool.get(), h.d_in.get(), h.d_out.get(), n, h.q, rows);
    if (rc != AIDAX_OK) return rc;
    const bool chained = pool_chained_kernel_in_use(h.pool.get());  // (asked after the launch: a pool that has just fallen back answers no)
    if (bytes != 0) HIP_TRY(hipMemcpyAsync(h.h_out[buf].get(), h.d_out.get(), bytes, hipMemcpyDeviceToHost, h.q));
    HIP_TRY(hipEventRecord(h.done[buf].get(), h.q));
    // normally one event query ("not ready" is an answer, not a failure)
    const int next = b.next_staging();
    b.passed(chained, b.staged_before(next) && hipEventQuery(h.done[next].get()) != hipSuccess);
    return AIDAX_OK;
}

// Close the period that is being collected (h.mu held). A period that cannot be launched is dropped (its instances read silence for it
// and the error is reported by their next run()): the launcher must never find the same failing period waiting for it again. Guarded as a
// whole: the launcher thread calls it, and no exception may leave a thread.
int flush_locked(aidax_hub& h)
{
    if (!h.book.begin_flush()) return AIDAX_OK;
    const int rc = guarded([&]() -> int { return launch_period(h); });
    if (rc != AIDAX_OK) h.book.dropped();
    return rc;
}

// ... ahead of a call that changes what a seat plays under, if the seat has a block waiting for its pass
int close_if_submitted(aidax_hub& h, int32_t slot) { return h.book.must_close(static_cast<uint32_t>(slot)) ? flush_locked(h) : AIDAX_OK; }

void launcher_main(aidax_hub* h)
{
    HubBook& b = h->book;
    std::unique_lock<std::mutex> lk(h->mu);
    while (!h->stop) {
        const bool timed = b.n_submitted != 0 && h->deadline_us != 0;
        if (b.flush_requested || (timed && Clock::now() >= h->deadline)) {
            if (!b.flush_requested) ++b.deadline_launches;
            const int rc = flush_locked(*h);
            if (rc != AIDAX_OK) b.last_error = rc;
            continue;
        }
        if (timed) h->cv.wait_until(lk, h->deadline);
        else h->cv.wait(lk);
    }
}

// counters read under the mutex: the launcher thread writes them
template <class T, class F>
T hub_read(const aidax_hub* h, F&& f)
{
    if (!h) return T{};
    aidax_hub* m = const_cast<aidax_hub*>(h);
    std::lock_guard<std::mutex> g(m->mu);
    return f(m->book);
}

int attach_locked(aidax_hub* h, int32_t* slot, const float* p_targets)
{
    HubBook& b = h->book;
    const int32_t s = b.free_seat();
    if (s < 0) return fail(AIDAX_ERR_STATE, "hub is full");
    // a fresh instance in this slot: a handful of asynchronous launches on the pool's stream, ordered
    // against the passes by the pool's stream edges — nothing here waits for the GPU
    int rc = pool_reset_stream_inherit(h->pool.get(), static_cast<uint32_t>(s), AIDAX_START_WARMUP, p_targets);
    if (rc != AIDAX_OK) return rc;
    rc = aidax_pool_activate(h->pool.get(), s);
    if (rc != AIDAX_OK) return rc;
    aidax_controls_default(&b.ctl[s]);
    rc = aidax_pool_set_controls(h->pool.get(), s, &b.ctl[s]);      // not the previous occupant's
    if (rc != AIDAX_OK) return rc;
    b.attach(static_cast<uint32_t>(s));
    *slot = s;
    return AIDAX_OK;
}

}  // namespace

extern "C" {

AIDAX_API int aidax_hub_create(uint32_t max_instances, uint32_t max_frames, double host_samplerate, int device_id, aidax_hub** out)
{
    if (!out) return fail(AIDAX_ERR_ARG, "null argument");
    *out = nullptr;
    return guarded([&]() -> int {
        aidax_pool* pool = nullptr;
        const int rc = aidax_pool_create(max_instances, max_frames, host_samplerate, device_id, &pool);
        if (rc != AIDAX_OK) return rc;
        auto h = std::make_unique<aidax_hub>();
        h->pool.reset(pool);
        h->max_frames = max_frames;
        h->device = device_id;
        h->host_sr = host_samplerate;
        h->book.init(max_instances);
        for (auto& c : h->book.ctl) aidax_controls_default(&c);
        // (a failure from here on: ~aidax_hub and the owning members give back what was made)
        const size_t count = static_cast<size_t>(max_instances) * max_frames;
        HIP_TRY(hipSetDevice(device_id));
        h->q.create();
        h->d_in.alloc(count);
        h->d_out.alloc(count);
        for (int i = 0; i < kHubBuffers; ++i) {
            h->h_in[i].alloc(count);
            h->h_out[i].alloc(count);
            h->done[i].create();
        }
        h->h_peek.alloc(1);
        h->peek_ev.create();
        // nobody is attached yet: every stream rests disabled
        for (uint32_t s = 0; s < max_instances; ++s) {
            if (pool_park_stream(h->pool.get(), s, true) != AIDAX_OK) return AIDAX_ERR_DEVICE;
            h->book.parked(s, true);
        }
        h->launcher = std::thread(launcher_main, h.get());
        *out = h.release();
        return AIDAX_OK;
    });
}

AIDAX_API void aidax_hub_destroy(aidax_hub* h) { delete h; }

AIDAX_API int aidax_hub_set_deadline_us(aidax_hub* h, int64_t microseconds)
{
    if (!h) return fail(AIDAX_ERR_ARG, "null hub");
    {
        std::lock_guard<std::mutex> g(h->mu);
        h->deadline_us = microseconds;
    }
    h->cv.notify_all();
    return AIDAX_OK;
}

AIDAX_API int aidax_hub_set_model(aidax_hub* h, const aidax_model* m, int start_mode)
{
    if (!h) return fail(AIDAX_ERR_ARG, "null hub");
    // the worker half needs no lock: it builds into buffers of its own on the pool's worker stream
    aidax_staged* sg = nullptr;
    int rc = aidax_pool_prepare_model(h->pool.get(), m, start_mode, &sg);
    if (rc != AIDAX_OK) return rc;
    {
        std::lock_guard<std::mutex> g(h->mu);
        rc = flush_locked(*h);                              // blocks submitted so far were played by the old model
        if (rc == AIDAX_OK) rc = aidax_pool_commit_model(h->pool.get(), sg);
    }
    aidax_staged_free(sg);
    return rc;
}

AIDAX_API int aidax_hub_attach(aidax_hub* h, int32_t* slot)
{
    if (!h || !slot) return fail(AIDAX_ERR_ARG, "null argument");
    std::lock_guard<std::mutex> g(h->mu);
    return attach_locked(h, slot, nullptr);
}

// Worker thread of an instance that plays on (prev, prev_slot) and has loaded another model file: a seat in `h` whose
// fresh DynamicModel is built around the PARAM targets its playing model holds (work(), :822-825, :1053-1061 — they
// are also the conditioning inputs of the 2048-zero warm-up). The predecessor's pending block is launched first, the
// read waits for it outside every lock.
AIDAX_API int aidax_hub_attach_successor(aidax_hub* h, aidax_hub* prev, int32_t prev_slot, int32_t* slot)
{
    if (!h || !slot) return fail(AIDAX_ERR_ARG, "null argument");
    return guarded([&]() -> int {
        float targets[2] = { 0.f, 0.f };                     // no predecessor / no model there: work() passes 0 / 0
        if (prev) {
            std::lock_guard<std::mutex> one(prev->peek_mu);
            bool reading = false;
            {
                std::lock_guard<std::mutex> g(prev->mu);
                if (prev->book.seated(prev_slot) && pool_has_model(prev->pool.get())) {
                    int rc = close_if_submitted(*prev, prev_slot);
                    if (rc != AIDAX_OK) return rc;
                    rc = pool_peek_stream_state(prev->pool.get(), static_cast<uint32_t>(prev_slot), prev->h_peek.get(), prev->peek_ev.get());
                    if (rc != AIDAX_OK) return rc;
                    reading = true;
                }
            }
            if (reading) {
                HIP_TRY(hipEventSynchronize(prev->peek_ev.get()));
                targets[0] = prev->h_peek.get()->p_tgt[0];
                targets[1] = prev->h_peek.get()->p_tgt[1];
            }
        }
        std::lock_guard<std::mutex> g(h->mu);
        return attach_locked(h, slot, targets);
    });
}

// Audio thread, work_response() of that instance (:859-893): from its next block on it plays on (h, slot). The
// plugin's own DSP members — the seven biquads' memories and both gain smoothers (rt-neural-generic.h:311-317), which
// the reference keeps across a model swap (:868-875) — move with it: the predecessor's pending block is launched, and a
// device-side copy ordered behind it fills the new seat's record. No wait, no allocation.
AIDAX_API int aidax_hub_adopt(aidax_hub* h, int32_t slot, aidax_hub* prev, int32_t prev_slot)
{
    if (!h || !prev) return fail(AIDAX_ERR_ARG, "null argument");
    auto body = [&]() -> int {
        if (!h->book.seated(slot)) return fail(AIDAX_ERR_ARG, "slot not attached");
        if (!prev->book.seated(prev_slot)) return fail(AIDAX_ERR_ARG, "predecessor not attached");
        const int rc = close_if_submitted(*prev, prev_slot);    // its last block belongs to the stream the new seat continues
        if (rc != AIDAX_OK) return rc;
        return pool_adopt_stream_dsp(h->pool.get(), static_cast<uint32_t>(slot), prev->pool.get(), static_cast<uint32_t>(prev_slot));
    };
    if (h == prev) {
        std::lock_guard<std::mutex> g(h->mu);
        return body();
    }
    std::scoped_lock g(h->mu, prev->mu);
    return body();
}

AIDAX_API int aidax_hub_detach(aidax_hub* h, int32_t slot)
{
    if (!h) return fail(AIDAX_ERR_ARG, "null hub");
    std::lock_guard<std::mutex> g(h->mu);
    if (!h->book.seated(slot)) return fail(AIDAX_ERR_ARG, "slot not attached");
    return h->book.detach(static_cast<uint32_t>(slot)) ? flush_locked(*h) : AIDAX_OK;
}

AIDAX_API int aidax_hub_set_controls(aidax_hub* h, int32_t slot, const aidax_controls* c)
{
    if (!h || !c) return fail(AIDAX_ERR_ARG, "null argument");
    std::lock_guard<std::mutex> g(h->mu);
    if (!h->book.seated(slot)) return fail(AIDAX_ERR_ARG, "slot not attached");
    if (std::memcmp(&h->book.ctl[slot], c, sizeof(*c)) == 0) return AIDAX_OK;
    // the instance's last block may still wait for its pass (somebody else has not submitted yet): that block was
    // played under the OLD controls, so its period is closed before the new ones go in
    const int rc = close_if_submitted(*h, slot);
    if (rc != AIDAX_OK) return rc;
    h->book.ctl[slot] = *c;
    return aidax_pool_set_controls(h->pool.get(), slot, c);      // the pool keeps the slot parked if it is
}

AIDAX_API int aidax_hub_set_loading(aidax_hub* h, int32_t slot, int loading)
{
    if (!h) return fail(AIDAX_ERR_ARG, "null hub");
    std::lock_guard<std::mutex> g(h->mu);
    if (!h->book.seated(slot)) return fail(AIDAX_ERR_ARG, "slot not attached");
    const int rc = close_if_submitted(*h, slot);                 // as for the controls: what was submitted plays under what was in force
    if (rc != AIDAX_OK) return rc;
    return aidax_pool_set_loading(h->pool.get(), slot, loading);
}

AIDAX_API int aidax_hub_activate(aidax_hub* h, int32_t slot)
{
    if (!h) return fail(AIDAX_ERR_ARG, "null hub");
    std::lock_guard<std::mutex> g(h->mu);
    if (!h->book.seated(slot)) return fail(AIDAX_ERR_ARG, "slot not attached");
    const int rc = close_if_submitted(*h, slot);
    if (rc != AIDAX_OK) return rc;
    return aidax_pool_activate(h->pool.get(), slot);
}

// (allocates nothing and launches nothing unless it closes a period itself; an error text is built only when an error is returned)
AIDAX_API int aidax_hub_run(aidax_hub* h, int32_t slot, const float* in, float* out, uint32_t n_frames)
{
    if (!h) return fail(AIDAX_ERR_ARG, "null hub");
    if (n_frames > h->max_frames) return fail(AIDAX_ERR_ARG, "n_frames exceeds the hub's max_frames");
    if (n_frames != 0 && (!in || !out)) return fail(AIDAX_ERR_ARG, "null buffer");
    return guarded([&]() -> int {
        HubBook& b = h->book;
        HubBook::Submitted sub{};
        bool wake = false;
        {
            std::unique_lock<std::mutex> g(h->mu);
            for (;;) {
                if (!b.seated(slot)) return fail(AIDAX_ERR_ARG, "slot not attached");
                if (b.last_error != AIDAX_OK) return fail(b.take_error(), "hub: a pool pass failed to launch");      // a pass the launcher could not issue
                if (b.must_close(static_cast<uint32_t>(slot), n_frames)) {
                    const int rc = flush_locked(*h);
                    if (rc != AIDAX_OK) return rc;
                }
                // the staging buffer of the period being collected: if the pass that last used it (kHubBuffers back) has not
                // read its rows yet — a host far ahead of the GPU — wait for it WITHOUT the lock (the others keep running),
                // then look at everything again
                const int gb = b.cur;
                if (!b.guard[gb]) break;
                hipEvent_t ev = h->done[gb].get();
                if (hipEventQuery(ev) == hipSuccess) { b.guard[gb] = false; break; }
                g.unlock();
                const hipError_t we = hipEventSynchronize(ev);
                g.lock();
                if (we != hipSuccess) return fail(AIDAX_ERR_DEVICE, "hub: waiting for a pass failed");
            }
            if (n_frames != 0) std::memcpy(h->h_in[b.cur].get() + static_cast<size_t>(slot) * n_frames, in, sizeof(float) * n_frames);
            sub = b.submit(static_cast<uint32_t>(slot), n_frames);
            if (sub.first) {                                     // of a new period: its deadline
                const int64_t us = h->deadline_us < 0 ? static_cast<int64_t>(0.5e6 * n_frames / h->host_sr) : h->deadline_us;
                h->deadline = Clock::now() + std::chrono::microseconds(us);
                wake = h->deadline_us != 0;
            }
            wake = wake || sub.complete;
        }
        if (wake) h->cv.notify_one();
        if (n_frames == 0) return AIDAX_OK;
        // the previous period's output for this instance; its pass was launched a period ago
        HubBook::Verdict v = HubBook::SILENCE;
        if (sub.prev_buf >= 0) {
            hipEvent_t prev_done = h->done[sub.prev_buf].get();
            if (hipEventQuery(prev_done) != hipSuccess) HIP_TRY(hipEventSynchronize(prev_done));
        }
        {
            // The row is copied under the mutex, after checking that the buffer still holds that pass: while this thread
            // waited, further periods may have closed (deadline, another instance's block size, set_controls, detach),
            // and the pass kHubBuffers later is copied into this very buffer — a row read without the check could be
            // half of each. (A thousand floats under the lock: a fraction of a microsecond.)
            // With no previous block to hand back (first block on the seat, a changed block length) a pending give-up is taken
            // all the same, so that it marks the passes it belongs to and not a later, clean one.
            std::lock_guard<std::mutex> g(h->mu);
            if (pool_take_lp_fault(h->pool.get())) b.gave_up();
            if (sub.prev_buf >= 0) v = b.verdict(sub.prev_pass, sub.prev_buf);
            if (v == HubBook::DELIVER) std::memcpy(out, h->h_out[sub.prev_buf].get() + static_cast<size_t>(slot) * n_frames, sizeof(float) * n_frames);
        }
        if (v != HubBook::DELIVER) std::memset(out, 0, sizeof(float) * n_frames);
        if (v == HubBook::FAULT) return fail(AIDAX_ERR_DEVICE, "hub: k_mfma_lp gave up a layer hand-over in the pass of this block (silence; the pool falls back to k_mfma)");
        return AIDAX_OK;
    });
}

AIDAX_API int aidax_hub_flush(aidax_hub* h)
{
    if (!h) return fail(AIDAX_ERR_ARG, "null hub");
    std::lock_guard<std::mutex> g(h->mu);
    return flush_locked(*h);
}

AIDAX_API uint32_t aidax_hub_latency_frames(const aidax_hub* h) { return hub_read<uint32_t>(h, [](HubBook& x) { return x.latency; }); }
AIDAX_API uint32_t aidax_hub_max_frames(const aidax_hub* h) { return h ? h->max_frames : 0; }
AIDAX_API uint32_t aidax_hub_attached(const aidax_hub* h) { return hub_read<uint32_t>(h, [](HubBook& x) { return x.n_attached; }); }
AIDAX_API uint64_t aidax_hub_launches(const aidax_hub* h) { return hub_read<uint64_t>(h, [](HubBook& x) { return x.launches; }); }
AIDAX_API uint64_t aidax_hub_deadline_launches(const aidax_hub* h) { return hub_read<uint64_t>(h, [](HubBook& x) { return x.deadline_launches; }); }
AIDAX_API uint64_t aidax_hub_faults_unmapped(const aidax_hub* h) { return hub_read<uint64_t>(h, [](HubBook& x) { return x.faults_unmapped; }); }

}  // extern "C"
