// aidax_pool_io.cpp — the pool's host-buffer entry points (aidax_pool.h): the blocking aidax_pool_process, the pipelined submit /
// collect pair with registered caller buffers, and aidax_pool_sync; with the buffers each path owns. Host logic only.
#include <hip/hip_runtime_api.h>

#include <chrono>

#include "aidax_pool.h"

static constexpr size_t kStagingLimit = size_t(64) << 20;      // pinned staging per direction for aidax_pool_process
static constexpr size_t kZeroCopyLimit = size_t(64) << 10;     // blocks up to this size are read / written by the kernels in place in pinned host memory

// Poll done() for up to ~2 ms (a block that takes longer is not a real-time block; no interrupt, no wake-up of a blocked thread on the
// way back), looking at the clock once in mask + 1 polls. Returns whether done() came true: if not, the caller waits the usual way.
template <class Done> static bool spin_until(Done&& done, uint32_t mask)
{
    const auto t0 = std::chrono::steady_clock::now();
    uint32_t polls = 0;
    while (!done()) {
        if ((++polls & mask) == 0 && std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(2)) return false;
#if defined(__x86_64__)
        __builtin_ia32_pause();
#endif
    }
    return true;
}

void BlockingIo::alloc(size_t block_floats, int device)
{
    { const char* kw = std::getenv("AIDAX_KERNEL_WORD"); kernel_word = !(kw && kw[0] == '0'); }
    const size_t block_bytes = sizeof(float) * block_floats;
    d_in.alloc(block_floats);
    d_out.alloc(block_floats);
    if (block_bytes <= kStagingLimit) {
        h_in.alloc(block_floats);
        h_out.alloc(block_floats);
        const char* zc = std::getenv("AIDAX_ZEROCOPY");
        if (block_bytes <= kZeroCopyLimit && !(zc && zc[0] == '0')) {
            hd_in = h_in.device();
            hd_out = h_out.device();
            zero_copy = true;
            const char* sp = std::getenv("AIDAX_SPIN_WAIT");
            int can = 0;
            (void)hipDeviceGetAttribute(&can, hipDeviceAttributeCanUseStreamWaitValue, device);
            if (can && !(sp && sp[0] == '0')) {
                h_done.alloc(16);
                hd_done = h_done.device();
                *h_done.get() = 0;
                spin_wait = true;
            }
        }
    }
}

void Pipeline::alloc(size_t cap_floats)
{
    Pipeline fresh;
    fresh.q_up.create();
    fresh.q_down.create();
    for (int k = 0; k < kPipeSets; ++k) {
        fresh.h_in[k].alloc(cap_floats);
        fresh.h_out[k].alloc(cap_floats);
        fresh.d_in[k].alloc(cap_floats);
        fresh.d_out[k].alloc(cap_floats);
        fresh.ev_up[k].create();
        fresh.ev_pass[k].create();
        fresh.ev_down[k].create();
    }
    fresh.ready = true;
    *this = std::move(fresh);
}

extern "C" {

AIDAX_API int aidax_pool_process(aidax_pool* p, const float* in, float* out, uint32_t n_frames)
{
    if (!p) return fail(AIDAX_ERR_ARG, "null pool");
    if (n_frames > p->max_frames) return fail(AIDAX_ERR_ARG, "n_frames exceeds the pool's max_frames");
    if (n_frames != 0 && (!in || !out)) return fail(AIDAX_ERR_ARG, "null buffer");
    return guarded([&]() -> int {
        HIP_TRY(hipSetDevice(p->device));
        const size_t bytes = sizeof(float) * p->n_streams * static_cast<size_t>(n_frames);
        int rc;
        BlockingIo& io = p->io;
        PassEnd end;                                        // the completion word, for a pass whose one workgroup can write it
        const bool staged = static_cast<bool>(io.h_in);      // (no pinned staging: pageable copies from and to the caller's buffers — and no zero_copy or spin_wait, which aidax_pool_create sets only behind h_in)
        if (bytes && staged) std::memcpy(io.h_in.get(), in, bytes);
        if (io.zero_copy) {
            // small blocks (the one-instance plugin): the pass reads its input straight from pinned host memory;
            // a pass whose form allows it also writes its output there, every other pass works in place on d_out
            const PassForm form = p->resolved_playing_form(n_frames);      // (once: launch executes this one)
            const bool direct = form.host_in_place;
            if (direct && io.spin_wait && io.kernel_word) { end.word = io.hd_done; end.seq = io.done_seq + 1; }
            rc = pool_process_prefix(p, io.hd_in, direct ? io.hd_out : io.d_out.get(), n_frames, p->q, p->n_streams, &end, &form);
            if (rc != AIDAX_OK) return rc;
            if (!direct && bytes) HIP_TRY(hipMemcpyAsync(io.h_out.get(), io.d_out.get(), bytes, hipMemcpyDeviceToHost, p->q));
        } else {
            if (bytes) HIP_TRY(hipMemcpyAsync(io.d_in.get(), staged ? io.h_in.get() : in, bytes, hipMemcpyHostToDevice, p->q));
            rc = pool_process_prefix(p, io.d_in.get(), io.d_out.get(), n_frames, p->q, p->n_streams);
            if (rc != AIDAX_OK) return rc;
            if (bytes) HIP_TRY(hipMemcpyAsync(staged ? io.h_out.get() : out, io.d_out.get(), bytes, hipMemcpyDeviceToHost, p->q));
        }
        const uint32_t seq = io.spin_wait ? ++io.done_seq : 0;
        if (io.spin_wait && !end.word_taken && hipStreamWriteValue32(p->q, io.hd_done, seq, 0) != hipSuccess) {      // (taken: the pass writes it itself) — a runtime without stream memory operations
            (void)hipGetLastError();
            io.spin_wait = false;
        }
        if (io.spin_wait) {
            volatile uint32_t* w = io.h_done.get();
            if (!spin_until([&] { return *w == seq; }, 1023u)) HIP_TRY(hipStreamSynchronize(p->q));
            std::atomic_thread_fence(std::memory_order_acquire);
        } else {
            HIP_TRY(hipStreamSynchronize(p->q));
        }
        if (p->take_lp_fault()) {                           // the pass is wrong: silence, and k_mfma from the next one on
            if (bytes) std::memset(out, 0, bytes);
            return fail(AIDAX_ERR_DEVICE, "k_mfma_lp: a layer hand-over timed out (this block is silence; the pool falls back to k_mfma)");
        }
        if (bytes && staged) std::memcpy(out, io.h_out.get(), bytes);
        return AIDAX_OK;
    });
}

// The blocking call of a host that wants the buses only: the plain staged path of aidax_pool_process up to the pass, which runs into the
// pool's own device block; then the bus block alone comes down, through the mix stage's pinned staging.
AIDAX_API int aidax_pool_process_buses(aidax_pool* p, const float* in, float* bus_out, uint32_t n_frames)
{
    if (!p) return fail(AIDAX_ERR_ARG, "null pool");
    if (n_frames > p->max_frames) return fail(AIDAX_ERR_ARG, "n_frames exceeds the pool's max_frames");
    if (n_frames != 0 && (!in || !bus_out)) return fail(AIDAX_ERR_ARG, "null buffer");
    if (!p->mix.on) return fail(AIDAX_ERR_STATE, "the pool's buses are off (aidax_pool_set_buses)");
    return guarded([&]() -> int {
        HIP_TRY(hipSetDevice(p->device));
        const size_t bytes = sizeof(float) * p->n_streams * static_cast<size_t>(n_frames);
        const size_t bus_bytes = sizeof(float) * p->mix.book.n_buses * static_cast<size_t>(n_frames);
        BlockingIo& io = p->io;
        const bool staged = static_cast<bool>(io.h_in);
        if (bytes && staged) std::memcpy(io.h_in.get(), in, bytes);
        if (bytes) HIP_TRY(hipMemcpyAsync(io.d_in.get(), staged ? io.h_in.get() : in, bytes, hipMemcpyHostToDevice, p->q));
        const int rc = pool_process_prefix(p, io.d_in.get(), io.d_out.get(), n_frames, p->q, p->n_streams);
        if (rc != AIDAX_OK) return rc;
        if (bus_bytes) HIP_TRY(hipMemcpyAsync(p->mix.h_bus.get(), p->mix.d_bus.get(), bus_bytes, hipMemcpyDeviceToHost, p->q));
        HIP_TRY(hipStreamSynchronize(p->q));
        if (p->take_lp_fault()) {                           // the pass is wrong: silence, and k_mfma from the next one on
            if (bus_bytes) std::memset(bus_out, 0, bus_bytes);
            return fail(AIDAX_ERR_DEVICE, "k_mfma_lp: a layer hand-over timed out (this block is silence; the pool falls back to k_mfma)");
        }
        if (bus_bytes) std::memcpy(bus_out, p->mix.h_bus.get(), bus_bytes);
        return AIDAX_OK;
    });
}

// ---- the pipelined host-buffer path. One caller thread (the audio side); at most two blocks between submit and collect.
static int pool_submit_impl(aidax_pool* p, const float* in, float* out, uint32_t n_frames)
{
    if (!p) return fail(AIDAX_ERR_ARG, "null pool");
    if (n_frames == 0 || n_frames > p->max_frames) return fail(AIDAX_ERR_ARG, "n_frames out of range");
    if (!in) return fail(AIDAX_ERR_ARG, "null buffer");
    return guarded([&]() -> int {
        HIP_TRY(hipSetDevice(p->device));
        auto& pl = p->pipe;
        if (!pl.ready) pl.alloc(p->n_streams * static_cast<size_t>(p->max_frames));      // first call: not a real-time call
        if (pl.submitted - pl.collected >= static_cast<uint64_t>(kPipeSets)) return fail(AIDAX_ERR_STATE, "three blocks are in flight: collect one first");
        const int s = static_cast<int>(pl.submitted % kPipeSets);
        const size_t bytes = sizeof(float) * p->n_streams * static_cast<size_t>(n_frames);
        // set s was last used by block k-3, which has been collected: its pass and both its copies are complete
        const float* up_from = in;                          // a registered caller buffer is uploaded as it lies
        if (!p->host_registered(in, bytes)) {
            std::memcpy(pl.h_in[s].get(), in, bytes);
            up_from = pl.h_in[s].get();
        }
        HIP_TRY(hipMemcpyAsync(pl.d_in[s].get(), up_from, bytes, hipMemcpyHostToDevice, pl.q_up));
        HIP_TRY(hipEventRecord(pl.ev_up[s].get(), pl.q_up));
        p->enter_stream(p->q);
        HIP_TRY(hipStreamWaitEvent(p->q, pl.ev_up[s].get(), 0));
        // (a launch that can carry the "pass done" event on its dispatch packet saves the marker packet behind the pass: 78 -> 72.5 us per
        // cfg2 block, profiles/r06_host_pipeline.txt)
        PassEnd end;
        end.done = pl.ev_pass[s].get();
        const int rc = pool_process_prefix(p, pl.d_in[s].get(), pl.d_out[s].get(), n_frames, p->q, p->n_streams, &end);
        if (rc != AIDAX_OK) return rc;
        if (!end.done_taken) HIP_TRY(hipEventRecord(pl.ev_pass[s].get(), p->q));
        HIP_TRY(hipStreamWaitEvent(pl.q_down, pl.ev_pass[s].get(), 0));
        pl.direct_out[s] = (out && p->host_registered(out, bytes)) ? out : nullptr;
        HIP_TRY(hipMemcpyAsync(pl.direct_out[s] ? pl.direct_out[s] : pl.h_out[s].get(), pl.d_out[s].get(), bytes, hipMemcpyDeviceToHost, pl.q_down));
        HIP_TRY(hipEventRecord(pl.ev_down[s].get(), pl.q_down));
        pl.frames[s] = n_frames;
        ++pl.submitted;
        return AIDAX_OK;
    });
}

AIDAX_API int aidax_pool_submit(aidax_pool* p, const float* in, uint32_t n_frames) { return pool_submit_impl(p, in, nullptr, n_frames); }

AIDAX_API int aidax_pool_submit_to(aidax_pool* p, const float* in, float* out, uint32_t n_frames)
{
    if (!out) return fail(AIDAX_ERR_ARG, "null buffer");
    return pool_submit_impl(p, in, out, n_frames);
}

AIDAX_API int aidax_pool_register_host(aidax_pool* p, void* base, size_t bytes)
{
    if (!p || !base || bytes == 0) return fail(AIDAX_ERR_ARG, "null range");
    return guarded([&]() -> int {
        HIP_TRY(hipSetDevice(p->device));
        for (const auto& r : p->host_ranges)
            if (r.base == static_cast<char*>(base)) return fail(AIDAX_ERR_STATE, "range is registered already");
        HIP_TRY(hipHostRegister(base, bytes, hipHostRegisterDefault));
        p->host_ranges.push_back({ static_cast<char*>(base), bytes });
        return AIDAX_OK;
    });
}

AIDAX_API int aidax_pool_unregister_host(aidax_pool* p, void* base)
{
    if (!p || !base) return fail(AIDAX_ERR_ARG, "null range");
    return guarded([&]() -> int {
        HIP_TRY(hipSetDevice(p->device));
        for (size_t i = 0; i < p->host_ranges.size(); ++i)
            if (p->host_ranges[i].base == static_cast<char*>(base)) {
                // copies to or from the range that are still in flight finish first
                if (p->pipe.q_up) HIP_TRY(hipStreamSynchronize(p->pipe.q_up));
                if (p->pipe.q_down) HIP_TRY(hipStreamSynchronize(p->pipe.q_down));
                HIP_TRY(hipHostUnregister(base));
                p->host_ranges.erase(p->host_ranges.begin() + static_cast<long>(i));
                return AIDAX_OK;
            }
        return fail(AIDAX_ERR_ARG, "range was not registered");
    });
}

AIDAX_API int aidax_pool_collect(aidax_pool* p, float* out, uint32_t n_frames)
{
    if (!p || !out) return fail(AIDAX_ERR_ARG, "null argument");
    return guarded([&]() -> int {
        auto& pl = p->pipe;
        if (!pl.ready || pl.collected == pl.submitted) return fail(AIDAX_ERR_STATE, "nothing was submitted");
        const int s = static_cast<int>(pl.collected % kPipeSets);
        if (pl.frames[s] != n_frames) return fail(AIDAX_ERR_ARG, "n_frames differs from the submitted block's");
        if (pl.direct_out[s] && pl.direct_out[s] != out) return fail(AIDAX_ERR_ARG, "collect: the block was submitted with another destination");
        HIP_TRY(hipSetDevice(p->device));
        if (hipEventQuery(pl.ev_down[s].get()) != hipSuccess) {
            // like aidax_pool_process: poll, then wait the usual way
            bool done = false;
            if (p->spin_collect) {
                done = spin_until([&] { return hipEventQuery(pl.ev_down[s].get()) == hipSuccess; }, 63u);
                (void)hipGetLastError();                        // (hipErrorNotReady of the polls)
            }
            if (!done) HIP_TRY(hipEventSynchronize(pl.ev_down[s].get()));
        }
        ++pl.collected;
        const size_t bytes = sizeof(float) * p->n_streams * static_cast<size_t>(n_frames);
        if (p->take_lp_fault()) {
            std::memset(out, 0, bytes);
            return fail(AIDAX_ERR_DEVICE, "k_mfma_lp: a layer hand-over timed out (this block is silence; the pool falls back to k_mfma)");
        }
        if (!pl.direct_out[s]) std::memcpy(out, pl.h_out[s].get(), bytes);
        return AIDAX_OK;
    });
}

AIDAX_API int aidax_pool_sync(aidax_pool* p)
{
    if (!p) return fail(AIDAX_ERR_ARG, "null pool");
    return guarded([&]() -> int {
        HIP_TRY(hipSetDevice(p->device));
        p->sync_issued();
        HIP_TRY(hipStreamSynchronize(p->q));
        if (p->pipe.q_down) HIP_TRY(hipStreamSynchronize(p->pipe.q_down));
        // k_mfma_lp: did a layer hand-over of a pass since the last report give up waiting?
        if (p->take_lp_fault()) return fail(AIDAX_ERR_DEVICE, "k_mfma_lp: a layer hand-over timed out (a pass since the last sync is invalid; the pool falls back to k_mfma)");
        return AIDAX_OK;
    });
}

}  // extern "C"
