// aidax_hip_host.h — what every host source that issues HIP calls for a pool shares: the error plumbing (HIP_TRY throws HipFail, guarded
// turns it into AIDAX_ERR_DEVICE), the owners of device memory, pinned memory, events and streams (DevBuf, PinnedBuf, Event, Stream: the
// ONE place that frees them) and, in the test build, the call counting behind aidax_test_hip_calls. Include it last: its macros rename the
// calls of the source that follow it, the owners' among them (aidax_snapshot_ring.h, aidax_model_bank.h, aidax_stream_stages.h and
// aidax_pool.h include it and are counted: they go last too).
#pragma once

#include <hip/hip_runtime_api.h>

#include <cstdio>
#include <cstring>
#include <sstream>
#include <stdexcept>

#include "aidax_internal.h"
#include "aidax_kernels.h"

#ifdef AIDAX_TEST_HOOKS
// Test build only: per thread, how often the pool's sources call each HIP runtime entry point they use (every call site, checked with
// HIP_TRY or not), each IR stage launcher, the meters' (launch_meter), the gate's (launch_gate), the tuners' (launch_tune), the mix buses' (launch_mix), the bus reverbs' (launch_bus_reverb), the stream delays' (launch_delay) and the bus limiters' (launch_bus_limit), read and cleared by aidax_test_hip_calls (aidax_pool.cpp). ONE fixed table per thread for
// every source (an inline function's static): counting allocates nothing.
// (tests/test_gpu_ir_bank_rt.py: the audio-thread calls allocate, free and wait for nothing.)
namespace aidax {
struct HipCallTable { const char* name[48]; uint64_t n[48]; int used; };
inline HipCallTable& hip_call_table() { static thread_local HipCallTable t{}; return t; }
inline void note_hip_call(const char* name)
{
    HipCallTable& t = hip_call_table();
    for (int i = 0; i < t.used; ++i)
        if (std::strcmp(t.name[i], name) == 0) { ++t.n[i]; return; }
    if (t.used < 48) { t.name[t.used] = name; t.n[t.used++] = 1; }
}
// aidax_test_hip_calls: the calling thread's counted calls since the last read, one "name count" line each, into `buf` (NUL-terminated,
// cut at `cap` bytes); returns the number of entry points listed and starts the count afresh
inline int read_hip_calls(char* buf, uint32_t cap)
{
    HipCallTable& t = hip_call_table();
    size_t at = 0;
    if (buf && cap) buf[0] = '\0';
    for (int i = 0; i < t.used; ++i)
        if (buf && at < cap) {
            const int w = std::snprintf(buf + at, cap - at, "%s %llu\n", t.name[i], static_cast<unsigned long long>(t.n[i]));
            if (w > 0) at += static_cast<size_t>(w);
        }
    const int n = t.used;
    t.used = 0;
    return n;
}
}  // namespace aidax
#define AIDAX_COUNTED(fn, ...) (aidax::note_hip_call(#fn), ::fn(__VA_ARGS__))
#define hipSetDevice(...) AIDAX_COUNTED(hipSetDevice, __VA_ARGS__)
#define hipMalloc(...) AIDAX_COUNTED(hipMalloc, __VA_ARGS__)
#define hipHostMalloc(...) AIDAX_COUNTED(hipHostMalloc, __VA_ARGS__)
#define hipHostRegister(...) AIDAX_COUNTED(hipHostRegister, __VA_ARGS__)
#define hipEventCreateWithFlags(...) AIDAX_COUNTED(hipEventCreateWithFlags, __VA_ARGS__)
#define hipStreamCreateWithFlags(...) AIDAX_COUNTED(hipStreamCreateWithFlags, __VA_ARGS__)
#define hipStreamCreateWithPriority(...) AIDAX_COUNTED(hipStreamCreateWithPriority, __VA_ARGS__)
#define hipFree(...) AIDAX_COUNTED(hipFree, __VA_ARGS__)
#define hipHostFree(...) AIDAX_COUNTED(hipHostFree, __VA_ARGS__)
#define hipHostUnregister(...) AIDAX_COUNTED(hipHostUnregister, __VA_ARGS__)
#define hipEventDestroy(...) AIDAX_COUNTED(hipEventDestroy, __VA_ARGS__)
#define hipStreamDestroy(...) AIDAX_COUNTED(hipStreamDestroy, __VA_ARGS__)
#define hipStreamSynchronize(...) AIDAX_COUNTED(hipStreamSynchronize, __VA_ARGS__)
#define hipEventSynchronize(...) AIDAX_COUNTED(hipEventSynchronize, __VA_ARGS__)
#define hipDeviceSynchronize(...) AIDAX_COUNTED(hipDeviceSynchronize, __VA_ARGS__)
#define hipMemcpy(...) AIDAX_COUNTED(hipMemcpy, __VA_ARGS__)
#define hipMemcpyAsync(...) AIDAX_COUNTED(hipMemcpyAsync, __VA_ARGS__)
#define hipMemsetAsync(...) AIDAX_COUNTED(hipMemsetAsync, __VA_ARGS__)
#define hipEventRecord(...) AIDAX_COUNTED(hipEventRecord, __VA_ARGS__)
#define hipEventQuery(...) AIDAX_COUNTED(hipEventQuery, __VA_ARGS__)
#define hipStreamWaitEvent(...) AIDAX_COUNTED(hipStreamWaitEvent, __VA_ARGS__)
#define hipStreamWriteValue32(...) AIDAX_COUNTED(hipStreamWriteValue32, __VA_ARGS__)
#define launch_ir_append(...) (aidax::note_hip_call("launch_ir_append"), aidax::launch_ir_append(__VA_ARGS__))
#define launch_ir_conv(...) (aidax::note_hip_call("launch_ir_conv"), aidax::launch_ir_conv(__VA_ARGS__))
#define launch_ir_fade(...) (aidax::note_hip_call("launch_ir_fade"), aidax::launch_ir_fade(__VA_ARGS__))
#define launch_ir_mix(...) (aidax::note_hip_call("launch_ir_mix"), aidax::launch_ir_mix(__VA_ARGS__))
#define launch_meter(...) (aidax::note_hip_call("launch_meter"), aidax::launch_meter(__VA_ARGS__))
#define launch_gate(...) (aidax::note_hip_call("launch_gate"), aidax::launch_gate(__VA_ARGS__))
#define launch_tune(...) (aidax::note_hip_call("launch_tune"), aidax::launch_tune(__VA_ARGS__))
#define launch_mix(...) (aidax::note_hip_call("launch_mix"), aidax::launch_mix(__VA_ARGS__))
#define launch_bus_limit(...) (aidax::note_hip_call("launch_bus_limit"), aidax::launch_bus_limit(__VA_ARGS__))
#define launch_bus_reverb(...) (aidax::note_hip_call("launch_bus_reverb"), aidax::launch_bus_reverb(__VA_ARGS__))
#define launch_delay(...) (aidax::note_hip_call("launch_delay"), aidax::launch_delay(__VA_ARGS__))
#endif

namespace aidax {

struct HipFail : std::runtime_error { using std::runtime_error::runtime_error; };

inline void hip_check(hipError_t e, const char* what)
{
    if (e != hipSuccess) {
        std::ostringstream os;
        os << what << ": " << hipGetErrorString(e);
        throw HipFail(os.str());
    }
}
#define HIP_TRY(x) aidax::hip_check((x), #x)

// Who owns what on the device: a hipMalloc block (DevBuf), a pinned host block (PinnedBuf), an event without timing (Event) and a stream
// (Stream). Move-only; an empty one issues no HIP call when it is reset or destroyed (the call-count tests depend on it); alloc / create
// throw HipFail and leave the owner as it was. Kernel arguments and launchers take get() (a Stream converts). A struct's members are destroyed in reverse
// declaration order: one that declares its Streams first frees every block ahead of its streams.
template <class T>
class DevBuf {
    T* p_ = nullptr;

  public:
    DevBuf() = default;
    DevBuf(DevBuf&& o) noexcept : p_(o.p_) { o.p_ = nullptr; }
    DevBuf& operator=(DevBuf&& o) noexcept
    {
        if (this != &o) { reset(); p_ = o.p_; o.p_ = nullptr; }
        return *this;
    }
    ~DevBuf() { reset(); }
    // A block whose pointer travelled through a host-only record (IrSlot, BankSlot: the books swap them and the sanitizer harnesses fill
    // them with made-up addresses, so they stay plain) comes back under an owner where the record's life ends
    static DevBuf adopt(T* p) { DevBuf b; b.p_ = p; return b; }
    void alloc(size_t count)
    {
        T* p = nullptr;
        HIP_TRY(hipMalloc(reinterpret_cast<void**>(&p), sizeof(T) * count));
        reset();
        p_ = p;
    }
    // elements [first, first + count) zeroed on q: what a stage's enable() does to each block a pass must find cleared, and a restart to its runs
    void zero(size_t first, size_t count, hipStream_t q) const { HIP_TRY(hipMemsetAsync(p_ + first, 0, sizeof(T) * count, q)); }
    T* get() const { return p_; }
    T* release() { T* p = p_; p_ = nullptr; return p; }      // (into such a record)
    explicit operator bool() const { return p_ != nullptr; }
    void reset()
    {
        if (p_) (void)hipFree(p_);
        p_ = nullptr;
    }
};

template <class T>
class PinnedBuf {
    T* p_ = nullptr;

  public:
    PinnedBuf() = default;
    PinnedBuf(PinnedBuf&& o) noexcept : p_(o.p_) { o.p_ = nullptr; }
    PinnedBuf& operator=(PinnedBuf&& o) noexcept
    {
        if (this != &o) { reset(); p_ = o.p_; o.p_ = nullptr; }
        return *this;
    }
    ~PinnedBuf() { reset(); }
    void alloc(size_t count)
    {
        T* p = nullptr;
        HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&p), sizeof(T) * count, hipHostMallocDefault));
        reset();
        p_ = p;
    }
    T* get() const { return p_; }
    T* device() const                                        // the block as the device addresses it (zero-copy passes, the fault and completion words)
    {
        T* d = nullptr;
        HIP_TRY(hipHostGetDevicePointer(reinterpret_cast<void**>(&d), p_, 0));
        return d;
    }
    explicit operator bool() const { return p_ != nullptr; }
    void reset()
    {
        if (p_) (void)hipHostFree(p_);
        p_ = nullptr;
    }
};

class Event {
    hipEvent_t e_ = nullptr;

  public:
    Event() = default;
    Event(Event&& o) noexcept : e_(o.e_) { o.e_ = nullptr; }
    Event& operator=(Event&& o) noexcept
    {
        if (this != &o) { reset(); e_ = o.e_; o.e_ = nullptr; }
        return *this;
    }
    ~Event() { reset(); }
    void create()
    {
        hipEvent_t e = nullptr;
        HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        reset();
        e_ = e;
    }
    hipEvent_t get() const { return e_; }
    explicit operator bool() const { return e_ != nullptr; }
    void reset()
    {
        if (e_) (void)hipEventDestroy(e_);
        e_ = nullptr;
    }
};

class Stream {
    hipStream_t s_ = nullptr;

  public:
    Stream() = default;
    Stream(Stream&& o) noexcept : s_(o.s_) { o.s_ = nullptr; }
    Stream& operator=(Stream&& o) noexcept
    {
        if (this != &o) { reset(); s_ = o.s_; o.s_ = nullptr; }
        return *this;
    }
    ~Stream() { reset(); }
    void create()                                            // non-blocking, default priority
    {
        hipStream_t s = nullptr;
        HIP_TRY(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
        reset();
        s_ = s;
    }
    void create(int priority)
    {
        hipStream_t s = nullptr;
        HIP_TRY(hipStreamCreateWithPriority(&s, hipStreamNonBlocking, priority));
        reset();
        s_ = s;
    }
    operator hipStream_t() const { return s_; }              // (a stream is named at every call that issues work: it reads as the handle)
    void reset()
    {
        if (s_) (void)hipStreamDestroy(s_);
        s_ = nullptr;
    }
};

// A stage's read: `bytes` from d to its pinned staging h behind everything on q, `clear_behind` (the clear of what was copied, or nothing)
// behind the copy, the wait, then out of the staging (zero bytes: the wait alone)
template <class Clear>
void read_back(void* out, void* h, const void* d, size_t bytes, hipStream_t q, Clear&& clear_behind)
{
    if (bytes) HIP_TRY(hipMemcpyAsync(h, d, bytes, hipMemcpyDeviceToHost, q));
    clear_behind();
    HIP_TRY(hipStreamSynchronize(q));
    if (bytes) std::memcpy(out, h, bytes);
}
inline void read_back(void* out, void* h, const void* d, size_t bytes, hipStream_t q) { read_back(out, h, d, bytes, q, [] {}); }

template <class F>
int guarded(F&& f)
{
    try {
        return f();
    } catch (const HipFail& e) {
        return fail(AIDAX_ERR_DEVICE, e.what());
    } catch (const std::exception& e) {
        return fail(AIDAX_ERR_STATE, e.what());
    } catch (...) {
        return fail(AIDAX_ERR_STATE, "unknown failure");
    }
}

}  // namespace aidax
