// aidax_hip_host.h — what every host source that issues HIP calls for a pool shares: the error plumbing (HIP_TRY throws HipFail, guarded
// turns it into AIDAX_ERR_DEVICE) and, in the test build, the call counting behind aidax_test_hip_calls. Include it last: its macros
// rename the calls of the source that follow it (aidax_snapshot_ring.h, aidax_model_bank.h, aidax_stream_stages.h and aidax_pool.h include it and are counted: they go last too).
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
// HIP_TRY or not), each IR stage launcher, the meters' (launch_meter), the gate's (launch_gate), the mix buses' (launch_mix), the bus reverbs' (launch_bus_reverb) and the bus limiters' (launch_bus_limit), read and cleared by aidax_test_hip_calls (aidax_pool.cpp). ONE fixed table per thread for
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
#define launch_mix(...) (aidax::note_hip_call("launch_mix"), aidax::launch_mix(__VA_ARGS__))
#define launch_bus_limit(...) (aidax::note_hip_call("launch_bus_limit"), aidax::launch_bus_limit(__VA_ARGS__))
#define launch_bus_reverb(...) (aidax::note_hip_call("launch_bus_reverb"), aidax::launch_bus_reverb(__VA_ARGS__))
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
