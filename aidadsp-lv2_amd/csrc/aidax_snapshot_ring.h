// aidax_snapshot_ring.h — how host records reach the device: from a ring of pinned snapshots that nothing overwrites while an upload is
// in flight, stream-ordered with the pass that follows (the pool's control records, the model bank's per-stream records, the IR plan).
// What is to go up is a DirtyRange (aidax_stage_book.h, no HIP). It issues HIP calls and includes aidax_hip_host.h itself: include it where
// that header would go, last.
#pragma once

#include <algorithm>
#include <cstring>
#include <utility>

#include "aidax_stage_book.h"
#include "aidax_hip_host.h"

namespace aidax {

constexpr int kRing = 4;                                 // snapshots in flight

struct SnapshotRing {
    PinnedBuf<uint8_t> snap[kRing];
    Event ev[kRing];
    bool used[kRing] = {};
    int next = 0;

    void alloc(size_t bytes)                             // (set-up and worker side) all four or, where one fails, nothing
    {
        SnapshotRing fresh;
        for (int k = 0; k < kRing; ++k) {
            fresh.snap[k].alloc(bytes);
            fresh.ev[k].create();
        }
        *this = std::move(fresh);
    }
    // An upload is take(), fill what it returns, send(): the next snapshot (waited for only if its last upload, four back, is still in
    // flight: not seen in practice), then its bytes [off, off + bytes) to the same offset of `d_dst` on `s`, asynchronously.
    uint8_t* take()
    {
        if (used[next] && hipEventQuery(ev[next].get()) != hipSuccess) HIP_TRY(hipEventSynchronize(ev[next].get()));
        return snap[next].get();
    }
    void send(void* d_dst, size_t off, size_t bytes, hipStream_t s)
    {
        HIP_TRY(hipMemcpyAsync(static_cast<uint8_t*>(d_dst) + off, snap[next].get() + off, bytes, hipMemcpyHostToDevice, s));
        HIP_TRY(hipEventRecord(ev[next].get(), s));
        used[next] = true;
        next = (next + 1) % kRing;
    }
    // records [lo, hi] of h to the same records of d (HostRec: the host's name for the device's record, where a HIP-free book keeps it)
    template <class Rec, class HostRec>
    void upload_dirty(Rec* d, const HostRec* h, DirtyRange& dirty, hipStream_t s)
    {
        static_assert(sizeof(HostRec) == sizeof(Rec), "the host's record is the device's");
        if (dirty.empty()) return;
        const size_t off = sizeof(Rec) * dirty.lo, bytes = sizeof(Rec) * (static_cast<size_t>(dirty.hi - dirty.lo) + 1);
        std::memcpy(take() + off, h + dirty.lo, bytes);
        send(d, off, bytes, s);
        dirty.clear();
    }
};

}  // namespace aidax
