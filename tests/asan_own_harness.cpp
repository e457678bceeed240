// The owning types of aidax_hip_host.h (DevBuf, PinnedBuf, Event, Stream) and what is built from them (SnapshotRing, GateStage::enable)
// under AddressSanitizer + UndefinedBehaviorSanitizer (`make asan_own`, tests/test_asan_own.py). No HIP library is linked: the dozen
// runtime entry points the types call are defined HERE, over malloc and a book of what is live, so every create / destroy is seen, a
// second free of one handle is a failure, and the k-th creating call can be made to fail. CPU only: nothing here can touch a device.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <set>
#include <utility>

#include "aidax.h"
#include "../aidadsp-lv2_amd/csrc/aidax_stream_stages.h"

static int failures = 0, checks = 0;
#define EXPECT(c) do { ++checks; if (!(c)) { std::fprintf(stderr, "asan_own_harness: %s failed at line %d\n", #c, __LINE__); ++failures; } } while (0)

// ---- the stub runtime
static std::set<void*> live;
static int n_made = 0, n_freed = 0, n_other = 0, bad_frees = 0;
static int fail_at = 0;                                  // the k-th creating call from now fails (0: none)

static hipError_t make(void** out, size_t bytes)
{
    if (fail_at != 0 && --fail_at == 0) return hipErrorOutOfMemory;
    *out = std::malloc(bytes ? bytes : 1);
    live.insert(*out);
    ++n_made;
    return hipSuccess;
}
static hipError_t unmake(void* p)
{
    if (live.erase(p) != 1) { ++bad_frees; return hipErrorInvalidValue; }
    std::free(p);
    ++n_freed;
    return hipSuccess;
}

extern "C" {
hipError_t hipMalloc(void** ptr, size_t size) { return make(ptr, size); }
hipError_t hipFree(void* ptr) { return unmake(ptr); }
hipError_t hipHostMalloc(void** ptr, size_t size, unsigned int) { return make(ptr, size); }
hipError_t hipHostFree(void* ptr) { return unmake(ptr); }
hipError_t hipHostGetDevicePointer(void** dev, void* host, unsigned int) { *dev = host; ++n_other; return hipSuccess; }
hipError_t hipEventCreateWithFlags(hipEvent_t* e, unsigned) { return make(reinterpret_cast<void**>(e), 1); }
hipError_t hipEventDestroy(hipEvent_t e) { return unmake(e); }
hipError_t hipStreamCreateWithFlags(hipStream_t* s, unsigned int) { return make(reinterpret_cast<void**>(s), 1); }
hipError_t hipStreamCreateWithPriority(hipStream_t* s, unsigned int, int) { return make(reinterpret_cast<void**>(s), 1); }
hipError_t hipStreamDestroy(hipStream_t s) { return unmake(s); }
hipError_t hipMemsetAsync(void*, int, size_t, hipStream_t) { ++n_other; return fail_at != 0 && --fail_at == 0 ? hipErrorInvalidValue : hipSuccess; }
hipError_t hipStreamSynchronize(hipStream_t) { ++n_other; return fail_at != 0 && --fail_at == 0 ? hipErrorInvalidValue : hipSuccess; }
hipError_t hipEventQuery(hipEvent_t) { ++n_other; return hipSuccess; }
hipError_t hipEventSynchronize(hipEvent_t) { ++n_other; return hipSuccess; }
const char* hipGetErrorString(hipError_t) { return "stub failure"; }
}

struct Counts { int made, freed, other; };
static Counts now() { return { n_made, n_freed, n_other }; }
static bool moved(const Counts& a, int made, int freed) { return n_made - a.made == made && n_freed - a.freed == freed; }

// ---- one owner type: fill(x) makes x own something. Each resource is freed exactly once, and an empty owner calls nothing.
template <class Owner, class Fill>
static void owner_rules(Fill fill)
{
    Counts c = now();
    { Owner e; e.reset(); e.reset(); Owner f(std::move(e)); f = Owner(); }
    EXPECT(moved(c, 0, 0) && n_other == c.other);                    // empty: construct, reset twice, move, assign, destroy — no call at all

    c = now();
    {
        Owner a;
        fill(a);
        EXPECT(a && moved(c, 1, 0));
        Owner b(std::move(a));                                       // move-construct: the source is empty, nothing is freed
        EXPECT(!a && b && moved(c, 1, 0));
        Owner empty_target;
        empty_target = std::move(b);                                 // move-assign over an empty target
        EXPECT(!b && empty_target && moved(c, 1, 0));
        Owner full_target;
        fill(full_target);
        EXPECT(moved(c, 2, 0));
        full_target = std::move(empty_target);                       // ... over a full one: the target's old resource goes, once
        EXPECT(!empty_target && full_target && moved(c, 2, 1));
        Owner& self = full_target;
        full_target = std::move(self);                               // self-move: kept
        EXPECT(full_target && moved(c, 2, 1));
        Owner other;
        fill(other);
        const auto p = full_target.get(), q = other.get();
        std::swap(full_target, other);                               // swap: three moves, no call
        EXPECT(full_target.get() == q && other.get() == p && moved(c, 3, 1));
        other.reset();
        other.reset();                                               // reset twice: one free
        EXPECT(!other && moved(c, 3, 2));
        fill(other);
        fill(other);                                                 // a second alloc / create replaces: the first goes
        EXPECT(other && moved(c, 5, 3));
    }
    EXPECT(moved(c, 5, 5) && live.empty() && bad_frees == 0);       // the two still owned went with their owners

    c = now();
    {
        Owner a;
        fill(a);
        const auto kept = a.get();
        fail_at = 1;
        bool threw = false;
        try { fill(a); } catch (const aidax::HipFail&) { threw = true; }
        EXPECT(threw && a.get() == kept && moved(c, 1, 0));          // a failed alloc / create leaves the owner as it was
    }
    EXPECT(moved(c, 1, 1) && live.empty());
}

// Stream converts to its handle instead of get() / operator bool: the same rules through a thin view
struct StreamView : aidax::Stream {
    StreamView() = default;
    StreamView(StreamView&&) = default;
    StreamView& operator=(StreamView&&) = default;
    hipStream_t get() const { return *this; }
    explicit operator bool() const { return get() != nullptr; }
};

static void adopt_and_release()
{
    Counts c = now();
    aidax::DevBuf<float> a;
    a.alloc(8);
    float* raw = a.release();                                        // into a plain record ...
    EXPECT(!a && raw && moved(c, 1, 0));
    a.reset();
    EXPECT(moved(c, 1, 0));
    { aidax::DevBuf<float> back = aidax::DevBuf<float>::adopt(raw); EXPECT(back.get() == raw); }      // ... and back under an owner
    EXPECT(moved(c, 1, 1));
    aidax::DevBuf<float>::adopt(nullptr);                            // an empty record: nothing
    EXPECT(moved(c, 1, 1) && live.empty());
    aidax::PinnedBuf<uint32_t> h;
    h.alloc(16);
    EXPECT(h.device() == h.get());
}

// all or nothing: SnapshotRing::alloc and GateStage::enable with the k-th call failing, for every k, over an empty and over a built target
static void all_or_nothing()
{
    for (int k = 1; k <= 2 * aidax::kRing; ++k) {
        const Counts c = now();
        aidax::SnapshotRing r;
        fail_at = k;
        bool threw = false;
        try { r.alloc(64); } catch (const aidax::HipFail&) { threw = true; }
        EXPECT(threw && !r.snap[0] && !r.ev[aidax::kRing - 1] && n_made - c.made == n_freed - c.freed && live.empty());
    }
    {
        const Counts c = now();
        { aidax::SnapshotRing r; r.alloc(64); EXPECT(moved(c, 2 * aidax::kRing, 0) && r.take() == r.snap[0].get()); }
        EXPECT(moved(c, 2 * aidax::kRing, 2 * aidax::kRing) && live.empty());
    }
    // GateStage::enable: 3 blocks, the staging, 2 clears, the wait, then the ring's 8 — fifteen calls that can fail
    for (int k = 1; k <= 15; ++k) {
        const Counts c = now();
        aidax::GateStage g;
        fail_at = k;
        bool threw = false;
        try { g.enable(5, 16, nullptr); } catch (const aidax::HipFail&) { threw = true; }
        EXPECT(threw && !g.enabled() && g.book.h_rec.empty() && n_made - c.made == n_freed - c.freed && live.empty());
    }
    fail_at = 0;
    const Counts c = now();
    {
        aidax::GateStage g;
        g.enable(5, 16, nullptr);
        EXPECT(g.enabled() && g.book.h_rec.size() == 5 && moved(c, 4 + 2 * aidax::kRing, 0));
        const auto* rec = g.d_rec.get();
        fail_at = 9;                                                 // a second enable that fails in its ring: the stage stays as it was
        bool threw = false;
        try { g.enable(7, 16, nullptr); } catch (const aidax::HipFail&) { threw = true; }
        EXPECT(threw && g.enabled() && g.d_rec.get() == rec && g.book.h_rec.size() == 5 && live.size() == 4 + 2 * aidax::kRing);
    }
    EXPECT(live.empty() && bad_frees == 0 && n_made == n_freed);
    (void)c;
}

int main()
{
    owner_rules<aidax::DevBuf<float>>([](aidax::DevBuf<float>& b) { b.alloc(8); });
    owner_rules<aidax::PinnedBuf<uint8_t>>([](aidax::PinnedBuf<uint8_t>& b) { b.alloc(8); });
    owner_rules<aidax::Event>([](aidax::Event& e) { e.create(); });
    owner_rules<StreamView>([](StreamView& s) { s.create(); });
    owner_rules<StreamView>([](StreamView& s) { s.create(1); });
    adopt_and_release();
    all_or_nothing();
    EXPECT(live.empty() && bad_frees == 0 && n_made == n_freed);
    std::printf("asan_own_harness: %d checks, %d failures\n", checks, failures);
    return failures ? 1 : 0;
}
