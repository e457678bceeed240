// aidax_delay.hip — the per-stream delay line behind the cabinet IR (include/aidax.h, "Stream delays"): k_delay.
//
// One launch works in place on the block a pass returns, [n_active][n_frames]. Per stream, with its record (m, depth_q16, lfo_step, fade,
// fb, damp, wet, dry, on) and its state (pos, m_cur, m_old, fade_len, fade_left, phase, replaced), x the sanitised sample of the line's
// frame n (NaN and +-Inf are +0.0f, then clamped to +-2^64) and d the line's memory (0 before frame 0), every fp32 operation one rounded
// operation and none of them fused:
//     u = (phase >> 8) & 0xffffff    tri = u < 2^23 ? u : 2^24 - u    off = (depth_q16 * tri) >> 23              (Q16 frames)
//     tap(M): i = min(M + (off >> 16), cap)    fr = float(off & 0xffff) * 2^-16
//             a = d[n - i], b = d[n - i - 1], c = d[n - i - 2]    p0 = a + fr * (b - a)    p1 = b + fr * (c - b)    p0 + damp * (p1 - p0)
//     f = tap(m_cur); while a fade runs (fade_left > 0): w = float(double(fade_len - fade_left) / double(fade_len)),
//                                                        f = tap(m_old) + w * (f - tap(m_old))
//     d[n] = x + fb * f        out[n] = dry * x + wet * f
// Frame n reads nothing younger than n - min(m_cur, m_old while a fade runs), so the frames of a chunk of K <= that minimum are
// independent of one another: a lane is a frame, K is the largest multiple of 64 that is at most min(256, that minimum at the pass's
// first frame), and a pass is a chain of ceil(n_frames / K) chunks. Every lane derives its own n, phase and fade_left from the state read
// at the pass's start: nothing is carried from frame to frame but the line's memory.
//
// One workgroup of 256 threads per stream; it leaves at once when the stream does not play (its delay off, or its control record without
// CTL_ENABLED: the row keeps its bits, the state does not move). The memory is the stream's ring row in HBM (frame k in slot k & mask;
// the launch appends the pass's frames, and no slot it writes holds a frame the pass still reads: a row is at least cap + 3 + max_frames
// long). A chunk stores its d with plain vector stores, and __syncthreads() between two chunks is the workgroup-scope release and acquire
// and the barrier that make them visible to the next chunk's loads, which other waves of the same workgroup issue. (Outside
// threadgroup-split mode that release is no wait for the stores' completion: the workgroup's waves share one CU, whose vector memory path
// and L1 take the stores issued ahead of the barrier and the loads issued behind it in issue order, as for k_bus_reverb.) Thread 0
// writes the state back behind the last chunk; `replaced` is counted per wave (a ballot) and summed through four words of LDS. No scratch, no atomic, no order that depends on the data, and every ring index is masked.
#include <hip/hip_runtime.h>
#include <cstdint>
#include "aidax_kernels.h"

namespace aidax {

namespace {

constexpr uint32_t kDelayThreads = 256;        // threads of a workgroup, the longest chunk

// the line's frame n - i, i >= 1: 0 before the line's frame 0, whatever the slot holds
__device__ __forceinline__ float frame_or_zero(float v, uint64_t n, uint32_t i) { return n >= i ? v : 0.f; }

// p0 + damp * (p1 - p0) of the three frames at and behind the read position
__device__ __forceinline__ float tap_value(float a, float b, float c, float fr, float damp)
{
    const float p0 = __fadd_rn(a, __fmul_rn(fr, __fsub_rn(b, a)));
    const float p1 = __fadd_rn(b, __fmul_rn(fr, __fsub_rn(c, b)));
    return __fadd_rn(p0, __fmul_rn(damp, __fsub_rn(p1, p0)));
}

__global__ __launch_bounds__(kDelayThreads) void k_delay(DelayArgs a)
{
    __shared__ uint32_t bad_of_wave[kDelayThreads / 64u];
    const uint32_t tid = threadIdx.x, s = blockIdx.x;
    const DelayRec r = a.rec[s];
    if (r.on == 0u || !(a.ctl[s].flags & CTL_ENABLED)) return;              // (the whole workgroup's: one stream)

    // the pass's first frame: a fresh line takes the record's delay, another delay starts a fade from the one in force
    // (the host admits no record beyond these bounds; held to them here as well, they bound every ring index and the chunk below)
    const DelayState st = a.state[s];
    const uint32_t cap = max(a.cap, kDelayMin), mask = a.mask;
    const uint32_t m_rec = min(max(r.m, kDelayMin), cap);
    uint32_t m_cur = st.m_cur, m_old = st.m_old, fade_len = st.fade_len, fade_left = min(st.fade_left, st.fade_len);
    if (m_cur == 0u) {
        m_cur = m_rec;
    } else if (m_rec != m_cur) {
        m_old = m_cur; m_cur = m_rec; fade_len = fade_left = min(r.fade, kDelayMaxFade);
    }
    m_cur = min(max(m_cur, kDelayMin), cap);
    m_old = fade_left != 0u ? min(max(m_old, kDelayMin), cap) : m_old;
    const uint32_t m_min = fade_left != 0u ? min(m_cur, m_old) : m_cur;
    const uint32_t K = min(m_min, kDelayThreads) & ~63u;                     // 64, 128, 192 or 256
    const uint32_t depth = min(r.depth_q16, kDelayMaxDepth << 16);
    const float fb = r.fb, damp = r.damp, wet = r.wet, dry = r.dry;
    float* ring = a.ring + static_cast<size_t>(s) * (static_cast<size_t>(mask) + 1u);
    float* blk = a.block + static_cast<size_t>(s) * a.n_frames;
    uint32_t bad = 0;                                                       // the wave's count of replaced samples

    for (uint32_t c0 = 0; c0 < a.n_frames; c0 += K) {
        if (c0 != 0u) __syncthreads();                                      // the chunk before this one has stored its d: they are visible from here on
        const uint32_t t = c0 + tid;
        const bool mine = tid < K && t < a.n_frames;
        bool replaced = false;
        if (mine) {
            const uint64_t n = st.pos + t;
            const uint32_t n32 = static_cast<uint32_t>(n);
            const uint32_t phase = st.phase + t * r.lfo_step;
            const uint32_t u = (phase >> 8) & 0xffffffu, tri = u < (1u << 23) ? u : (1u << 24) - u;
            const uint32_t off = static_cast<uint32_t>((static_cast<uint64_t>(depth) * tri) >> 23);
            const float fr = __fmul_rn(static_cast<float>(off & 0xffffu), 0x1p-16f);      // exact
            const uint32_t left = fade_left > t ? fade_left - t : 0u;
            const uint32_t i = min(m_cur + (off >> 16), cap), io = min(m_old + (off >> 16), cap);
            // the taps: every load ahead of its use
            float ta = ring[(n32 - i) & mask], tb = ring[(n32 - i - 1u) & mask], tc = ring[(n32 - i - 2u) & mask];
            float oa = 0.f, ob = 0.f, oc = 0.f;
            if (left != 0u) { oa = ring[(n32 - io) & mask]; ob = ring[(n32 - io - 1u) & mask]; oc = ring[(n32 - io - 2u) & mask]; }
            const float x_raw = blk[t];
            replaced = !(__builtin_fabsf(x_raw) < __builtin_inff());          // (true for a NaN)
            float x = replaced ? 0.f : x_raw;
            x = __builtin_fminf(__builtin_fmaxf(x, -0x1p64f), 0x1p64f);
            ta = frame_or_zero(ta, n, i); tb = frame_or_zero(tb, n, i + 1u); tc = frame_or_zero(tc, n, i + 2u);
            float f = tap_value(ta, tb, tc, fr, damp);
            if (left != 0u) {
                oa = frame_or_zero(oa, n, io); ob = frame_or_zero(ob, n, io + 1u); oc = frame_or_zero(oc, n, io + 2u);
                const float fo = tap_value(oa, ob, oc, fr, damp);
                const float w = static_cast<float>(static_cast<double>(fade_len - left) / static_cast<double>(fade_len));
                f = __fadd_rn(fo, __fmul_rn(w, __fsub_rn(f, fo)));
            }
            ring[n32 & mask] = __fadd_rn(x, __fmul_rn(fb, f));
            blk[t] = __fadd_rn(__fmul_rn(dry, x), __fmul_rn(wet, f));
        }
        bad += static_cast<uint32_t>(__popcll(__ballot(replaced)));
    }
    if ((tid & 63u) == 0u) bad_of_wave[tid >> 6] = bad;
    __syncthreads();
    if (tid == 0u) {
        DelayState next;
        next.pos = st.pos + a.n_frames;
        next.m_cur = m_cur; next.m_old = m_old; next.fade_len = fade_len;
        next.fade_left = fade_left > a.n_frames ? fade_left - a.n_frames : 0u;
        next.phase = st.phase + a.n_frames * r.lfo_step;
        next.replaced = st.replaced + ((bad_of_wave[0] + bad_of_wave[1]) + (bad_of_wave[2] + bad_of_wave[3]));
        a.state[s] = next;
    }
}

}  // namespace

hipError_t launch_delay(const DelayArgs& a, hipStream_t q)
{
    if (a.n_active == 0 || a.n_frames == 0) return hipSuccess;
    k_delay<<<a.n_active, kDelayThreads, 0, q>>>(a);
    return hipGetLastError();
}

}  // namespace aidax
