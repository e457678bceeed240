// aidax_bus_reverb.hip — the feedback-delay-network reverb of every mix bus (include/aidax.h, "Bus reverbs"): k_bus_reverb.
//
// One launch works in place on the block k_mix wrote, [n_buses][n_frames]. Per bus, with its record (m[8], gq[8], a, wet, dry, on,
// epoch), x the sanitised sample of absolute frame n (NaN and +-Inf are +0.0f, then clamped to +-2^64) and d_i line i's memory (0 before
// the epoch), every operation one rounded fp32 operation and none of them fused:
//     s_i = d_i[n - m_i]        t_i = d_i[n - m_i - 1]        f_i = s_i + a * (t_i - s_i)
//     h   = the unnormalised Hadamard butterfly of f, strides 1, 2, 4 (the stride bit clear: lo + hi, its partner: lo - hi)
//     d_i[n] = x + gq_i * h_i
//     w   = ((s_0 - s_1) + (s_2 - s_3)) + ((s_4 - s_5) + (s_6 - s_7))        out[n] = dry * x + wet * w
// Frame n reads nothing younger than n - m_min, so the frames of a chunk of K <= m_min are independent of one another: a lane is a frame,
// K is the largest multiple of 64 that is at most min(m_min, 256), and a pass is a chain of ceil(n_frames / K) chunks.
//
// One workgroup of 256 threads per bus; it leaves at once when the bus's reverb is off. The memories are the bus's eight ring rows in
// HBM (frame k in slot k & mask; the launch appends the pass's frames, and no slot it writes holds a frame the pass still reads: a row is
// at least max_delay + 1 + max_frames long). A chunk stores its d_i with plain vector stores, and __syncthreads() between two chunks is
// the workgroup-scope release and acquire (it waits for the stores) and the barrier that make them visible to the next chunk's loads,
// which other waves of the same workgroup issue. The sixteen taps of a frame are sixteen loads in flight per lane, neighbouring lanes on
// neighbouring addresses. No LDS, no scratch, no atomic, no order that depends on the data, and every ring index is masked.
#include <hip/hip_runtime.h>
#include <cstdint>
#include "aidax_kernels.h"

namespace aidax {

namespace {

constexpr uint32_t kRevThreads = 256;          // threads of a workgroup, the longest chunk

__global__ __launch_bounds__(kRevThreads) void k_bus_reverb(BusReverbArgs a)
{
    const uint32_t tid = threadIdx.x, bus = blockIdx.x;
    const ReverbRec& r = a.rec[bus];
    if (r.on == 0u) return;                                                // (the whole workgroup's: one bus)

    // (the host admits no record beyond these bounds; held to them here as well, they bound every ring index and the chunk below)
    uint32_t m[kReverbLines], m_min = a.max_delay;
    float gq[kReverbLines];
#pragma unroll
    for (uint32_t i = 0; i < kReverbLines; ++i) {
        m[i] = min(max(r.m[i], kReverbMinDelay), a.max_delay);
        m_min = min(m_min, m[i]);
        gq[i] = r.gq[i];
    }
    const float damp = r.a, wet = r.wet, dry = r.dry;
    const uint32_t epoch = r.epoch, mask = a.mask;
    const uint32_t K = min(m_min, kRevThreads) & ~63u;                     // 64, 128, 192 or 256
    const size_t row = static_cast<size_t>(mask) + 1u;
    float* ring = a.ring + static_cast<size_t>(bus) * kReverbLines * row;
    float* blk = a.block + static_cast<size_t>(bus) * a.n_frames;

    for (uint32_t c0 = 0; c0 < a.n_frames; c0 += K) {
        if (c0 != 0u) __syncthreads();                                     // the chunk before this one has stored its d_i: they are visible from here on
        const uint32_t t = c0 + tid;
        if (tid >= K || t >= a.n_frames) continue;
        const uint32_t n = a.pos + t;
        float s[kReverbLines], u[kReverbLines];
#pragma unroll
        for (uint32_t i = 0; i < kReverbLines; ++i) {                      // the taps: all sixteen loads ahead of their uses
            const uint32_t j = n - m[i];
            s[i] = ring[i * row + (j & mask)];
            u[i] = ring[i * row + ((j - 1u) & mask)];
        }
        float x = blk[t];
        x = __builtin_fabsf(x) < __builtin_inff() ? x : 0.f;              // (false for a NaN)
        x = __builtin_fminf(__builtin_fmaxf(x, -0x1p64f), 0x1p64f);
        float f[kReverbLines];
#pragma unroll
        for (uint32_t i = 0; i < kReverbLines; ++i) {
            const uint32_t j = n - m[i];
            s[i] = static_cast<int32_t>(j - epoch) >= 0 ? s[i] : 0.f;      // a frame before the epoch: 0, whatever the slot holds
            u[i] = static_cast<int32_t>(j - 1u - epoch) >= 0 ? u[i] : 0.f;
            f[i] = __fadd_rn(s[i], __fmul_rn(damp, __fsub_rn(u[i], s[i])));
        }
#pragma unroll
        for (uint32_t st = 1; st < kReverbLines; st <<= 1)
#pragma unroll
            for (uint32_t i = 0; i < kReverbLines; ++i)
                if ((i & st) == 0u) {
                    const float lo = f[i], hi = f[i + st];
                    f[i] = __fadd_rn(lo, hi);
                    f[i + st] = __fsub_rn(lo, hi);
                }
#pragma unroll
        for (uint32_t i = 0; i < kReverbLines; ++i) ring[i * row + (n & mask)] = __fadd_rn(x, __fmul_rn(gq[i], f[i]));
        const float w = __fadd_rn(__fadd_rn(__fsub_rn(s[0], s[1]), __fsub_rn(s[2], s[3])), __fadd_rn(__fsub_rn(s[4], s[5]), __fsub_rn(s[6], s[7])));
        blk[t] = __fadd_rn(__fmul_rn(dry, x), __fmul_rn(wet, w));
    }
}

}  // namespace

hipError_t launch_bus_reverb(const BusReverbArgs& a, hipStream_t q)
{
    if (a.n_buses == 0 || a.n_frames == 0) return hipSuccess;
    k_bus_reverb<<<a.n_buses, kRevThreads, 0, q>>>(a);
    return hipGetLastError();
}

}  // namespace aidax
