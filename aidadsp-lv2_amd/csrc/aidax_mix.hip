// aidax_mix.hip — the mix buses behind a pool's last stage (include/aidax.h, "Mix buses"): k_mix.
//
// One launch reads the block a pass returns, [n_streams][n_frames] floats, and writes the pool's bus block, [n_buses][n_frames]: bus b
// is the sum of its entries' rows, each times the gain of its send. The sum has ONE defined order (so that a bus sounds the same on
// every launch shape and in the numpy restatement of tests/mixhelp.py): the entries of a bus, in the order of the plan, are cut into
// groups of kMixGroup = 32; a group sum starts at +0.0f and adds its terms g * y in order, product and sum each rounded to fp32 (no
// fma); the bus sample starts at +0.0f and adds the group sums in group order. A term whose gain is exactly 0 is left out, whatever y
// holds (a muted send of a stream that plays NaN does not poison its bus).
//
// A gather per (bus, tile of 64 frames): one frame per lane, so every row is read in 256-byte pieces with no alignment question at odd
// block lengths, and nothing is ever added across lanes. A workgroup is WAVES waves of one tile of one bus. Wave w sums the groups
// WAVES r + w, r = 0, 1, ..: eight entries at a time, their rows' loads issued together ahead of the eight dependent adds, the entry
// records (wave-uniform) read through the scalar cache. After every round the WAVES group sums meet in LDS (two buffers: one barrier
// per round) and wave 0 adds those that exist in group order. WAVES = 1 serves a plan whose every bus has at most 32 entries (no LDS,
// no barrier), WAVES = 4 one of up to 128 (one round), WAVES = 16 every longer one: a bus of a thousand entries is four workgroups
// per 256-frame block, and what bounds it is the chain of row loads a wave waits for, two groups deep instead of eight; all three
// give the same bits. No atomic, no scratch, no order that depends on the data, and the stream block is only read.
//
// The gain of ramp frame k is ramp_value (aidax_kernels.h), in fp64: a division per entry and lane. A tile that lies behind its
// entry's ramp end as a whole (the common case: a send at rest) takes g1 without it; the branch is wave-uniform and picks between two
// ways of computing the same number.
#include <hip/hip_runtime.h>
#include <cstdint>
#include "aidax_kernels.h"

namespace aidax {

namespace {

constexpr uint32_t kMixBatch = 8;              // entries whose rows are in flight together

// the sum of the entries [lo, hi) (one group: at most kMixGroup of them) for this lane's frame t of the tile that starts at t0
__device__ __forceinline__ float group_sum(const MixArgs& a, uint32_t lo, uint32_t hi, uint32_t t0, uint32_t t, bool valid)
{
    float acc = 0.f;
    for (uint32_t i = lo; i < hi; i += kMixBatch) {
        float y[kMixBatch], g[kMixBatch];
#pragma unroll
        for (uint32_t j = 0; j < kMixBatch; ++j) {
            const MixEntry e = a.entries[min(i + j, hi - 1u)];            // (wave-uniform; a slot behind the group's end re-reads its last entry and is left out)
            const bool live = i + j < hi && e.stream < a.n_streams;
            const uint32_t k0 = e.k + a.k_off + t0;                       // (<= 2^24 + 2^25 + the block: no wrap)
            float gain = e.g1;
            if (live && k0 + 1u < e.ramp) gain = static_cast<float>(ramp_value(e.g0, e.g1, e.ramp, k0 + (t - t0)));
            g[j] = live ? gain : 0.f;
            y[j] = live && valid ? a.y[static_cast<size_t>(e.stream) * a.n_frames + t] : 0.f;
        }
#pragma unroll
        for (uint32_t j = 0; j < kMixBatch; ++j) {
            const float sum = __fadd_rn(acc, __fmul_rn(g[j], y[j]));
            acc = g[j] != 0.f ? sum : acc;
        }
    }
    return acc;
}

template <uint32_t WAVES>
__global__ __launch_bounds__(64 * WAVES) void k_mix(MixArgs a)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t w = static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x >> 6)));
    const uint32_t bus = blockIdx.y, t0 = blockIdx.x * 64u, t = t0 + lane;
    const bool valid = t < a.n_frames;
    const uint32_t lo = a.bus_start[bus], hi = a.bus_start[bus + 1u];
    const uint32_t n_groups = (hi - lo + kMixGroup - 1u) / kMixGroup;

    float sample = 0.f;
    if constexpr (WAVES == 1u) {                                          // (no LDS is declared in this form, and no barrier)
        for (uint32_t g = 0; g < n_groups; ++g)
            sample = __fadd_rn(sample, group_sum(a, lo + g * kMixGroup, min(lo + (g + 1u) * kMixGroup, hi), t0, t, valid));
    } else {
        __shared__ float part[2][WAVES][64];
        for (uint32_t g0 = 0, round = 0; g0 < n_groups; g0 += WAVES, ++round) {
            const uint32_t g = g0 + w;
            float acc = 0.f;
            if (g < n_groups) acc = group_sum(a, lo + g * kMixGroup, min(lo + (g + 1u) * kMixGroup, hi), t0, t, valid);
            // (round r + 2 writes this buffer again behind the barrier of round r + 1, which wave 0 reaches after these reads)
            part[round & 1u][w][lane] = acc;
            __syncthreads();
            if (w == 0u)
                for (uint32_t j = 0; j < WAVES && g0 + j < n_groups; ++j) sample = __fadd_rn(sample, part[round & 1u][j][lane]);
        }
    }
    if (w == 0u && valid) a.out[static_cast<size_t>(bus) * a.n_frames + t] = sample;
}

}  // namespace

hipError_t launch_mix(const MixArgs& a, uint32_t max_entries, hipStream_t q)
{
    if (a.n_buses == 0 || a.n_frames == 0) return hipSuccess;
    const dim3 grid((a.n_frames + 63u) / 64u, a.n_buses);
    if (max_entries <= kMixGroup) k_mix<1><<<grid, 64, 0, q>>>(a);
    else if (max_entries <= 4u * kMixGroup) k_mix<4><<<grid, 256, 0, q>>>(a);
    else k_mix<16><<<grid, 1024, 0, q>>>(a);
    return hipGetLastError();
}

}  // namespace aidax
