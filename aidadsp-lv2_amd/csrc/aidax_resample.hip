// aidax_resample.hip — the streaming polyphase resampler of the rate adapter (include/aidax.h, "Rate conversion"): k_resample.
//
//   out[s][j] = sum_{i = -H .. H} w_phi[i + H] * x[s][q - i]        a = (j - d_out) M - d_in L = q L + phi,  0 <= phi < L
//
// The work is tiny (about 36 MFLOP and 2 MB for 1024 streams x 256 frames at 160 / 147), so a call is ONE launch whatever the number of
// streams: workgroups over (output tile of kRsTile frames, stream), a thread per output. A workgroup stages its tile's input window
// x[q_first - H .. q_last + H] in LDS, out of the stream's history ring (frames of earlier calls) and the call's new block, and each
// thread walks its phase's row of the weight table. The table lies transposed in memory, [T][L]: at one tap the lanes of a wave, whose
// phases differ, read one row of L floats (a few cache lines, L2- and L1-resident: at most 172 KB for the audio rates) instead of 64 rows.
// The same launch appends the new block to the ring, each tile's workgroup a share of it; the host keeps the ring large enough that the
// slots written are never slots a window of this call reads (aidax_rate.cpp: the capacity check), so no order between workgroups matters.
//
// One summation order per output sample, whatever the tile, the block boundary or the cut of the input into calls: four fp32
// accumulators, tap ii of the row (ii = i + H, ascending) into accumulator ii mod 4 by FMA, then (acc0 + acc1) + (acc2 + acc3). Whether a
// frame comes from LDS, the ring or the new block does not touch its bits. Equal rates are a bit copy (x[q], no arithmetic).
// A ratio whose window would not fit kRsWindow floats reads its frames in place instead of staging them: the same sums in the same
// order. The window is ceil(255 M / L) + 2 ceil(32 M / L) + 1 floats, about 319 M / L: the in-place form starts at M / L of about 12.84
// (77 -> 6 fills the 4096 floats exactly and is still staged, 90 -> 7 is the first pair in place; of the audio pairs only those at
// 16 : 1 and beyond, such as 192000 -> 8000). AIDAX_RS_STAGED=0 (test build) forces the in-place form at any ratio.
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstdlib>
#include "aidax_kernels.h"

namespace aidax {

namespace {

constexpr uint32_t kRsThreads = kRsTile;       // one thread per output of a tile

template <bool STAGED>
__global__ __launch_bounds__(kRsThreads) void k_resample(ResampleArgs a)
{
    __shared__ float win[STAGED ? kRsWindow : 1];
    const uint32_t s = blockIdx.y, tile = blockIdx.x, tid = threadIdx.x;
    const float* in = a.in + static_cast<size_t>(s) * a.n_in;
    float* ring = a.ring + static_cast<size_t>(s) * (a.mask + 1u);

    // this workgroup's share of the append: new frame c into ring slot (pos + c) & mask
    const uint32_t share = (a.n_in + gridDim.x - 1u) / gridDim.x;
    const uint32_t c0 = tile * share, c1 = min(a.n_in, c0 + share);
    for (uint32_t c = c0 + tid; c < c1; c += kRsThreads) ring[(a.pos + c) & a.mask] = in[c];

    const uint32_t t0 = tile * kRsTile;
    if (t0 >= a.n_out) return;                                            // (the whole workgroup: a call without outputs)
    const uint32_t n_t = min(kRsTile, a.n_out - t0);
    // input frame k, counted from the call's first new frame: the new block, the ring, or zeros before the stream's history
    auto frame = [&](int32_t k) -> float {
        if (k >= 0) return in[k];
        if (k < -static_cast<int32_t>(a.n_hist)) return 0.f;
        return ring[(a.pos + static_cast<uint32_t>(k)) & a.mask];
    };
    const uint32_t u_first = a.phi0 + t0 * a.M, u_last = a.phi0 + (t0 + n_t - 1u) * a.M;
    const int32_t base = a.q0 + static_cast<int32_t>(u_first / a.L) - static_cast<int32_t>(a.H);
    if (STAGED) {
        const uint32_t wlen = u_last / a.L - u_first / a.L + 2u * a.H + 1u;
        for (uint32_t i = tid; i < wlen; i += kRsThreads) win[i] = frame(base + static_cast<int32_t>(i));
        __syncthreads();
    }
    if (tid >= n_t) return;
    const uint32_t u = a.phi0 + (t0 + tid) * a.M, phi = u % a.L;
    const uint32_t top = static_cast<uint32_t>(a.q0 + static_cast<int32_t>(u / a.L) + static_cast<int32_t>(a.H) - base);     // the window index of x[q + H]
    auto x = [&](uint32_t idx) -> float { return STAGED ? win[idx] : frame(base + static_cast<int32_t>(idx)); };
    float* out = a.out + static_cast<size_t>(s) * a.n_out + t0 + tid;
    if (a.copy) { *out = x(top - a.H); return; }
    const float* w = a.wt + phi;
    const uint32_t T = 2u * a.H + 1u, L = a.L;
    float acc0 = 0.f, acc1 = 0.f, acc2 = 0.f, acc3 = 0.f;
    uint32_t ii = 0;
    for (; ii + 4u <= T; ii += 4u) {
        acc0 = __builtin_fmaf(w[static_cast<size_t>(ii) * L], x(top - ii), acc0);
        acc1 = __builtin_fmaf(w[static_cast<size_t>(ii + 1u) * L], x(top - ii - 1u), acc1);
        acc2 = __builtin_fmaf(w[static_cast<size_t>(ii + 2u) * L], x(top - ii - 2u), acc2);
        acc3 = __builtin_fmaf(w[static_cast<size_t>(ii + 3u) * L], x(top - ii - 3u), acc3);
    }
    if (ii < T) acc0 = __builtin_fmaf(w[static_cast<size_t>(ii) * L], x(top - ii), acc0);
    if (ii + 1u < T) acc1 = __builtin_fmaf(w[static_cast<size_t>(ii + 1u) * L], x(top - ii - 1u), acc1);
    if (ii + 2u < T) acc2 = __builtin_fmaf(w[static_cast<size_t>(ii + 2u) * L], x(top - ii - 2u), acc2);
    *out = (acc0 + acc1) + (acc2 + acc3);
}

}  // namespace

uint32_t resample_window(uint32_t L, uint32_t M, uint32_t H) { return ((kRsTile - 1u) * M + L - 1u) / L + 2u * H + 1u; }

hipError_t launch_resample(const ResampleArgs& a, hipStream_t q)
{
    if (a.n_in == 0 && a.n_out == 0) return hipSuccess;
    const uint32_t tiles = a.n_out ? (a.n_out + kRsTile - 1u) / kRsTile : 1u;
    const dim3 grid(tiles, a.n_streams);
    // (read on every call: tests switch forms within one process)
    const bool in_place = [] { const char* e = AIDAX_HOOK_ENV("AIDAX_RS_STAGED"); return e && e[0] == '0'; }();
    if (!in_place && resample_window(a.L, a.M, a.H) <= kRsWindow) k_resample<true><<<grid, kRsThreads, 0, q>>>(a);
    else k_resample<false><<<grid, kRsThreads, 0, q>>>(a);
    return hipGetLastError();
}

}  // namespace aidax
