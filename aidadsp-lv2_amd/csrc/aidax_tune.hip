// aidax_tune.hip — the per-stream tuners of a pool (include/aidax.h, "Stream tuners"): k_tune.
//
// One launch goes ahead of the model's launch of a pass, a workgroup of four waves per stream of the pass. It appends the stream's row
// of the block the pass was handed to the stream's history ring (frame p of the tuner's count in slot p & mask) and moves the count;
// where the count crosses a hop boundary b (the device decides from its own count, by rule 1 of the header) it analyses the W frames
// that end at b: the McLeod pitch method, a normalised autocorrelation.
//
// The autocorrelation r[t] = sum_j x[j] x[j + t] is a Toeplitz x Hankel tile product on the matrix cores, both operands the stream's
// own window. Per K step of 32 frames at j0 and per lag tile of 256:
//     A[i][k] = x[j0 + k - i]                  (16 x 32: depends on the step alone, one fragment serves every tile)
//     B[k][nn] = x[j0 + k + 16 nn + 256 tile]  (32 x 16)
//     C[i][nn] += A B                          accumulates lag i + 16 nn + 256 tile
// A pair (x[a], x[a + t]) meets in exactly one step (j0 + k = a + i), and only steps with j0 + 256 tile < W reach into the window, so
// W / 32 steps cover the sum; reads below 0 and at or above W are zeros. Both operands are split exactly into three bf16 terms
// (x = x0 + x1 + x2) and six of the nine term products go out on v_mfma_f32_16x16x32_bf16, the project's fp32-parity idiom
// (aidax_ir_mfma.hip). The window is split ONCE, into LDS: per term a plane of W + 264 bf16 with 16 zeros in front and 248 behind (the
// B fragments are 16-byte loads: a lane's eight frames start at a multiple of 8), and a second copy of it one element later, because a
// lane's eight A frames start at j0 + 8 g - i, odd for odd i: the lane reads the copy in which its start is an even position, as four
// aligned dwords. Wave w takes the steps w, w + 4, .. of every tile; the four partial sums are added in wave order: no atomics, the
// same bits on every run.
//
// m[t] comes from the fp64 prefix sums of x^2 (a chunk per thread, a shuffle scan per wave, the waves' totals in order), the NSDF row
// goes to LDS and to the stream's curve row, and wave 0 picks the peak: an inclusive segmented maximum over the lobes (the runs of
// lags with n > 0), 64 lags per chunk with a carry as k_gate carries its maps, once for the largest key maximum and once more for the
// first one at or above k times it. Every lane then holds the chosen lag; lane 0 interpolates in fp64 and writes the reading.
#include <hip/hip_runtime.h>
#include <cstdint>
#include "aidax_kernels.h"

namespace aidax {

namespace {

typedef float tn_f32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 tn_bf16x8 __attribute__((ext_vector_type(8)));
typedef unsigned tn_u32x4 __attribute__((ext_vector_type(4)));

constexpr uint32_t kTuneThreads = 256, kTuneMaxWindow = 4096;
constexpr uint32_t kTunePadLo = 16, kTunePads = 264;     // zeros in front of a plane's frame 0, and in front and behind together

// LDS: six planes (term x copy), then the prefix sums the normalisation reads — c[0 .. tmax + 1] and c[W - tmax - 1 .. W], 2 (tmax + 2)
// doubles — and the waves' totals. Behind the autocorrelation the planes' room is used again: the waves' partial sums, [4][tiles][256]
// floats, and behind them the NSDF row (10 W + 4100 bytes at most, of 12 W + 3168). The default design (W = 2048, lags to 687) takes
// 38784 bytes: four workgroups to a CU.
__host__ __device__ constexpr uint32_t tune_plane(uint32_t W) { return W + kTunePads; }
__host__ __device__ constexpr uint32_t tune_off_cs(uint32_t W) { return 12u * tune_plane(W); }
__host__ __device__ constexpr uint32_t tune_off_wt(uint32_t W, uint32_t tmax) { return tune_off_cs(W) + 16u * (tmax + 2u); }
__host__ __device__ constexpr uint32_t tune_lds(uint32_t W, uint32_t tmax) { return tune_off_wt(W, tmax) + 32u; }

__device__ __forceinline__ unsigned short tune_bf16(float x) { return __builtin_bit_cast(unsigned short, static_cast<__bf16>(x)); }
__device__ __forceinline__ float tune_bf16_value(unsigned short h) { return __builtin_bit_cast(float, static_cast<unsigned>(h) << 16); }

// One element of the segmented maximum: f = a lag that is not positive lies at or ahead of this one in the scanned range (what came
// before the range does not reach it), (v, l) = the best candidate since, v < 0: none
struct TuneEl {
    uint32_t f;
    float v;
    uint32_t l;
};
__device__ __forceinline__ TuneEl tune_then(const TuneEl& lo, const TuneEl& hi)      // the lower lags first
{
    if (hi.f) return hi;
    const bool better = hi.v > lo.v;                                      // (a tie keeps the earlier lag)
    return { lo.f, better ? hi.v : lo.v, better ? hi.l : lo.l };
}

// The element of the lane a DPP control names, the identity (f = 0, no candidate) where it names none (a shift past the row's start, a
// row the mask leaves out)
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ uint32_t tune_dpp(uint32_t idle, uint32_t v)
{
    return static_cast<uint32_t>(__builtin_amdgcn_update_dpp(static_cast<int>(idle), static_cast<int>(v), CTRL, ROW_MASK, 0xf, false));
}
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ TuneEl tune_lower(const TuneEl& e)
{
    return { tune_dpp<CTRL, ROW_MASK>(0u, e.f), __builtin_bit_cast(float, tune_dpp<CTRL, ROW_MASK>(0xbf800000u, __builtin_bit_cast(uint32_t, e.v))),
             tune_dpp<CTRL, ROW_MASK>(0u, e.l) };
}

// What the pick needs of the design
struct TunePick {
    const float* nsdf;
    uint32_t tmin, tmax, t_start;
};
// Lags base .. base + 63, one per lane: the inclusive segmented maximum with `carry` folded in (and carried on), and whether this
// lane's lag ends a lobe that has a key maximum (then e holds it)
__device__ __forceinline__ bool tune_chunk(const TunePick& k, uint32_t base, uint32_t lane, TuneEl& carry, TuneEl& e)
{
    const uint32_t t = base + lane, last = k.tmax + 1u;
    const bool in = t >= 1u && t <= last;
    const float n0 = in ? k.nsdf[t] : 0.f, nm1 = in ? k.nsdf[t - 1u] : 0.f, np1 = in && t < last ? k.nsdf[t + 1u] : 0.f;
    const bool p = in && n0 > 0.f;
    const bool cand = p && t > k.t_start && t >= k.tmin && t <= k.tmax && n0 >= nm1 && n0 > np1;
    e = { p ? 0u : 1u, cand ? n0 : -1.f, t };
    // the inclusive scan on the DPP network, as k_gate scans its maps: recursive doubling inside every row of 16 lanes (row_shr 1, 2,
    // 4, 8), then the total of row 0 into row 1 and of row 2 into row 3 (row_bcast:15), then that of rows 0 and 1 into rows 2 and 3
    // (row_bcast:31); a lane without a lower partner takes the identity
    e = tune_then(tune_lower<0x111, 0xf>(e), e);
    e = tune_then(tune_lower<0x112, 0xf>(e), e);
    e = tune_then(tune_lower<0x114, 0xf>(e), e);
    e = tune_then(tune_lower<0x118, 0xf>(e), e);
    e = tune_then(tune_lower<0x142, 0xa>(e), e);
    e = tune_then(tune_lower<0x143, 0xc>(e), e);
    e = tune_then(carry, e);
    carry.f = static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(e.f), 63));
    carry.v = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, e.v), 63));
    carry.l = static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(e.l), 63));
    return p && t > k.t_start && !(np1 > 0.f) && e.v > 0.f;
}

__device__ __forceinline__ void tune_analyse(const TuneArgs& a, uint32_t s, const float* ring, uint64_t b)
{
#pragma clang fp contract(off)
    extern __shared__ __attribute__((aligned(16))) unsigned char tune_smem[];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t W = a.window, PL = tune_plane(W), tmax = a.tmax, n_lags = tmax + 2u;
    unsigned short* planes = reinterpret_cast<unsigned short*>(tune_smem);              // [term][copy][PL]
    const uint32_t n_tiles = (tmax + 1u) / 256u + 1u;
    double* cs = reinterpret_cast<double*>(tune_smem + tune_off_cs(W));                 // c[t] at t, c[W - t] at 2 tmax + 3 - t
    double* wt = reinterpret_cast<double*>(tune_smem + tune_off_wt(W, tmax));
    float* part = reinterpret_cast<float*>(tune_smem);                                  // (behind the autocorrelation)
    float* nsdf = part + 4u * n_tiles * 256u;

    // the window, oldest frame first: a thread's frames tid, tid + 256, .. are all asked for before the first one is used (one trip
    // to memory, not W / 256 of them one behind the other)
    const uint32_t w0 = static_cast<uint32_t>(b - W);
    float xs[kTuneMaxWindow / kTuneThreads];
#pragma unroll
    for (uint32_t i = 0; i < kTuneMaxWindow / kTuneThreads; ++i) {
        const uint32_t j = tid + i * kTuneThreads;
        xs[i] = j < W ? ring[(w0 + j) & a.mask] : 0.f;
    }
    // the planes' zeros: positions [0, 16 + copy) and [W + 16 + copy, PL) of copy 0 / 1, 264 of each plane
    for (uint32_t i = tid; i < 6u * kTunePads; i += kTuneThreads) {
        const uint32_t pl = i / kTunePads, k = i - pl * kTunePads, copy = pl & 1u;
        planes[pl * PL + (k < kTunePadLo + copy ? k : W + k)] = 0;
    }
    // the frames' terms into both copies
#pragma unroll
    for (uint32_t i = 0; i < kTuneMaxWindow / kTuneThreads; ++i) {
        const uint32_t j = tid + i * kTuneThreads;
        if (j >= W) break;
        const float x = xs[i];
        float r = x;
#pragma unroll
        for (uint32_t term = 0; term < 3u; ++term) {
            const unsigned short h = tune_bf16(r);
            planes[(2u * term) * PL + kTunePadLo + j] = h;
            planes[(2u * term + 1u) * PL + kTunePadLo + 1u + j] = h;
            r -= tune_bf16_value(h);
        }
    }
    if (tid == 0) cs[0] = 0.0;
    __syncthreads();

    // c[1 + j] = sum of the squares up to frame j: a chunk of W / 256 frames per thread (read back from the planes: t0 + (t1 + t2) is
    // the frame, exactly), the threads of a wave by shuffles, the waves in order; only the sums the normalisation reads are kept
    {
        const uint32_t ch = W / kTuneThreads, j_first = tid * ch;
        double loc[kTuneMaxWindow / kTuneThreads];
        double run = 0.0;
#pragma unroll
        for (uint32_t i = 0; i < kTuneMaxWindow / kTuneThreads; ++i) {
            if (i >= ch) break;
            const uint32_t at = kTunePadLo + j_first + i;
            const float x = tune_bf16_value(planes[at]) + (tune_bf16_value(planes[2u * PL + at]) + tune_bf16_value(planes[4u * PL + at]));
            run += static_cast<double>(x) * static_cast<double>(x);
            loc[i] = run;
        }
        double inc = run;
        for (uint32_t d = 1; d < 64u; d <<= 1) {
            const double o = __shfl_up(inc, d, 64);
            if (lane >= d) inc = o + inc;
        }
        if (lane == 63u) wt[wave] = inc;
        double excl = __shfl_up(inc, 1, 64);
        if (lane == 0) excl = 0.0;
        __syncthreads();
        double off = 0.0;
        for (uint32_t w = 0; w < wave; ++w) off += wt[w];
        off += excl;
#pragma unroll
        for (uint32_t i = 0; i < kTuneMaxWindow / kTuneThreads; ++i) {
            if (i >= ch) break;
            const uint32_t at = j_first + i + 1u;                         // c's index
            const double v = off + loc[i];
            if (at <= tmax + 1u) cs[at] = v;
            if (at + tmax + 1u >= W) cs[tmax + 2u + (at + tmax + 1u - W)] = v;
        }
    }

    // the autocorrelation: this wave's steps of every lag tile
    const uint32_t nl = lane & 15u, g = lane >> 4, copy = nl & 1u;
    tn_f32x4 acc[kTuneMaxTiles];
#pragma unroll
    for (uint32_t tile = 0; tile < kTuneMaxTiles; ++tile) acc[tile] = tn_f32x4{ 0.f, 0.f, 0.f, 0.f };
    for (uint32_t j0 = 32u * wave; j0 < W; j0 += 128u) {
        // frames j0 + 8 g - nl .. + 7: an even position of the lane's copy
        const uint32_t pa = j0 + 8u * g + kTunePadLo + copy - nl;
        tn_u32x4 af[3];
#pragma unroll
        for (uint32_t term = 0; term < 3u; ++term) {
            const uint32_t* q = reinterpret_cast<const uint32_t*>(planes + (2u * term + copy) * PL + pa);
            af[term] = tn_u32x4{ q[0], q[1], q[2], q[3] };
        }
        // Three tiles at a time, their products interleaved: a tile's six MFMAs are a dependent chain on its accumulator, and three
        // chains side by side keep the matrix core issuing. A tile of the group that is past the design's lags, or whose step is past
        // the window (j0 + 256 tile >= W), reads eight of the plane's trailing zeros instead and adds nothing (a window that holds a
        // NaN or an Inf has no finite lag anyway: every r[t] up to W / 2 takes a product with it).
#pragma unroll
        for (uint32_t grp = 0; grp < kTuneMaxTiles / 3u; ++grp) {
            if (3u * grp >= n_tiles || j0 + 768u * grp >= W) continue;    // (wave-uniform)
            tn_u32x4 bt[3][3];
#pragma unroll
            for (uint32_t u = 0; u < 3u; ++u) {
                const uint32_t tile = 3u * grp + u;
                const bool live = tile < n_tiles && j0 + 256u * tile < W;
                const uint32_t pb = live ? j0 + 8u * g + 16u * nl + 256u * tile + kTunePadLo : W + kTunePadLo + 8u;
#pragma unroll
                for (uint32_t term = 0; term < 3u; ++term) bt[u][term] = *reinterpret_cast<const tn_u32x4*>(planes + (2u * term) * PL + pb);
            }
            // (a0 a1 a2) b0 | (a0 a1) b1 | a0 b2: the six term products, the large ones first
#pragma unroll
            for (uint32_t th = 0; th < 3u; ++th)
#pragma unroll
                for (uint32_t tw = 0; tw < 3u - th; ++tw)
#pragma unroll
                    for (uint32_t u = 0; u < 3u; ++u)
                        acc[3u * grp + u] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(tn_bf16x8, af[tw]), __builtin_bit_cast(tn_bf16x8, bt[u][th]), acc[3u * grp + u], 0, 0, 0);
        }
    }
    __syncthreads();                                                      // (every wave has read its last fragment, the prefix sums are whole)

    // the waves' partial sums over the planes: [wave][tile][256 lags]; a lane holds lags 4 g .. 4 g + 3 (+ 16 nl) of every tile
#pragma unroll
    for (uint32_t tile = 0; tile < kTuneMaxTiles; ++tile) {
        if (tile >= n_tiles) continue;
        float* dst = part + (wave * n_tiles + tile) * 256u + 16u * nl + 4u * g;
        dst[0] = acc[tile].x; dst[1] = acc[tile].y; dst[2] = acc[tile].z; dst[3] = acc[tile].w;
    }
    __syncthreads();

    const double cW = cs[2u * tmax + 3u];
    float* curve = a.curve + static_cast<size_t>(s) * a.curve_row;
    for (uint32_t t = tid; t < n_lags; t += kTuneThreads) {
        const uint32_t at = (t >> 8) * 256u + (t & 255u), step = n_tiles * 256u;
        float r = part[at];
        r += part[at + step];
        r += part[at + 2u * step];
        r += part[at + 3u * step];
        const double m = cs[2u * tmax + 3u - t] + (cW - cs[t]);
        const float n = m <= 0.0 ? 0.f : static_cast<float>((2.0 * static_cast<double>(r)) / m);
        nsdf[t] = n;
        curve[t] = n;
    }
    __syncthreads();
    if (wave != 0) return;

    // the first lag from 1 on that is not positive: the end of the lobe around lag 0 (0: the whole row is one lobe, no key maximum)
    TunePick k{ nsdf, a.tmin, tmax, 0u };
    for (uint32_t base = 0; base < n_lags && k.t_start == 0u; base += 64u) {
        const uint32_t t = base + lane;
        const bool z = t >= 1u && t <= tmax + 1u && !(nsdf[t] > 0.f);
        const unsigned long long found = __ballot(z);
        if (found) k.t_start = base + static_cast<uint32_t>(__builtin_ctzll(found));
    }
    float nmax = -1.f;
    uint32_t q = 0;
    if (k.t_start != 0u) {
        TuneEl carry{ 1u, -1.f, 0u }, e;
        for (uint32_t base = 0; base < n_lags; base += 64u) {
            const bool key = tune_chunk(k, base, lane, carry, e);
            nmax = key && e.v > nmax ? e.v : nmax;                        // (per lane; folded once behind the loop)
        }
        for (int d = 32; d > 0; d >>= 1) {
            const float o = __shfl_xor(nmax, d, 64);
            nmax = o > nmax ? o : nmax;
        }
        if (nmax > 0.f) {
            const float bar = __fmul_rn(a.threshold, nmax);
            carry = { 1u, -1.f, 0u };
            for (uint32_t base = 0; base < n_lags && q == 0u; base += 64u) {
                const bool key = tune_chunk(k, base, lane, carry, e);
                const unsigned long long hit = __ballot(key && e.v >= bar);
                if (hit) q = __shfl(e.l, static_cast<int>(__builtin_ctzll(hit)), 64);
            }
        }
    }
    if (lane != 0) return;

    const float level = static_cast<float>(sqrt(cW / static_cast<double>(W)));
    float hz = 0.f, period = 0.f, clarity = 0.f;
    if (q != 0u) {
        const double na = static_cast<double>(nsdf[q - 1u]), nb = static_cast<double>(nsdf[q]), nc = static_cast<double>(nsdf[q + 1u]);
        const double twice = 2.0 * nb;
        const double left = na - twice;
        const double den = left + nc;
        const double diff = na - nc;
        const double half = 0.5 * diff;
        const double d = den < 0.0 ? half / den : 0.0;
        const double pd = static_cast<double>(q) + d;
        const double quarter = 0.25 * diff;
        const double lift = quarter * d;
        const double cl = nb - lift;
        const double f = a.samplerate / pd;
        period = static_cast<float>(pd);
        clarity = static_cast<float>(cl);
        hz = static_cast<float>(f);
    }
    const bool voiced = q != 0u && !(clarity < a.clarity_min) && !(level < a.level_min);
    TunerReading& rd = a.reading[s];
    rd.frame = b;
    rd.analyses += 1u;
    rd.lag = voiced ? q : 0u;
    rd.hz = voiced ? hz : 0.f;
    rd.period = voiced ? period : 0.f;
    rd.clarity = clarity;
    rd.level = level;
}

template <bool ANALYSE>
__global__ __launch_bounds__(kTuneThreads) void k_tune(TuneArgs a)
{
    const uint32_t tid = threadIdx.x, s = blockIdx.x;
    if (s >= a.n_active || !a.on[s]) return;                              // (the whole workgroup)
    const uint64_t p0 = a.pos[s], p1 = p0 + a.n_frames;
    float* ring = a.ring + static_cast<size_t>(s) * (a.mask + 1u);
    const float* row = a.in + static_cast<size_t>(s) * a.n_frames;
    for (uint32_t t = tid; t < a.n_frames; t += kTuneThreads) ring[(static_cast<uint32_t>(p0) + t) & a.mask] = row[t];
    __syncthreads();                                                      // every thread has read the count; the workgroup sees the appended frames
    if (tid == 0) a.pos[s] = p1;
    if constexpr (ANALYSE) {
        const uint64_t b = (p1 / a.hop) * a.hop;
        if (b > p0 && b >= a.window) tune_analyse(a, s, ring, b);         // (workgroup-uniform)
    }
}

}  // namespace

size_t tune_lds_bytes(uint32_t window, uint32_t tmax) { return tune_lds(window, tmax); }

hipError_t launch_tune(const TuneArgs& a, bool analyse, hipStream_t q)
{
    if (a.n_active == 0 || a.n_frames == 0) return hipSuccess;
    if (!analyse) {
        hipLaunchKernelGGL(k_tune<false>, dim3(a.n_active), dim3(kTuneThreads), 0, q, a);
        return hipGetLastError();
    }
    const size_t lds = tune_lds(a.window, a.tmax);
    if (lds > 64 * 1024) {
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(k_tune<true>), hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(lds));
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(k_tune<true>, dim3(a.n_active), dim3(kTuneThreads), lds, q, a);
    return hipGetLastError();
}

}  // namespace aidax
