// aidax_bus_limit.hip — the look-ahead limiter and the meter of every mix bus (include/aidax.h, "Bus limiters"): k_bus_limit.
//
// One launch reads the raw bus block k_mix wrote, [n_buses][n_frames], and writes the pool's bus block of the same shape. Per bus, with
// its record (C, L, H, on), U = 2^22, W = L + 1 + H and x the sanitised samples (NaN and +-Inf are +0.0f) of all absolute frames:
//     q[j] = U where |x[j]| <= C, else floor(((double)C / (double)|x[j]|) * 2^22)
//     h[m] = min q[m - W + 1 .. m]          s[n] = h[n - L + 1] + .. + h[n]
//     g[n] = (float)((double)s[n] / (double)(L U))          out[n] = x[n - L] * g[n]
// Integer minima, an integer sum of at most 2^31, one fp64 division and one fp32 product: no order of evaluation changes a bit, so the
// kernel is free in how it forms them. A bus whose limiter is off gets its raw bits, undelayed; its history is kept all the same.
//
// One workgroup of 256 threads per bus, looping over tiles of 256 frames. The past comes from the bus's ring row of sanitised samples
// (frame k in slot k & mask; the launch appends the pass's frames, and no slot it writes holds a frame the pass still reads: the row
// is at least 2 L + H - 1 + max_frames long). In LDS, all indexed by absolute frame modulo their power-of-two size:
//   q    8192 entries: at the pass's start the 2 L + H - 1 frames of history are converted, then every tile converts only its own frames;
//   bm   the minima of the aligned blocks of 64 q, four lanes per block, formed when a block's last frame arrives;
//   h    1024 entries: the first tile forms the L - 1 values behind the pass's start too, every later one only its own.
// A window minimum is the entries up to the first block boundary, whole blocks out of bm, and the entries behind the last boundary (at
// most 63 + 72 + 63 reads, neighbouring lanes on neighbouring banks or on one address, sixteen of a lane's in flight); a box sum is L
// reads of h. The meter folds in registers, meets in LDS, and thread 0 reads, updates and writes the bus's record: passes are
// stream-ordered and one workgroup owns a bus, so there is no atomic. No scratch, no order that depends on the data, and every LDS and
// ring index is masked.
#include <hip/hip_runtime.h>
#include <cstdint>
#include "aidax_kernels.h"

namespace aidax {

namespace {

constexpr uint32_t kLimTile = 256;             // threads of a workgroup, frames of a tile
constexpr uint32_t kLimQ = 8192;               // q entries in LDS (>= 256 + 2 * 512 + 4096 - 1)
constexpr uint32_t kLimH = 1024;               // h entries in LDS (>= 256 + 512 - 1)
constexpr uint32_t kLimBlock = 64;             // q entries of one block minimum
static_assert(kLimQ >= kLimTile + 2u * kLimitMaxLookahead + kLimitMaxHold && kLimH >= kLimTile + kLimitMaxLookahead, "the windows fit their LDS rings");

__device__ __forceinline__ bool is_finite(float x) { return __builtin_fabsf(x) < __builtin_inff(); }      // (false for a NaN)

// q of a sanitised sample. Without a branch: at or below the ceiling the quotient is C / C, exactly 1, and q is U as the rule says;
// beyond it the quotient lies below 1 and the cast is the floor.
__device__ __forceinline__ uint32_t gain_position(float xs, float ceiling)
{
    const float a = __builtin_fmaxf(__builtin_fabsf(xs), ceiling);
    return static_cast<uint32_t>((static_cast<double>(ceiling) / static_cast<double>(a)) * 4194304.0);
}

// The minimum and the sum of `count` consecutive entries of an LDS ring from `start` on, sixteen reads in flight at a time: the reads of a
// batch do not wait for one another (a lane's run is a chain of LDS latencies otherwise), and those behind the run's end are masked
// into the ring like every other one and left out.
constexpr uint32_t kLimBatch = 16;
__device__ __forceinline__ uint32_t run_min(const uint32_t* ring, uint32_t mask, uint32_t start, uint32_t count)
{
    uint32_t r = kLimitUnit;
    for (uint32_t j = 0; j < count; j += kLimBatch) {
        uint32_t v[kLimBatch];
#pragma unroll
        for (uint32_t k = 0; k < kLimBatch; ++k) v[k] = ring[(start + j + k) & mask];
#pragma unroll
        for (uint32_t k = 0; k < kLimBatch; ++k) r = j + k < count ? min(r, v[k]) : r;
    }
    return r;
}
__device__ __forceinline__ uint32_t run_sum(const uint32_t* ring, uint32_t mask, uint32_t start, uint32_t count)
{
    uint32_t s = 0u;
    for (uint32_t j = 0; j < count; j += kLimBatch) {
        uint32_t v[kLimBatch];
#pragma unroll
        for (uint32_t k = 0; k < kLimBatch; ++k) v[k] = ring[(start + j + k) & mask];
#pragma unroll
        for (uint32_t k = 0; k < kLimBatch; ++k) s += j + k < count ? v[k] : 0u;
    }
    return s;
}

// The minima of the `count` whole blocks from absolute frame `first` (a multiple of 64) on, 64 blocks per round: four lanes per block,
// sixteen entries each, all sixteen reads in flight; a lane starts its sixteen at an offset of its block's number, so that the lanes of a
// half-wave (eight blocks, four quarters) touch 32 different banks at every read. Two shuffles fold the four quarters.
__device__ __forceinline__ void block_minima(const uint32_t* q, uint32_t* bm, uint32_t first, uint32_t count, uint32_t tid)
{
    for (uint32_t base = 0; base < count; base += kLimTile / 4u) {
        const uint32_t b = base + tid / 4u, part = tid & 3u, f0 = first + b * kLimBlock;
        uint32_t v[16];
#pragma unroll
        for (uint32_t k = 0; k < 16u; ++k) v[k] = q[(f0 + part * 16u + ((k + b) & 15u)) & (kLimQ - 1u)];      // (a block behind the last one: masked, left out below)
        uint32_t r = v[0];
#pragma unroll
        for (uint32_t k = 1; k < 16u; ++k) r = min(r, v[k]);
        r = min(r, static_cast<uint32_t>(__shfl_xor(static_cast<int>(r), 1, 64)));
        r = min(r, static_cast<uint32_t>(__shfl_xor(static_cast<int>(r), 2, 64)));
        if (part == 0u && b < count) bm[(f0 / kLimBlock) & (kLimQ / kLimBlock - 1u)] = r;
    }
}

// min q[m - W + 1 .. m]
__device__ __forceinline__ uint32_t window_min(const uint32_t* q, const uint32_t* bm, uint32_t m, uint32_t W)
{
    const uint32_t f = m - W + 1u;
    const uint32_t head = min(W, (kLimBlock - (f & (kLimBlock - 1u))) & (kLimBlock - 1u));
    const uint32_t blocks = (W - head) / kLimBlock, tail = (W - head) % kLimBlock;
    uint32_t r = run_min(q, kLimQ - 1u, f, head);
    r = min(r, run_min(bm, kLimQ / kLimBlock - 1u, (f + head) / kLimBlock, blocks));
    return min(r, run_min(q, kLimQ - 1u, f + head + blocks * kLimBlock, tail));
}

__global__ __launch_bounds__(kLimTile) void k_bus_limit(BusLimitArgs a)
{
    __shared__ uint32_t q[kLimQ];
    __shared__ uint32_t bm[kLimQ / kLimBlock];
    __shared__ uint32_t h[kLimH];
    __shared__ uint32_t fold_u[2][kLimTile / 64u];
    __shared__ float fold_f[3][kLimTile / 64u];

    const uint32_t tid = threadIdx.x, lane = tid & 63u, bus = blockIdx.x;
    const uint32_t wave = static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(static_cast<int>(tid >> 6)));
    const LimitRec r = a.rec[bus];
    const float* raw = a.raw + static_cast<size_t>(bus) * a.n_frames;
    float* out = a.out + static_cast<size_t>(bus) * a.n_frames;
    float* ring = a.ring + static_cast<size_t>(bus) * (static_cast<size_t>(a.mask) + 1u);
    // (the host admits no record beyond these bounds; held to them here as well, they bound every loop and window below)
    const uint32_t L = min(max(r.lookahead, 1u), kLimitMaxLookahead), H = min(r.hold, kLimitMaxHold), W = L + 1u + H;
    const float C = r.ceiling;
    const bool on = r.on != 0u;                                            // (the whole workgroup's: one bus)

    uint32_t nonfinite = 0u, limited = 0u;
    float in_peak = 0.f, out_peak = 0.f, min_gain = 1.f;

    if (on) {
        const uint32_t reach = 2u * L + H - 1u, first = a.pos - reach;    // the history a pass needs: frames first .. pos - 1
        for (uint32_t base = tid; base < reach; base += kLimTile * kLimBatch) {      // (sixteen of a lane's loads in flight, like the LDS runs)
            float v[kLimBatch];
#pragma unroll
            for (uint32_t k = 0; k < kLimBatch; ++k) v[k] = ring[(first + min(base + k * kLimTile, reach - 1u)) & a.mask];
#pragma unroll
            for (uint32_t k = 0; k < kLimBatch; ++k)
                if (base + k * kLimTile < reach) q[(first + base + k * kLimTile) & (kLimQ - 1u)] = gain_position(v[k], C);
        }
        __syncthreads();
        const uint32_t lead = (kLimBlock - (first & (kLimBlock - 1u))) & (kLimBlock - 1u);      // frames ahead of the history's first block boundary
        if (reach >= lead) block_minima(q, bm, first + lead, (reach - lead) / kLimBlock, tid);
    }

    for (uint32_t t0 = 0; t0 < a.n_frames; t0 += kLimTile) {
        const uint32_t n = min(kLimTile, a.n_frames - t0), a0 = a.pos + t0;
        // the tile's own frames: sanitised into the ring, their gain positions into q
        if (tid < n) {
            const float x = raw[t0 + tid];
            const bool finite = is_finite(x);
            const float xs = finite ? x : 0.f;
            nonfinite += finite ? 0u : 1u;
            in_peak = __builtin_fmaxf(in_peak, __builtin_fabsf(xs));
            ring[(a0 + tid) & a.mask] = xs;
            if (on) q[(a0 + tid) & (kLimQ - 1u)] = gain_position(xs, C);
            else out[t0 + tid] = x;
        }
        if (!on) continue;
        __syncthreads();
        // the blocks whose last frame lies in this tile
        const uint32_t d0 = (kLimBlock - 1u - a0) & (kLimBlock - 1u);     // the first frame of the tile that ends a block
        if (d0 < n) block_minima(q, bm, a0 + d0 - (kLimBlock - 1u), (n - 1u - d0) / kLimBlock + 1u, tid);
        __syncthreads();
        // h of the tile's frames, and behind the pass's first frame the L - 1 values its box sums reach back to
        const uint32_t back = t0 == 0u ? L - 1u : 0u;
        for (uint32_t i = tid; i < n + back; i += kLimTile) {
            const uint32_t m = a0 - back + i;
            h[m & (kLimH - 1u)] = window_min(q, bm, m, W);
        }
        __syncthreads();
        if (tid < n) {
            const uint32_t f = a0 + tid, t = t0 + tid;
            const uint32_t s = run_sum(h, kLimH - 1u, f - L + 1u, L);
            const uint32_t full = L * kLimitUnit;                          // (<= 2^31)
            const float g = static_cast<float>(static_cast<double>(s) / static_cast<double>(full));
            float xd;
            if (t >= L) {                                                  // the delayed sample: of this pass, or out of the ring
                const float x = raw[t - L];
                xd = is_finite(x) ? x : 0.f;
            } else {
                xd = ring[(f - L) & a.mask];
            }
            const float y = __fmul_rn(xd, g);
            out[t] = y;
            out_peak = __builtin_fmaxf(out_peak, __builtin_fabsf(y));
            limited += s < full ? 1u : 0u;
            min_gain = __builtin_fminf(min_gain, g);
        }
    }

    // the meter: a butterfly per wave, the four waves through LDS, one read-modify-write
    if (!on) out_peak = in_peak;
    for (int d = 32; d > 0; d >>= 1) {
        nonfinite += __shfl_xor(nonfinite, d, 64);
        limited += __shfl_xor(limited, d, 64);
        in_peak = __builtin_fmaxf(in_peak, __shfl_xor(in_peak, d, 64));
        out_peak = __builtin_fmaxf(out_peak, __shfl_xor(out_peak, d, 64));
        min_gain = __builtin_fminf(min_gain, __shfl_xor(min_gain, d, 64));
    }
    if (lane == 0u) {
        fold_u[0][wave] = nonfinite; fold_u[1][wave] = limited;
        fold_f[0][wave] = in_peak; fold_f[1][wave] = out_peak; fold_f[2][wave] = min_gain;
    }
    __syncthreads();
    if (tid != 0u) return;
    for (uint32_t w = 1; w < kLimTile / 64u; ++w) {
        nonfinite += fold_u[0][w]; limited += fold_u[1][w];
        in_peak = __builtin_fmaxf(in_peak, fold_f[0][w]);
        out_peak = __builtin_fmaxf(out_peak, fold_f[1][w]);
        min_gain = __builtin_fminf(min_gain, fold_f[2][w]);
    }
    BusMeterRec& m = a.meter[bus];
    m.frames += a.n_frames;
    m.passes += 1u;
    m.in_nonfinite += nonfinite;
    m.in_peak = __builtin_fmaxf(m.in_peak, in_peak);
    m.out_peak = __builtin_fmaxf(m.out_peak, out_peak);
    if (on) {
        m.limited += limited;
        m.min_gain = __builtin_fminf(m.min_gain, min_gain);
    }
}

}  // namespace

hipError_t launch_bus_limit(const BusLimitArgs& a, hipStream_t q)
{
    if (a.n_buses == 0 || a.n_frames == 0) return hipSuccess;
    k_bus_limit<<<a.n_buses, kLimTile, 0, q>>>(a);
    return hipGetLastError();
}

}  // namespace aidax
