// aidax_meter.hip — the per-stream level meters of a pool (include/aidax.h, "Stream meters"): k_meter.
//
// One launch reads a pass's block, [n_active][n_frames] floats, and folds every row into its stream's 64-byte record: the largest |x| and
// the fp64 sum of x * x over the finite samples, and the counts of non-finite samples and (output side) of finite samples beyond 1.0.
// A pool issues it twice per metered pass on the pass's stream: over the block the pass was handed, ahead of the model's launch (the pass
// may work in place), and over the block it returns, behind the last stage.
//
// One 64-lane wave per stream, four to a workgroup. The lanes stride the row in 16-byte loads from the first 16-byte boundary of the row
// on (rows lie n_frames floats apart: at an odd block length most rows start off one) and take the floats before that boundary and
// behind the last whole quad one by one. Every lane keeps a maximum, a sum and two counts; a butterfly of shuffles folds the wave, and
// lane 0 reads, updates and writes the record. One wave owns a stream and passes are stream-ordered: no LDS, no barrier, no atomic.
// Each square is formed in fp64 from the fp32 sample (exact: 48 significant bits), so the sum's only error is that of its additions,
// all of non-negative terms, in an order the row's alignment and the butterfly fix.
#include <hip/hip_runtime.h>
#include <cstdint>
#include "aidax_kernels.h"

namespace aidax {

namespace {

constexpr uint32_t kMeterWaves = 4;            // streams of a workgroup

// what a lane has seen of its row
struct Fold {
    float peak;
    double energy;
    uint32_t nonfinite, over;
};
__device__ __forceinline__ void take(Fold& f, float x)
{
    const float a = __builtin_fabsf(x);
    const bool finite = a < __builtin_inff();                             // (false for a NaN)
    const double d = finite ? static_cast<double>(x) : 0.0;
    f.peak = finite && a > f.peak ? a : f.peak;
    f.energy += d * d;
    f.over += finite && a > 1.0f ? 1u : 0u;
    f.nonfinite += finite ? 0u : 1u;
}

__global__ __launch_bounds__(64 * kMeterWaves) void k_meter(const float* buf, MeterRec* rec, uint32_t n_active, uint32_t n_frames, int side)
{
    const uint32_t lane = threadIdx.x & 63u, s = blockIdx.x * kMeterWaves + (threadIdx.x >> 6);
    if (s >= n_active) return;                                            // (the whole wave)
    const float* row = buf + static_cast<size_t>(s) * n_frames;

    Fold f{0.f, 0.0, 0u, 0u};
    // floats in front of the row's first 16-byte boundary (at most three), the whole quads behind it, the floats behind the last quad
    const uint32_t off = static_cast<uint32_t>(reinterpret_cast<uintptr_t>(row) >> 2) & 3u;
    const uint32_t head = min(n_frames, (4u - off) & 3u);
    const uint32_t n_quads = (n_frames - head) >> 2;
    const uint32_t tail = head + 4u * n_quads;
    if (lane < head) take(f, row[lane]);
    const float4* quads = reinterpret_cast<const float4*>(row + head);
    for (uint32_t i = lane; i < n_quads; i += 64u) {
        const float4 q = quads[i];
        take(f, q.x); take(f, q.y); take(f, q.z); take(f, q.w);
    }
    if (tail + lane < n_frames) take(f, row[tail + lane]);

    float peak = f.peak;
    double energy = f.energy;
    uint32_t nonfinite = f.nonfinite, over = f.over;
    for (int d = 32; d > 0; d >>= 1) {
        const float p = __shfl_xor(peak, d, 64);
        peak = p > peak ? p : peak;
        energy += __shfl_xor(energy, d, 64);
        nonfinite += __shfl_xor(nonfinite, d, 64);
        over += __shfl_xor(over, d, 64);
    }
    if (lane != 0) return;
    MeterRec& r = rec[s];
    if (side == kMeterIn) {
        r.in_nonfinite += nonfinite;
        r.in_energy += energy;
        r.in_peak = peak > r.in_peak ? peak : r.in_peak;
    } else {
        r.frames += n_frames;
        r.passes += 1u;
        r.out_nonfinite += nonfinite;
        r.out_over += over;
        r.out_energy += energy;
        r.out_peak = peak > r.out_peak ? peak : r.out_peak;
    }
}

}  // namespace

hipError_t launch_meter(const float* buf, MeterRec* rec, uint32_t n_active, uint32_t n_frames, int side, hipStream_t q)
{
    if (n_active == 0 || n_frames == 0) return hipSuccess;
    k_meter<<<(n_active + kMeterWaves - 1u) / kMeterWaves, 64 * kMeterWaves, 0, q>>>(buf, rec, n_active, n_frames, side);
    return hipGetLastError();
}

}  // namespace aidax
