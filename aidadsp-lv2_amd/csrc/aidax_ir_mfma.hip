// aidax_ir_mfma.hip — the cabinet impulse-response stage: every stream's block convolved with its IR (the pool IR or a bank slot),
// causally and without latency, as a time-domain Toeplitz GEMM on the matrix cores (k_ir_conv), behind the whole run() of the pass.
//
//   y[s][t] = sum_{k < L} h[k] * x[s][t - k]        x = the dry signal (what the pool returns without an IR), L <= the pool's IR capacity (8192 .. 65536)
//
// Per block of n frames and a pool of N streams: M = the block's frames (tiles of 16), N = the streams (16 per MFMA), K = input frames
// (steps of 32). With the output tile at frame t0 and the input window at frame j0, the A operand is a Toeplitz slice of the IR,
// A[m][k] = h[t0 - j0 + m - k]: it depends on the diagonal d = t0 - j0 alone, a multiple of 16 here, so the packer builds every
// diagonal's fragment once (aidax_ir.cpp: pack_ir_fragments, 3 KiB per diagonal, 514 of them for 8192 taps) and the kernel loads them
// ready, in lane order, from L2. The B operand is the stream's input window, out of its history ring in HBM.
// Both operands are split exactly into three bf16 terms (x = x0 + x1 + x2, 8 + 8 + 8 significant bits) and six of the nine term
// products go out on v_mfma_f32_16x16x32_bf16, the project's fp32-parity idiom (aidax_convs.hip): the three dropped ones are together
// <= 2^-23 |h x|. An IR of one non-zero tap that is a power of two (a delay, a gain of 2^-k) is exact: the output is the dry signal.
//
// A wave owns 4 output tiles (64 frames) x 4 stream groups (64 streams): 16 accumulators, 64 registers. Input window b of the wave
// (j0 = T + 32 - 32 b for the wave's first frame T) meets output tile a on diagonal q = a + 2 b - 2 (d = 16 q): tiles 2, 3 of window b
// and tiles 0, 1 of window b + 1 share their A fragments, which stay in registers from one step to the next; a window's B fragments
// serve all four tiles. Small pools (the LV2 instance's one stream) would leave the machine idle with one wave per 64 frames, so the
// windows are split over S workgroups (the K split, ir_k_splits) whose partial sums a second launch (k_ir_reduce) adds in a fixed order:
// no atomics, the same bits on every run. S == 1 writes the output directly.
//
// The history ring: per stream a row of R + 32 floats, R a power of two >= the pool's IR capacity + max_frames; frame p of the stream's life sits at
// p mod R, and the first 32 slots are mirrored behind slot R - 1, so that a lane's eight consecutive inputs are contiguous whatever the
// ring position. k_ir_append writes the block's dry samples into the ring before k_ir_conv reads it (the conv kernel then never reads
// what it writes: the output may be the same buffer as the dry input). Input frames past the block's end are read as zeros.
//
// Nothing here knows the capacity: ring mask and row, and every IR's diagonal count, are run-time arguments. At 65536 taps an IR has 4098
// diagonals (12.6 MiB of fragments) and a wave walks 2050 windows: frame and window numbers stay below 2^17 in the int arithmetic, ring
// positions are masked, and stream x row and fragment offsets are formed in size_t. The oldest window may reach up to 31 frames past
// the IR's last tap; those frames meet zero taps, and their ring slots are in range whatever they hold.
#include <hip/hip_runtime.h>
#include <cstdint>
#include "aidax_kernels.h"
#include "aidax_layout.h"

namespace aidax {

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 ir_bf16x8 __attribute__((ext_vector_type(8)));
typedef unsigned ir_u32x4 __attribute__((ext_vector_type(4)));

constexpr int kIrTiles = 4;        // output tiles of 16 frames per wave
constexpr int kIrGroups = 4;       // stream groups of 16 per wave

// a, b -> (bf16(a) | bf16(b) << 16), round to nearest even (one v_cvt_pk_bf16_f32)
__device__ __forceinline__ unsigned ir_pack_bf16(float a, float b)
{
    typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
    const bf16x2 v = { static_cast<__bf16>(a), static_cast<__bf16>(b) };
    unsigned u = __builtin_bit_cast(unsigned, v);
    asm volatile("" : "+v"(u));
    return u;
}

// eight fp32 values -> three terms of eight bf16 each, x = t0 + t1 + t2 exactly
__device__ __forceinline__ void ir_split8(float (&r)[8], ir_u32x4 (&t)[3])
{
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        unsigned p[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) p[i] = ir_pack_bf16(r[2 * i], r[2 * i + 1]);
        t[k] = ir_u32x4{ p[0], p[1], p[2], p[3] };
        if (k < 2) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                r[2 * i] -= __builtin_bit_cast(float, p[i] << 16);
                r[2 * i + 1] -= __builtin_bit_cast(float, p[i] & 0xffff0000u);
            }
        }
    }
}

__global__ __launch_bounds__(256) void k_ir_append(float* __restrict__ ring, uint32_t row, uint32_t mask, uint32_t pos,
                                                   const float* __restrict__ dry, uint32_t n_frames, uint32_t count)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    const uint32_t s = i / n_frames, t = i - s * n_frames;
    const float v = dry[i];
    const uint32_t k = (pos + t) & mask;
    float* r = ring + static_cast<size_t>(s) * row;
    r[k] = v;
    if (k < kIrMirror) r[k + mask + 1] = v;
}

// grid: (wave tiles along the block) x (work items of the plan) x S; one wave per workgroup. A work item is one IR and up to 64 streams
// that use it (aidax_pool.cpp: the plan): its fragments, diagonals and stream count are wave-uniform, and a lane finds its stream in each
// of the four groups through the item's stream list. With every stream on one IR the plan is the identity (item i: streams 64 i ..), the
// grid of a one-IR pool.
__global__ __launch_bounds__(64) void k_ir_conv(IrArgs a)
{
    const int lane = threadIdx.x;
    const int nl = lane & 15, g = lane >> 4;
    const int T = 64 * static_cast<int>(blockIdx.x);                  // the wave's first output frame
    const IrItem item = a.items[blockIdx.y];
    const int split = static_cast<int>(blockIdx.z);
    const int n = static_cast<int>(a.n_frames);
    const int Q = static_cast<int>(item.n_diag);
    const int nb = (Q + 1) / 2 + 1;                                    // windows b = 0 .. nb-1 meet a diagonal q in [0, Q)
    const int per = (nb + static_cast<int>(a.n_splits) - 1) / static_cast<int>(a.n_splits);
    const int b_lo = split * per, b_hi = b_lo + per < nb ? b_lo + per : nb;

    bool tile_on[kIrTiles], grp_on[kIrGroups];
#pragma unroll
    for (int i = 0; i < kIrTiles; ++i) tile_on[i] = T + 16 * i < n;
    // a group with streams of the pass: its first one is (an item's list is in stream order, so a group that starts at or beyond a
    // prefix pass's n_streams has no lane on, and skips its MFMAs as the one-IR kernel skipped the groups past the prefix)
#pragma unroll
    for (int i = 0; i < kIrGroups; ++i) grp_on[i] = 16u * i < item.count && a.streams[item.first + 16u * i] < a.n_streams;
    // this lane's stream in each group, and its ring row (a lane past the item's end, or on a stream past the pass's prefix, reads zeros)
    const float* rows[kIrGroups];
    uint32_t strm[kIrGroups];
    bool lane_on[kIrGroups];
#pragma unroll
    for (int i = 0; i < kIrGroups; ++i) {
        const uint32_t k = 16u * i + static_cast<uint32_t>(nl);
        strm[i] = k < item.count ? a.streams[item.first + k] : 0u;
        lane_on[i] = k < item.count && strm[i] < a.n_streams;
        rows[i] = a.ring + static_cast<size_t>(lane_on[i] ? strm[i] : 0u) * a.ring_row;
    }
    const bool aligned = (a.pos & 3u) == 0u;                           // the lanes' 8-frame windows start on 16-byte boundaries

    f32x4 acc[kIrTiles][kIrGroups];
#pragma unroll
    for (int i = 0; i < kIrTiles; ++i)
#pragma unroll
        for (int j = 0; j < kIrGroups; ++j) acc[i][j] = f32x4{ 0.f, 0.f, 0.f, 0.f };

    const ir_u32x4* frag = reinterpret_cast<const ir_u32x4*>(item.frag) + lane;
    auto load_a = [&](int q, ir_u32x4 (&f)[3]) {
        if (q >= 0 && q < Q) {
#pragma unroll
            for (int term = 0; term < 3; ++term) f[term] = frag[(static_cast<size_t>(q) * 3 + term) * 64];
        } else {
#pragma unroll
            for (int term = 0; term < 3; ++term) f[term] = ir_u32x4{ 0u, 0u, 0u, 0u };
        }
    };
    ir_u32x4 alo[2][3], ahi[2][3];
    load_a(2 * b_lo - 2, alo[0]);
    load_a(2 * b_lo - 1, alo[1]);

    for (int b = b_lo; b < b_hi; ++b) {
        const int j0 = T + 32 - 32 * b;                                // the window's first input frame (block-relative, may be < 0)
        load_a(2 * b, ahi[0]);
        load_a(2 * b + 1, ahi[1]);
        if (j0 < n) {                                                  // (a window wholly past the block's end contributes nothing)
            const int jl = j0 + 8 * g;                                 // this lane's eight inputs: frames jl .. jl + 7
            const uint32_t idx = (a.pos + static_cast<uint32_t>(jl)) & a.mask;
            ir_u32x4 bt[kIrGroups][3];
#pragma unroll
            for (int i = 0; i < kIrGroups; ++i) {
                float x[8];
                if (!grp_on[i]) continue;
                if (aligned) {
                    const f32x4* p = reinterpret_cast<const f32x4*>(rows[i] + idx);
                    const f32x4 v0 = p[0], v1 = p[1];
                    x[0] = v0.x; x[1] = v0.y; x[2] = v0.z; x[3] = v0.w; x[4] = v1.x; x[5] = v1.y; x[6] = v1.z; x[7] = v1.w;
                } else {
#pragma unroll
                    for (int e = 0; e < 8; ++e) x[e] = rows[i][idx + e];
                }
#pragma unroll
                for (int e = 0; e < 8; ++e)
                    if (!lane_on[i] || jl + e >= n) x[e] = 0.f;
                ir_split8(x, bt[i]);
            }
#pragma unroll
            for (int t = 0; t < kIrTiles; ++t) {
                const int q = 2 * b - 2 + t;
                if (!tile_on[t] || q < 0 || q >= Q) continue;
                const ir_u32x4 (&af)[3] = t < 2 ? alo[t] : ahi[t - 2];
#pragma unroll
                for (int i = 0; i < kIrGroups; ++i) {
                    if (!grp_on[i]) continue;
                    // (h0 h1 h2) x0 | (h0 h1) x1 | h0 x2: the six term products, the large ones first
#pragma unroll
                    for (int th = 0; th < 3; ++th)
#pragma unroll
                        for (int tw = 0; tw < 3 - th; ++tw)
                            acc[t][i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(ir_bf16x8, af[tw]), __builtin_bit_cast(ir_bf16x8, bt[i][th]), acc[t][i], 0, 0, 0);
                }
            }
        }
#pragma unroll
        for (int k = 0; k < 2; ++k)
#pragma unroll
            for (int term = 0; term < 3; ++term) alo[k][term] = ahi[k][term];
    }

    // a lane holds frames t0 + 4 g .. + 3 of its stream in group i: the output row, or this split's partial row
    float* dst = a.n_splits > 1 ? a.part + static_cast<size_t>(split) * a.n_streams * a.n_frames : a.out;
#pragma unroll
    for (int i = 0; i < kIrGroups; ++i) {
        if (!grp_on[i] || !lane_on[i]) continue;
        float* r = dst + static_cast<size_t>(strm[i]) * a.n_frames;
#pragma unroll
        for (int t = 0; t < kIrTiles; ++t) {
            const int f = T + 16 * t + 4 * g;
            if (f + 0 < n) r[f + 0] = acc[t][i].x;
            if (f + 1 < n) r[f + 1] = acc[t][i].y;
            if (f + 2 < n) r[f + 2] = acc[t][i].z;
            if (f + 3 < n) r[f + 3] = acc[t][i].w;
        }
    }
}

// the K split's partial sums, added in split order (the same bits on every run), for the streams of the plan only: a stream on no IR
// keeps its dry row. Thread i: entry i / n_frames of the stream lists, frame i % n_frames
__global__ __launch_bounds__(256) void k_ir_reduce(const float* __restrict__ part, float* __restrict__ out, const uint32_t* __restrict__ streams,
                                                   uint32_t n_listed, uint32_t n_streams, uint32_t n_frames, uint32_t n_splits)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_listed * n_frames) return;
    const uint32_t j = i / n_frames;
    const uint32_t s = streams[j];
    if (s >= n_streams) return;
    const uint32_t e = s * n_frames + (i - j * n_frames);
    const size_t count = static_cast<size_t>(n_streams) * n_frames;
    // (eight loads in flight at a time, added in split order: a small pool's 64 partials cost 8 round trips, not 64)
    float v = part[e];
    uint32_t k = 1;
    for (; k + 8 <= n_splits; k += 8) {
        float t[8];
#pragma unroll
        for (int j8 = 0; j8 < 8; ++j8) t[j8] = part[static_cast<size_t>(k + j8) * count + e];
#pragma unroll
        for (int j8 = 0; j8 < 8; ++j8) v += t[j8];
    }
    for (; k < n_splits; ++k) v += part[static_cast<size_t>(k) * count + e];
    out[e] = v;
}

// The crossfade of an IR change, in place on the first lf frames of the fading streams' output rows (which hold the new side: the
// main section's convolution, or the dry block of a stream that goes to no IR). The old side is the fade-out section's row of the side
// buffer, or, for a stream that came from no IR, its dry samples out of the history ring. Thread i: entry i / lf of `mix`, frame i % lf.
// Both weights are quotients of small integers, rounded once each; at the last frame they are 1 and 0, and the new side comes out as it is.
__global__ __launch_bounds__(256) void k_ir_fade(IrFadeArgs a)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.n_mix * a.lf) return;
    const uint32_t j = i / a.lf, t = i - j * a.lf;
    const uint32_t e = a.mix[j];
    const uint32_t s = e & ~kIrFadeDry;
    if (s >= a.n_streams) return;
    const size_t at = static_cast<size_t>(s) * a.n_frames + t;
    const float was = (e & kIrFadeDry) ? a.ring[static_cast<size_t>(s) * a.ring_row + ((a.pos + t) & a.mask)] : a.side[at];
    const float lf = static_cast<float>(a.lf);
    const float w = static_cast<float>(t + 1u) / lf, u = static_cast<float>(a.lf - 1u - t) / lf;
    a.out[at] = __builtin_fmaf(w, a.out[at], u * was);
}

// The blend of two IRs, in place on ALL frames of the blended streams' output rows (which hold the A side: the main section's
// convolution, or the dry block of a stream whose A is no IR). The B side is the blend section's row of the side buffer, or the dry
// samples out of the history ring. Thread i: entry i / n_frames of `list`, frame i % n_frames. The weight is a function of the ramp
// frame alone (aidax_kernels.h): every fp64 operation is rounded on its own (no contraction in here; the v_fma_f64 of the disassembly
// are the division's own refinement steps), so a ramp gives the same bits however the host cuts it into blocks.
__global__ __launch_bounds__(256) void k_ir_mix(IrBlendArgs a)
{
#pragma clang fp contract(off)
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.n_blend * a.n_frames) return;
    const uint32_t j = i / a.n_frames, t = i - j * a.n_frames;
    const IrBlendEntry e = a.list[j];
    const uint32_t s = e.stream & ~kIrBlendDry;
    if (s >= a.n_streams) return;
    const uint32_t k = e.k + a.k_off + t;                              // (<= 2^24 + 2^25 + the block: no wrap)
    const double wd = ramp_value(e.m0, e.m1, e.ramp, k);               // (behind the ramp's end: m1 itself)
    const float w = static_cast<float>(wd), u = static_cast<float>(1.0 - wd);
    const size_t at = static_cast<size_t>(s) * a.n_frames + t;
    if (w == 0.f) return;                                              // A's bits, as they are
    const float yb = (e.stream & kIrBlendDry) ? a.ring[static_cast<size_t>(s) * a.ring_row + ((a.pos + t) & a.mask)] : a.side[at];
    if (w == 1.f) { a.out[at] = yb; return; }
    const float ua = u * a.out[at];
    a.out[at] = __builtin_fmaf(w, yb, ua);
}

}  // namespace

uint32_t ir_diagonals(uint32_t n_taps) { return (n_taps + 30u) / 16u + 1u; }
uint32_t ir_windows(uint32_t n_diag) { return (n_diag + 1u) / 2u + 1u; }

uint32_t ir_k_splits(uint32_t n_items, uint32_t n_frames, uint32_t n_diag, int cus, uint32_t cap)
{
    if (n_frames == 0 || n_items == 0) return 1;
    const uint32_t waves = ((n_frames + 63u) / 64u) * n_items;
    const uint32_t target = 4u * static_cast<uint32_t>(cus > 0 ? cus : 256);         // a wave per SIMD
    uint32_t s = (target + waves - 1u) / waves;
    const uint32_t nb = ir_windows(n_diag);
    if (s > nb / 4u) s = nb / 4u;                                                  // at least four windows per split
    if (s > cap) s = cap;
    return s ? s : 1u;
}

hipError_t launch_ir_append(float* ring, uint32_t ring_row, uint32_t mask, uint32_t pos, const float* dry, uint32_t n_streams, uint32_t n_frames,
                            hipStream_t q)
{
    if (n_frames == 0 || n_streams == 0) return hipSuccess;
    const uint32_t count = n_streams * n_frames;
    hipLaunchKernelGGL(k_ir_append, dim3((count + 255u) / 256u), dim3(256), 0, q, ring, ring_row, mask, pos, dry, n_frames, count);
    return hipGetLastError();
}

hipError_t launch_ir_conv(const IrArgs& a, hipStream_t q)
{
    if (a.n_frames == 0 || a.n_items == 0 || a.n_listed == 0) return hipSuccess;
    hipLaunchKernelGGL(k_ir_conv, dim3((a.n_frames + 63u) / 64u, a.n_items, a.n_splits), dim3(64), 0, q, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess || a.n_splits <= 1) return e;
    const uint32_t count = a.n_listed * a.n_frames;
    hipLaunchKernelGGL(k_ir_reduce, dim3((count + 255u) / 256u), dim3(256), 0, q, a.part, a.out, a.streams, a.n_listed, a.n_streams, a.n_frames, a.n_splits);
    return hipGetLastError();
}

hipError_t launch_ir_fade(const IrFadeArgs& a, hipStream_t q)
{
    if (a.n_mix == 0 || a.lf == 0 || a.n_frames == 0) return hipSuccess;
    const uint32_t count = a.n_mix * a.lf;
    hipLaunchKernelGGL(k_ir_fade, dim3((count + 255u) / 256u), dim3(256), 0, q, a);
    return hipGetLastError();
}

hipError_t launch_ir_mix(const IrBlendArgs& a, hipStream_t q)
{
    if (a.n_blend == 0 || a.n_frames == 0) return hipSuccess;
    const uint32_t count = a.n_blend * a.n_frames;
    hipLaunchKernelGGL(k_ir_mix, dim3((count + 255u) / 256u), dim3(256), 0, q, a);
    return hipGetLastError();
}

}  // namespace aidax
