// aidax_gate.hip — the per-stream noise gate ahead of a pool's model (include/aidax.h, "Noise gate"): k_gate.
//
// One launch reads the block a pass was handed, [n_active][n_frames] floats, and writes the gated block of the same shape into the pool's
// side block, which the model's launch then takes as its input. The rule is sequential per stream (a hold counter c and an attenuation
// position q, both integers, stepped once per frame), and it is evaluated here as two inclusive scans per chunk of 64 frames:
//
//   c: every frame is one of three maps on c, closed under composition —
//        SHIFT(n)        c -> max(c - n, 0)          a quiet frame is SHIFT(1)
//        THRESH(d, A, B) c -> c > d ? A : B          a frame at the close level is THRESH(0, hold, 0), one at the open level THRESH(0, hold, hold)
//      SHIFT(n1) then SHIFT(n2) = SHIFT(n1 + n2); SHIFT(n1) then THRESH(d, A, B) = THRESH(d + n1, A, B); THRESH(d, A, B) then f =
//      THRESH(d, f(A), f(B)).
//   q: given c, every frame is a clamped add q -> min(hi, max(lo, q + delta)) with (delta, lo, hi) = (-up, 0, P) while c > 0, else
//      (down, 0, P); g1 then g2 = (delta1 + delta2, g2(lo1), g2(hi1)). |delta| <= P = 2^24 per frame, so a chunk's sum fits int32; the
//      carry is folded in after every chunk, so nothing longer is ever summed.
//
// All of it is integer arithmetic: the scans give the sequential rule's (c, q) for every frame exactly, in any order of composition.
//
// One 64-lane wave per stream, four to a workgroup, one frame per lane (256-byte loads and stores, no alignment question at odd block
// lengths). The scans run on the DPP network (shifts inside the rows of 16 lanes, then two row broadcasts: no LDS traffic), and the next
// chunk's frames are loaded while a chunk is scanned. Lanes behind the row's end carry identity maps. Lane 0 reads the stream's 8-byte
// state before the first chunk and writes it behind the last: one wave owns a stream and passes are stream-ordered, so no LDS, no
// barrier, no atomic.
// A stream whose gate is off, or whose control record lacks CTL_ENABLED (a disabled plugin, a parked seat: the model kernels copy such a
// stream's input row raw, and that must be the ungated row), has its row copied bit for bit and its state left alone.
#include <hip/hip_runtime.h>
#include <cstdint>
#include "aidax_kernels.h"

namespace aidax {

namespace {

constexpr uint32_t kGateWaves = 4;             // streams of a workgroup

// a map on the hold counter: SHIFT(n) (thresh == 0, n in `d`) or THRESH(d, A, B)
struct HoldMap {
    uint32_t thresh, d, a, b;
};
__device__ __forceinline__ uint32_t apply(const HoldMap& f, uint32_t c)
{
    return f.thresh ? (c > f.d ? f.a : f.b) : (c > f.d ? c - f.d : 0u);
}
// f1 first, then f2
__device__ __forceinline__ HoldMap then(const HoldMap& f1, const HoldMap& f2)
{
    HoldMap r;
    if (f1.thresh) {
        r.thresh = 1u; r.d = f1.d; r.a = apply(f2, f1.a); r.b = apply(f2, f1.b);
    } else {
        r.thresh = f2.thresh; r.d = f1.d + f2.d; r.a = f2.a; r.b = f2.b;
    }
    return r;
}

// a map on the attenuation position: q -> min(hi, max(lo, q + delta))
struct RampMap {
    int32_t delta, lo, hi;
};
__device__ __forceinline__ int32_t apply(const RampMap& g, int32_t q)
{
    return min(g.hi, max(g.lo, q + g.delta));
}
__device__ __forceinline__ RampMap then(const RampMap& g1, const RampMap& g2)
{
    return { g1.delta + g2.delta, apply(g2, g1.lo), apply(g2, g1.hi) };
}

// The value `v` of the lane a DPP control names, `idle` where it names none (a shift past the row's start, a row the mask leaves out)
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ uint32_t dpp_or(uint32_t idle, uint32_t v)
{
    return static_cast<uint32_t>(__builtin_amdgcn_update_dpp(static_cast<int>(idle), static_cast<int>(v), CTRL, ROW_MASK, 0xf, false));
}
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ HoldMap lower_lane(const HoldMap& f)          // idle: SHIFT(0), the identity
{
    return { dpp_or<CTRL, ROW_MASK>(0u, f.thresh), dpp_or<CTRL, ROW_MASK>(0u, f.d), dpp_or<CTRL, ROW_MASK>(0u, f.a), dpp_or<CTRL, ROW_MASK>(0u, f.b) };
}
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ RampMap lower_lane(const RampMap& g)          // idle: (0, 0, P), the identity on [0, P]
{
    return { static_cast<int32_t>(dpp_or<CTRL, ROW_MASK>(0u, static_cast<uint32_t>(g.delta))), static_cast<int32_t>(dpp_or<CTRL, ROW_MASK>(0u, static_cast<uint32_t>(g.lo))),
             static_cast<int32_t>(dpp_or<CTRL, ROW_MASK>(kGateUnit, static_cast<uint32_t>(g.hi))) };
}
// The inclusive scan of the wave's 64 maps, lane 0's first: recursive doubling inside every row of 16 lanes (row_shr 1, 2, 4, 8), then
// the total of row 0 into row 1 and of row 2 into row 3 (row_bcast:15), then the total of rows 0 and 1 into rows 2 and 3 (row_bcast:31).
// Every step composes "the lower lanes' map first, then mine"; a lane without a lower partner composes with the identity.
template <class Map>
__device__ __forceinline__ Map wave_scan(Map f)
{
    f = then(lower_lane<0x111, 0xf>(f), f);
    f = then(lower_lane<0x112, 0xf>(f), f);
    f = then(lower_lane<0x114, 0xf>(f), f);
    f = then(lower_lane<0x118, 0xf>(f), f);
    f = then(lower_lane<0x142, 0xa>(f), f);
    f = then(lower_lane<0x143, 0xc>(f), f);
    return f;
}

__global__ __launch_bounds__(64 * kGateWaves) void k_gate(const float* in, float* out, const GateRec* rec, GateState* state, const StreamCtl* ctl,
                                                          uint32_t n_active, uint32_t n_frames)
{
    const uint32_t lane = threadIdx.x & 63u, s = blockIdx.x * kGateWaves + (threadIdx.x >> 6);
    if (s >= n_active) return;                                            // (the whole wave)
    const float* x_row = in + static_cast<size_t>(s) * n_frames;
    float* y_row = out + static_cast<size_t>(s) * n_frames;
    const GateRec r = rec[s];

    if (!r.on || !(ctl[s].flags & CTL_ENABLED)) {                         // (wave-uniform)
        const uint32_t* x_bits = reinterpret_cast<const uint32_t*>(x_row);
        uint32_t* y_bits = reinterpret_cast<uint32_t*>(y_row);
        for (uint32_t t = lane; t < n_frames; t += 64u) y_bits[t] = x_bits[t];
        return;
    }

    constexpr int32_t P = static_cast<int32_t>(kGateUnit);
    float x_next = lane < n_frames ? x_row[lane] : 0.f;                   // (a chunk's frames are loaded while the chunk before it is scanned)
    const GateState st = state[s];
    uint32_t c = min(st.hold_left, r.hold);                               // (a parameter change may have shortened the hold)
    int32_t q = static_cast<int32_t>(min(st.atten, kGateUnit));
    const int32_t up = static_cast<int32_t>(r.up), down = static_cast<int32_t>(r.down);

    for (uint32_t base = 0; base < n_frames; base += 64u) {
        const uint32_t t = base + lane;
        const bool valid = t < n_frames;
        const float x = x_next;
        x_next = t + 64u < n_frames ? x_row[t + 64u] : 0.f;
        const float a = __builtin_fabsf(x);                               // (a NaN compares false: a quiet frame)

        HoldMap f;
        if (!valid) f = { 0u, 0u, 0u, 0u };                               // identity
        else if (a >= r.t_open) f = { 1u, 0u, r.hold, r.hold };
        else if (a >= r.t_close) f = { 1u, 0u, r.hold, 0u };              // the close level only keeps an open gate open
        else f = { 0u, 1u, 0u, 0u };
        const uint32_t c_t = apply(wave_scan(f), c);

        RampMap g;
        if (!valid) g = { 0, 0, P };                                      // identity on [0, P]
        else if (c_t > 0u) g = { -up, 0, P };
        else g = { down, 0, P };
        const int32_t q_t = apply(wave_scan(g), q);

        if (valid) {
            float y = x;                                                  // q == 0: the input's bits
            if (q_t != 0) {
                const float w = __fmul_rn(static_cast<float>(P - q_t), 0x1p-24f);      // exact
                const float gain = __fadd_rn(r.floor, __fmul_rn(r.span, w));           // two roundings, no fma
                y = __fmul_rn(x, gain);
            }
            y_row[t] = y;
        }
        // the chunk's last lane holds the carry (lanes behind the row's end are identities)
        c = static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(c_t), 63));
        q = __builtin_amdgcn_readlane(q_t, 63);
    }
    if (lane == 0) state[s] = { c, static_cast<uint32_t>(q) };
}

}  // namespace

hipError_t launch_gate(const float* in, float* out, const GateRec* rec, GateState* state, const StreamCtl* ctl, uint32_t n_active, uint32_t n_frames,
                       hipStream_t q)
{
    if (n_active == 0 || n_frames == 0) return hipSuccess;
    k_gate<<<(n_active + kGateWaves - 1u) / kGateWaves, 64 * kGateWaves, 0, q>>>(in, out, rec, state, ctl, n_active, n_frames);
    return hipGetLastError();
}

}  // namespace aidax
