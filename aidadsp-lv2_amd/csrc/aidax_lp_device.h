// aidax_lp_device.h — what the register-resident matrix-core kernels share: k_mfma_lp (aidax_mfmalp.hip), its bf16 x 3 twin
// k_mfma_ls / k_mfma_ls1 (aidax_mfmals.h) and the tick kernels k_gru_gm / k_gru_gs / k_lstm_gs (aidax_tick.hip). Staging and ring
// constants, the ring's 16-byte device-scope accesses, the helper waves of the one-launch forms (lp_helper), the chain passes around
// a body (lp_chain_rows), the exact bf16 x 3 split of fp32 values, and the launch helpers of the host side.
#pragma once
#include <cstdlib>
#include "aidax_device.h"
#include "aidax_kernels.h"
#include "aidax_layout.h"

namespace aidax {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kLpChunk = 256;            // frames of audio staged in LDS at a time
constexpr int kLpRing = 32;              // frames of h in flight between two layers
constexpr int kLpBatch = 8;              // frames per counter update (a release costs ~2-6 us, an acquire ~1.7 us: MI355X_MICROARCH.md)
// (a ring of 16 with counters every 4: cfg5 710.1 against 707.7 us, within the noise — profiles/r05_cfg5_modes.txt)
// A waiting workgroup gives up after kLpGiveUpTicks of the 100 MHz wall clock (250 ms: far beyond any wait that co-tenant
// kernels can cause while the partner still gets a CU — a launch must end even if its partner never runs). The pass is then
// wrong; the workgroup says so in the pool's fault word (pinned host memory), the pool reports AIDAX_ERR_DEVICE for it
// and serves the model with k_mfma from then on (aidax_pool.cpp).
constexpr uint64_t kLpGiveUpTicks = 25000000ull;
__device__ __forceinline__ bool lp_timed_out(uint32_t& spins, uint64_t& t0)
{
    if (spins++ == 0) { t0 = wall_clock64(); return false; }
    return (spins & 63u) == 0 && wall_clock64() - t0 > kLpGiveUpTicks;
}

// Tiles per wave whose input half moves from the upper layer's workgroup to the lower one's. Two layers: the upper
// has 8G k-steps per tile, the lower 4G + 1 — moving one tile's input half (4G MFMAs per wave) evens them out
// (LSTM-96: 75 / 144 -> 99 / 120 MFMAs per wave and frame). Deeper stacks are bound by their last layer either way.
// LSTM-96 (three tiles per wave): one moved tile still leaves 99 / 120; the waves of a workgroup's FIRST half move two
// and those of the second half one (waves w and w + NW/2 share a SIMD, so every SIMD carries one of each): 111 / 108.
// Returned as the LARGEST count a wave moves: 2 means "two for waves < NW/2, one for the others".
// (Only with eight waves: four waves sit on a SIMD each, and an uneven split would just make the slowest wave slower.)
__host__ __device__ constexpr int lp_moved_tiles(int n_layers, int tpw, int nw) { return n_layers != 2 ? 0 : (nw == 8 && tpw == 3) ? 2 : tpw >= 2 ? 1 : 0; }
constexpr int kLpCounterStride = 32;     // uint32 per (group, boundary): produced at [0], consumed at [16] (own cache lines)

// 16-byte device-scope (sc0 sc1) accesses: write-through stores / L1-bypassing loads. Buffer instructions, so the
// compiler keeps track of their completion (vmcnt) like of any other load.
typedef unsigned lp_u32x4 __attribute__((ext_vector_type(4)));
constexpr int kLpDeviceScope = 17;                         // aux bits: sc0 | sc1
// (The ring's loads / stores at a nearer scope — sc1, sc0 or none — buy no time, and below device scope a layer on another XCD reads
// stale lines: profiles/r05_cfg5_modes.txt, profiles/r04_ls_parts8.txt.)
__device__ __forceinline__ __amdgpu_buffer_rsrc_t lp_rsrc(const float* base, size_t bytes)
{
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(base), 0, (int)bytes, 0x00020000);
}
__device__ __forceinline__ f32x4 lp_load16(__amdgpu_buffer_rsrc_t r, uint32_t byte_off)
{
    return __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(r, byte_off, 0, kLpDeviceScope));
}
__device__ __forceinline__ void lp_store16(__amdgpu_buffer_rsrc_t r, uint32_t byte_off, f32x4 v)
{
    __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(lp_u32x4, v), r, byte_off, 0, kLpDeviceScope);
}

__device__ __forceinline__ float lp_row_sum16(float v)
{
    v = v + dpp_take<0xB1, 0xf>(v);
    v = v + dpp_take<0x4E, 0xf>(v);
    v = v + dpp_take<0x141, 0xf>(v);
    v = v + dpp_take<0x140, 0xf>(v);
    return v;
}

#ifdef AIDAX_LP_TRACE
#define LP_STAMP(k) do { if ((int)blockIdx.x == ((AIDAX_TUNE(a) >> 16) & 0xff) && tick >= kTraceT0 && tick < kTraceT0 + 8) {                         \
        __builtin_amdgcn_sched_barrier(0); const unsigned long long t_ = clock64(); __builtin_amdgcn_sched_barrier(0); \
        if ((threadIdx.x & 63) == 0) trace[((tick - kTraceT0) * 12 + (threadIdx.x >> 6)) * 8 + (k)] = t_; } } while (0)
#else
#define LP_STAMP(k) do {} while (0)
#endif

// ---------------------------------------------------------------- one-launch form: the helper waves
// One-layer models whose main waves leave room for a third wave per SIMD (lp_helpers) run their whole run() in this
// launch: NHELP extra waves, each the keeper of 16 / NHELP streams of the group in 8-lane groups like k_chain's. A helper
//   * runs the PRE pass (LPF -> pre-gain ramp -> EQ-pre) on its streams' rows in LDS ahead of the frame loop — as many
//     macro-steps of eight frames as the cascade is deep before the first tick, one more per tick until the chunk is done;
//   * writes the model inputs of the next frame (x * in_gain, the PARAM smoothers' samples) and finishes the Dense of
//     the frame before last (partial sums, bias, skip, output gain) — what lane < 16 of wave 0 did at the head of every
//     tick while seven waves waited (scratch/lp_trace.py: 2 100 cycles against 460);
//   * runs the POST pass (DC blocker -> EQ-post -> master ramp) over the finished frames, one macro-step whenever eight
//     more are there, the rest after the last tick, and stores the rows.
// The passes are k_chain's own (chain_macro_step): same operations per sample and stage, bit-identical state. The helper
// meets the main waves at every barrier — of lp_body's one-launch form (aidax_mfmalp.hip) and of the tick kernels' frame, where the
// protocol is written down barrier by barrier (tick_frame, aidax_tick.hip): (1) .. (5) below are its numbers, and the sequences on both
// sides must stay the same.
template <int H, int NW, int NHELP>
__device__ __forceinline__ void lp_helper(const LaunchArgs& a, float* xb, float* xin, const float* wdl, float* livef,
                                          const float* dpart, float* hands, int grp, int nP)
{
    constexpr int NS = kMfmaStreams;
    constexpr int SPH = NS / NHELP;                        // streams per helper wave
    static_assert(SPH * NHELP == NS && SPH <= 8, "eight lanes per stream");
    if (!(AIDAX_TUNE(a) & 1024)) __builtin_amdgcn_s_setprio(3);   // (measurement: AIDAX_TUNE bit 1024 leaves the helpers at the main waves' priority)
    const int lane = threadIdx.x & 63;
    const int hw = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)) - NW;
    const int gl = lane >> 3, stage = lane & 7;
    const int n = (int)a.n_frames;
    const int I = a.input_size;
    const int s_base = grp * NS;
    const bool slot_ok = gl < SPH;                         // this lane group stands for stream slot `sl` of the group
    const int sl = hw * SPH + (slot_ok ? gl : 0);
    const bool valid = slot_ok && s_base + sl < (int)a.n_streams;
    const int sg = valid ? s_base + sl : s_base;           // the others shadow the group's first stream and never store
    const bool keeper = slot_ok && stage == 0;             // the lane that does the per-stream scalar work

    const StreamCtl& ctl = a.ctl[sg];
    StreamState& st = a.st[sg];
    const uint32_t flags = ctl.flags;
    const uint32_t pending0 = st.pending;
    const bool live = valid && n != 0 && (flags & CTL_ENABLED);                 // :607-619
    const bool net = live && (flags & CTL_NET_ON);                             // :631-632

    ParamRamps pr;
    pr.load(st);
    uint32_t pending = pending0 & ~PEND_ACTIVATE;
    if (net) {
        pending = pr.begin_block(ctl, pending);
    }
    if (keeper) livef[sl] = net ? 1.f : 0.f;

    // the two passes of this lane's stage, set up like k_chain<true> / k_chain<false>
    ChainPass P, Q;
    const int slot_p = chain_setup<true>(P, ctl, st, flags, stage);
    const GainLatch pre0 = chain_latch<true>(P, ctl, st, pending0, live);
    const int slot_q = chain_setup<false>(Q, ctl, st, flags, stage);
    const GainLatch master0 = chain_latch<false>(Q, ctl, st, pending0, live);
    const bool run_p = live && stage < P.K, run_q = live && stage < Q.K;
    const bool general = (AIDAX_TUNE(a) & 8) != 0;
    const int depth_p = general || __builtin_amdgcn_ballot_w64(run_p && stage > 0) != 0 ? 6 : 1;
    const int depth_q = general || __builtin_amdgcn_ballot_w64(run_q && stage > 0) != 0 ? 6 : 1;
    float* row = xb + sl * nP;
    float* hand_p = hands + (size_t)(2 * hw) * kChainHandFloats;
    float* hand_q = hand_p + kChainHandFloats;
#ifdef AIDAX_LP_TRACE
    unsigned long long* trace = reinterpret_cast<unsigned long long*>(hands + NHELP * 2 * kChainHandFloats);
    constexpr int kTraceT0 = 96;
#endif
    __syncthreads();                                       // (1) set-up

    auto write_xin = [&](int parity, int f) {              // x * in_gain, PARAM1, PARAM2 of frame f (:171-181, :195-231)
        float q1 = 0.f, q2 = 0.f;
        if (I >= 2) q1 = pr.next1();
        if (I >= 3) q2 = pr.next2();
        if (keeper) {
            float* col = xin + parity * 64;
            col[sl] = net ? row[f] * a.in_gain : 0.f;
            col[NS + sl] = q1;
            col[2 * NS + sl] = q2;
            col[3 * NS + sl] = 0.f;
        }
    };

    for (int base = 0; base < n; base += kLpChunk) {
        const int cnt = n - base < kLpChunk ? n - base : kLpChunk;
        const int n_full = cnt & ~(kChainBlock - 1);
        __syncthreads();                                   // (2) the chunk's rows are in LDS
        ChainJob jp, jq;
        chain_job_begin(jp, P, stage, run_p, n_full, general);
        bool p_open = true;
        auto pre_work = [&](int steps) {                   // the ragged tail right behind the last whole block
            for (int k = 0; k < steps && chain_job_pending(jp, depth_p); ++k) chain_job_step(jp, P, stage, run_p, row, hand_p, lane);
            if (p_open && !chain_job_pending(jp, depth_p)) {
                chain_job_end(jp, P, run_p);
                if (n_full != cnt) chain_sweep<1>(P, stage, run_p, depth_p, row + n_full, row + n_full, cnt - n_full);
                p_open = false;
            }
        };
        pre_work(depth_p);                                 // frames 0..7 (and what a short chunk has) are final: block 0 has left the cascade after `depth` macro-steps
        chain_job_begin(jq, Q, stage, run_q, n_full, general);
        write_xin(0, 0);
        __syncthreads();                                   // (3)
        const int ticks = cnt + 2;
        for (int tick = 0; tick < ticks; ++tick) {
            LP_STAMP(0);
            if (tick >= 2 && keeper) {                     // Dense of frame tick-2: the waves' partial sums, bias, skip, gain
                const int fd = tick - 2;
                float y = wdl[H];
#pragma unroll
                for (int w = 0; w < NW; ++w) y += dpart[(((tick - 1) & 1) * NW + w) * NS + sl];
                const float x = row[fd] * a.in_gain;
                float o = a.input_skip ? x + y : y;
                o = o * a.out_gain;
                if (net) row[fd] = o;
            }
            __builtin_amdgcn_wave_barrier();
            // frames 0 .. tick-2 of the rows are model output now: a post-pass step when eight more are there
            if (chain_job_pending(jq, depth_q) && chain_job_needs(jq) <= tick - 1) chain_job_step(jq, Q, stage, run_q, row, hand_q, lane);
            pre_work(1);
            if (tick + 1 < cnt) write_xin((tick + 1) & 1, tick + 1);
            LP_STAMP(4);
            __syncthreads();                               // the tick's barrier
            LP_STAMP(5);
        }
        while (chain_job_pending(jq, depth_q)) chain_job_step(jq, Q, stage, run_q, row, hand_q, lane);
        chain_job_end(jq, Q, run_q);
        if (n_full != cnt) chain_sweep<1>(Q, stage, run_q, depth_q, row + n_full, row + n_full, cnt - n_full);
        __builtin_amdgcn_wave_barrier();
        // every valid row goes out: processed, or — a disabled stream — the raw input (the hard bypass copy of :612-619)
        for (int g = 0; g < SPH; ++g) {
            const int s2 = s_base + hw * SPH + g;
            if (s2 >= (int)a.n_streams) continue;
            if ((a.ctl[s2].flags & CTL_ENABLED) || a.out != a.in) {
                float* dst = a.out + (size_t)s2 * n + base;
                const float* src = xb + (hw * SPH + g) * nP;
                if (((n | base) & 3) == 0) store_block(dst, src, cnt, lane);
                else for (int t = lane; t < cnt; t += kWave) dst[t] = src[t];
            }
        }
        __syncthreads();                                   // (4) the rows may be overwritten
    }
#ifdef AIDAX_LP_TRACE
    if ((int)blockIdx.x == ((AIDAX_TUNE(a) >> 16) & 0xff)) __syncthreads();
#endif
    __syncthreads();                                       // (5)
    if (!valid) return;
    if (run_p) { st.z[slot_p][0] = P.z1; st.z[slot_p][1] = P.z2; }
    if (run_q) { st.z[slot_q][0] = Q.z1; st.z[slot_q][1] = Q.z2; }
    if (stage == 0) { st.pre_mem = live ? P.g.mem : pre0.mem; st.pre_tgt = pre0.tgt; }
    if (stage == Q.gain_lane) { st.master_mem = live ? Q.g.mem : master0.mem; st.master_tgt = master0.tgt; }
    if (keeper) {
        st.pending = pending;
        if (net) {
            pr.store(st);
        }
    }
}

// Stacked models, the one-launch form: their main waves hold the whole register file, so there is no room for helper waves
// — the packed chain passes (k_chain's body, chain_wave_pass) run on waves 0 and 1 of the first / last layer's workgroup
// BEFORE and AFTER lp_body, which stays exactly the body that runs between two k_chain launches (reshaping it for rows kept
// in LDS cost its frame loop 6 %: 1 096 -> 1 150 us on LSTM-96 x2 before a single chain instruction ran). The pre pass
// reads a.in and leaves its rows in a.out, where the body expects them — the LAST layer's workgroup needs them too (the model
// input for in_skip, and what a net-off stream delivers) and WAITS for them: the first layer's workgroup stores the rows
// write-through (device scope) and lets the stores drain before it computes its first frame, so the last layer's workgroup
// loads its rows only once frames exist in the ring below it (lp_body: the wait it has to do anyway, moved in front of
// the load). (Round 3's first version let the
// last layer's workgroup run the pre pass itself, uncommitted: it read the biquad states the first layer's workgroup was
// about to overwrite — right while the two started together, wrong once in 150 runs of the test suite.) The post pass
// takes the rows the body stored. Blocks of one staging chunk.
template <bool PRE>
__device__ __forceinline__ void lp_chain_rows(const LaunchArgs& a, float* smem, int grp, bool commit)
{
    constexpr int NS = kMfmaStreams;
    const int NT = (int)blockDim.x;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int n = (int)a.n_frames;
    const int nP = (n + 3) & ~3;
    const int s_base = grp * NS;
    float* rows = smem;                                    // [NS][nP]
    float* hands = rows + NS * nP;                         // [2][kChainPackHandFloats]
    const float* src_base = PRE ? a.in : a.out;
    // Device-scope loads, past this CU's vector cache. POST: the rows were stored by this workgroup a moment ago, and the
    // body's own read of them may have left their lines there, stale. PRE: with a.in == a.out the body would otherwise
    // find the lines this read brought in instead of the rows stored below.
    for (int i = tid; i < NS * n; i += NT) {
        const int sl = i / n, t = i - sl * n, sg = s_base + sl;
        rows[sl * nP + t] = sg < (int)a.n_streams ? __hip_atomic_load(src_base + (size_t)sg * n + t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0.f;
    }
    __syncthreads();
    if (wave < 2)
        chain_wave_pass<PRE>(a, s_base + kChainWaveStreams * wave, rows + kChainWaveStreams * wave * nP, nP,
                             hands + wave * kChainPackHandFloats, n, lane, commit, !PRE);
    __syncthreads();
    // PRE: every valid row goes to out (a disabled stream's row is still the raw input: the hard bypass copy of :612-619);
    // POST: only rows that were processed
    for (int i = tid; i < NS * n; i += NT) {
        const int sl = i / n, t = i - sl * n, sg = s_base + sl;
        if (sg >= (int)a.n_streams) continue;
        const bool row_live = (a.ctl[sg].flags & CTL_ENABLED) != 0;
        if (PRE ? (row_live || a.out != a.in) : row_live)           // (device scope: another workgroup reads the pre pass's rows)
            __hip_atomic_store(a.out + (size_t)sg * n + t, rows[sl * nP + t], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __syncthreads();                                       // (waits for the stores: the body's loads come after them)
}

// ---------------------------------------------------------------- exact bf16 x 3 split (k_gru_gs, k_lstm_gs, k_mfma_ls: see aidax_tick.hip)
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

// a, b -> (bf16(a) | bf16(b) << 16), round to nearest even
__device__ __forceinline__ unsigned gs_pack_bf16(float a, float b)
{
    typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
    const bf16x2 v = { static_cast<__bf16>(a), static_cast<__bf16>(b) };
    unsigned u = __builtin_bit_cast(unsigned, v);
    asm volatile("" : "+v"(u));                               // ONE v_cvt_pk_bf16_f32: left to itself the compiler converts each value again to widen it back
    return u;
}
// four fp32 values -> three terms of four bf16 each (term t: two dwords), v = t0 + t1 + t2 exactly
typedef float gs_f32x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ void gs_split4(const float (&v)[4], u32x2 (&t)[3])
{
    // The residuals' subtractions two values per instruction (v_pk_add_f32: the same IEEE subtraction per value). The main waves of the
    // tick kernels share their SIMD with one helper wave: they issue like a lone wave, for which a packed instruction costs what a plain
    // one does (profiles/r05_lone_wave_issue.txt) — and this split sits between a tick's last MFMA and its barrier.
    // (One value per instruction, here and in k_gru_gs's cell update: cfg3 192.6 against 188.0 us, profiles/r05_DESIGN_archive.md.)
    gs_f32x2 r01 = { v[0], v[1] }, r23 = { v[2], v[3] };
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const unsigned p01 = gs_pack_bf16(r01.x, r01.y), p23 = gs_pack_bf16(r23.x, r23.y);
        t[k] = u32x2{ p01, p23 };
        if (k < 2) {
            r01 = r01 - gs_f32x2{ __builtin_bit_cast(float, p01 << 16), __builtin_bit_cast(float, p01 & 0xffff0000u) };
            r23 = r23 - gs_f32x2{ __builtin_bit_cast(float, p23 << 16), __builtin_bit_cast(float, p23 & 0xffff0000u) };
        }
    }
}

// ---------------------------------------------------------------- host side: launching
typedef void (*LpFn)(LaunchArgs, MfmaDesc, float*, uint32_t*, uint32_t*);
typedef void (*GmFn)(LaunchArgs, MfmaDesc);
[[maybe_unused]] constexpr int kLpHelpers = 4;
// The chained kernels (two or more layers: workgroups that wait for each other) go out through hipLaunchCooperativeKernel: the
// runtime REFUSES a grid that cannot be co-resident on the device (hipErrorCooperativeLaunchTooLarge — the pool then serves the
// model with k_mfma at once, aidax_pool.cpp) and schedules the grid as a gang, so that another process's kernels cannot sit
// between its workgroups: next to a process that keeps every CU busy a cfg5 block took 7.8 ms through the plain launch and
// 0.71 ms through this one; alone it costs 15 us per block (698 -> 713 us, profiles/r04_lp_coop.txt). AIDAX_LP_COOP=0: the
// plain launch (A/B runs).
[[maybe_unused]] static bool lp_coop_launch()
{
    static const bool on = [] { const char* e = AIDAX_HOOK_ENV("AIDAX_LP_COOP"); return !(e && e[0] == '0'); }();
    return on;
}
[[maybe_unused]] static hipError_t lp_launch(LpFn fn, uint32_t blocks, uint32_t threads, size_t lds, hipStream_t stream, LaunchArgs a, MfmaDesc d,
                            float* ring, uint32_t* counters, uint32_t* fault)
{
    if (lp_coop_launch() && d.n_layers >= 2) {
        void* args[] = { &a, &d, &ring, &counters, &fault };
        return hipLaunchCooperativeKernel(reinterpret_cast<const void*>(fn), dim3(blocks), dim3(threads), args, (unsigned)lds, stream);
    }
    hipLaunchKernelGGL(fn, dim3(blocks), dim3(threads), lds, stream, a, d, ring, counters, fault);
    return hipGetLastError();
}
// more than 64 KiB of dynamic LDS has to be asked for, kernel by kernel
template <typename Fn>
[[maybe_unused]] static hipError_t lp_allow_lds(Fn fn, size_t bytes)
{
    if (bytes <= 64 * 1024) return hipSuccess;
    return hipFuncSetAttribute(reinterpret_cast<const void*>(fn), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
}

}  // namespace aidax
