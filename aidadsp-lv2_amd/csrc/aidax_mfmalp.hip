// aidax_mfmalp.hip — k_mfma_lp: STACKED recurrent models on the matrix cores, one workgroup per (16 streams, LAYER),
// the layers of a stream group chained through a small ring in global memory.
//
// Why: k_mfma (aidax_mfma.hip) gives a group of 16 streams ONE workgroup that walks all layers, streaming 437 KiB of
// A fragments from L2 every frame (LSTM-96 x2). At BASELINE cfg5's per-GPU size (2048 streams = 128 groups) that
// fills half of the 256 CUs, and the fragment stream plus its address arithmetic sits between the MFMAs. Here
//   * a group's layers run on SEPARATE workgroups (2048 streams x 2 layers = 256 workgroups: every CU busy), layer l
//     one or more frames behind layer l-1;
//   * each workgroup keeps ITS layer's A fragments in registers for the whole launch (LSTM-96 layer 1: 384 rows x
//     192 columns = 288 KiB = 144 registers per lane over 8 waves): the frame loop is MFMAs fed by one
//     conflict-free ds_read_b32 per k-step, no global loads, no address arithmetic;
//   * h of layer l-1 travels to layer l through a ring of kLpRing frames in global memory, in the layout layer l
//     reads it in ([unit][stream] = ready B fragments). ONE-directional hand-over in the write-through form of
//     cdna_hip_programming.md G16: the payload leaves as 16-byte device-scope (sc1) stores and is read with 16-byte
//     sc1 loads, so no L2 write-back and no L1 invalidate is ever needed (measured here: an agent-scope release costs
//     the publishing wave ~18 k cycles, 16 producers per XCD flushing one L2); the producer publishes a frame counter
//     every kLpBatch frames after its stores have drained (per-wave s_waitcnt vmcnt(0) -> barrier), the consumer's lane
//     0 polls it only when it has used up what it knows of; the producer waits only when the ring is full.
//     Latency of the hand-over is hidden by the skew between the layers, nobody waits per frame.
//
// Forward progress: the pool uses this kernel only while groups x layers <= the number of CUs (one workgroup
// fits per CU), so EVERY workgroup of the grid becomes resident whatever the dispatch order, and a spinning consumer
// can never keep its producer off the machine. (Forced on larger pools with AIDAX_MFMA_LP=1 — measurements only —
// it leans on the dispatcher's observed id order: a layer's workgroup has a LOWER id than the layer above it, ids of
// one group are 8 apart.) Every spin is bounded in time. The premise also needs the grid to have the CUs to itself: the
// pool lets ONE pool per device use this kernel, warms models up with k_mfma and never puts two of these grids in flight
// (aidax_pool.cpp, lp_gate); what it cannot see (another process on the GPU) ends in a reported give-up. Nothing depends on placement: ids of one group being equal modulo
// 8 puts them on one XCD under the observed b % 8 placement, a locality hint only.
//
// Same arithmetic as k_mfma (same fragments from pack_mfma, same accumulation order, same activations): the two
// kernels leave bit-identical recurrent state on the same model, which tests/test_gpu_parity.py checks (Dense(H,1) is
// summed in a different order, so the outputs agree to ~1e-7).
//
// Two one-launch forms live here too: one-layer models with helper waves for the DSP chain (lp_helper) and stacked models with the
// packed chain passes around the unchanged body (lp_chain_rows); both building blocks are in aidax_lp_device.h, which this file
// shares with the tick kernels (aidax_tick.hip) and the bf16 x 3 twin k_mfma_ls (aidax_mfmals.h).
#include "aidax_lp_device.h"

namespace aidax {

__host__ __device__ inline size_t lp_lds_floats(int hidden, int n_frames, int n_helpers = 0)
{
    const size_t nP = (size_t)(((n_frames < kLpChunk ? n_frames : kLpChunk) + 3) & ~3);
    return (size_t)kMfmaStreams * nP                          /* xb: audio rows (first and last layer)   */
         + 2 * 64                                             /* xin[parity][4][n]  (first layer)        */
         + (size_t)2 * hidden * kMfmaStreams                  /* below[parity][unit][n] (layers >= 1)    */
         + (size_t)2 * hidden * kMfmaStreams                  /* hT[parity][unit][n]                     */
         + (size_t)hidden * kMfmaStreams                      /* cT[unit][n]                             */
         + (size_t)((hidden + 1 + 3) & ~3)                    /* Dense weights + bias (last layer)       */
         + kMfmaStreams                                       /* live flags                              */
         + 2 * 8 * kMfmaStreams                               /* Dense partial sums [parity][wave][n]    */
         + (size_t)n_helpers * 2 * kChainHandFloats           /* one-launch form: hand-over slots of the helper waves' pre and post pass */
#ifdef AIDAX_LP_TRACE
         + 2048                                               /* scratch/lp_trace.py: time stamps of eight ticks, 12 waves, 8 stamps (u64) needs 1536 floats */
#endif
         ;
}

// one frame in the ring: h [unit][stream], then (M > 0) the pre-activations of the first M tiles of every wave of the
// layer above, started by the layer below ([wave][tile][lane] x 4 gate rows)
__host__ __device__ constexpr size_t lp_slot_floats(int hidden, int waves, int m) { return (size_t)hidden * kMfmaStreams + (size_t)waves * m * kWave * 4; }
__host__ __device__ constexpr size_t lp_ring_floats(int hidden, int waves, int m) { return (size_t)kLpRing * lp_slot_floats(hidden, waves, m); }

// acc[tl] += A(groups G0..G0+NG) . B, A resident in `wres`, B fragments from `src` ([unit][stream] in LDS).
// The B values of group g+1 are read while the MFMAs of group g issue (two register sets alternate by the parity of
// g under the full unroll): left to itself the compiler reads a pair of values, waits for the LDS, issues six MFMAs,
// and exposes the LDS latency 24 times per layer half.
template <int TPW, int NG, int G0, int NRES, int TL0 = 0, int TL1 = TPW, int NACC = TPW>
__device__ __forceinline__ void lp_gates(f32x4 (&acc)[NACC], const f32x4 (&wres)[NRES], const float* src, int lane)
{
    if constexpr (TL0 < TL1) {
        float b0[4], b1[4];
        auto read_b = [&](float (&b)[4], int g) {
#pragma unroll
            for (int j = 0; j < 4; ++j) b[j] = src[256 * g + 64 * j + lane];
        };
        auto group = [&](const float (&b)[4], int g) {
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int tl = TL0; tl < TL1; ++tl) {
                    const int e = j * TPW + tl;
                    acc[tl] = __builtin_amdgcn_mfma_f32_16x16x4f32(wres[(G0 + g) * TPW + e / 4][e % 4], b[j], acc[tl], 0, 0, 0);
                }
        };
        read_b(b0, 0);
#pragma unroll
        for (int g = 0; g < NG; ++g) {
            if (g & 1) {
                if (g + 1 < NG) read_b(b0, g + 1);
                __builtin_amdgcn_sched_barrier(0);
                group(b1, g);
            } else {
                if (g + 1 < NG) read_b(b1, g + 1);
                __builtin_amdgcn_sched_barrier(0);
                group(b0, g);
            }
            __builtin_amdgcn_sched_barrier(0);
        }
    }
}

// M: tiles per wave of the layer above whose input half the first layer computes (lp_moved_tiles; two-layer models).
// FIRST / LAST: the role of this workgroup's layer, a compile-time constant of the body — the kernel branches once on the
// layer index, so each role's registers are allocated for that role only (the first layer carries no fetched tiles, no
// Dense fragments; the others no started-tile accumulators): LSTM-96 x2 fits its 256 registers without scratch.
template <int TPW, int NW, int M, bool FIRST, bool LAST, int NHELP = 0, bool CHAIN = false>
__device__ __forceinline__ void lp_body(const LaunchArgs& a, const MfmaDesc& d, float* ring, uint32_t* counters, uint32_t* fault,
                                        float* smem, int grp, int l)
{
    constexpr int H = 4 * TPW * NW;
    constexpr int NT = NW * kWave;
    constexpr int NS = kMfmaStreams;
    constexpr int G = H / 16;                              // k-step groups per H columns
    constexpr int NRES = 2 * G * TPW;                      // f32x4 of resident A fragments: [h below | own h]
    constexpr int MA = M > 0 ? M : 1;                      // array extent of the moved-tile registers
    constexpr size_t kSlot = lp_slot_floats(H, NW, M);     // floats of one ring frame
    static_assert(NHELP == 0 || (FIRST && LAST), "helper waves serve one-layer models");
    constexpr bool fused = NHELP > 0;                      // the whole run() in this launch: a.in -> a.out, MODE_CHAIN only
    // CHAIN: the kernel runs the DSP chain around this body (lp_chain_rows); the body itself is the same as between two
    // k_chain launches, except that it clears its bit of StreamState::pending with an atomic.
    constexpr bool chain = CHAIN;
    static_assert(!(CHAIN && NHELP > 0), "one form or the other");
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int mw = M == 2 ? (wave < NW / 2 ? 2 : 1) : M;   // tiles THIS wave moves (M == 2: the first half of the waves two, the others one)
    const int n = (int)a.n_frames;
    const int NL = d.n_layers;
    const int Ht = d.hidden_true;
    const int I = a.input_size;
    const int mode = a.mode;
    const int blk = (int)blockIdx.x;
    constexpr bool first = FIRST, last = LAST;
    const int s_base = grp * NS;
    const int chunk = n < kLpChunk ? n : kLpChunk;
    const int nP = (chunk + 3) & ~3;

    float* xb    = smem;                                   // [NS][nP]
    float* xin   = xb + NS * nP;                           // [2][4][NS]
    float* below = xin + 2 * 64;                           // [2][H][NS]
    float* hT    = below + 2 * H * NS;                     // [2][H][NS]
    float* cT    = hT + 2 * H * NS;                        // [H][NS]
    float* wdl   = cT + H * NS;                            // Dense weights, bias at [H]
    float* livef = wdl + ((H + 1 + 3) & ~3);               // [NS]
    float* dpart = livef + NS;                             // [2][NW][NS] Dense partial sums of the waves (last layer)
#ifdef AIDAX_LP_TRACE
    // measurement build only (scratch/lp_trace.py): workgroup 0 stamps the shader clock at six points of ticks 96..103
    unsigned long long* trace = reinterpret_cast<unsigned long long*>(dpart + 2 * 8 * NS + NHELP * 2 * kChainHandFloats);
    constexpr int kTraceT0 = 96;
#endif

    if constexpr (fused) {
        if (wave >= NW) {
            lp_helper<H, NW, NHELP>(a, xb, xin, wdl, livef, dpart, dpart + 2 * 8 * NS, grp, nP);
            return;
        }
    }
    const float* W = a.wpack;
    const MfmaLayer& L = d.L[l];

    // ---- per-stream bookkeeping: lanes tid < NS own stream s_base+tid (live flag; PARAM smoothers on the first layer)
    ParamRamps pr{};
    uint32_t pending = 0, st_pending0 = 0;
    bool mine_live = false;
    if (!fused && tid < NS) {
        const int sg = s_base + tid;
        const bool valid = sg < (int)a.n_streams;
        if (valid) {
            StreamState& st = a.st[sg];
            pr.load(st);
            pending = st_pending0 = st.pending;
            if (mode == MODE_CHAIN) {
                const StreamCtl& ctl = a.ctl[sg];
                const uint32_t flags = ctl.flags;
                mine_live = n != 0 && (flags & CTL_ENABLED) && (flags & CTL_NET_ON);      // :607-619, :631-632
                if (mine_live) {
                    pending = pr.begin_block(ctl, pending);
                }
            } else {
                mine_live = n != 0 && (mode == MODE_WARMUP || sg == 0);
            }
        }
        livef[tid] = mine_live ? 1.f : 0.f;
    }
    if (last) for (int i = tid; i < H + 1; i += NT) wdl[i] = W[d.wd_off + i];
    // this layer's recurrent state -> LDS (parity 0 is what frame 0 reads)
    for (int i = tid; i < H * NS; i += NT) {
        const int u = i / NS, sn = i % NS, sg = s_base + sn;
        const bool valid = sg < (int)a.n_streams;
        const float* stp = a.nn + (size_t)(valid ? sg : 0) * a.nn_stride + L.state_off;
        hT[i] = (valid && u < Ht) ? stp[u] : 0.f;           // padded units rest at 0
        cT[i] = (valid && u < Ht && L.cell == 0) ? stp[Ht + u] : 0.f;
    }

    // ---- this layer's bias rows (the accumulators start from them) and A fragments, resident for the launch
    f32x4 bias_r[TPW];
#pragma unroll
    for (int tl = 0; tl < TPW; ++tl)
        bias_r[tl] = *reinterpret_cast<const f32x4*>(W + L.b_off + 4 * (4 * (wave * TPW + tl) + (lane >> 4)));
    // One register set, two uses that exclude each other: on the first layer the bias rows the moved tiles start from
    // (the upper layer's), on the others the started tiles of the NEXT frame on their way in from the ring.
    f32x4 upx[MA];
#pragma unroll
    for (int tl = 0; tl < MA; ++tl)
        upx[tl] = (M > 0 && first) ? *reinterpret_cast<const f32x4*>(W + d.L[M > 0 ? 1 : 0].b_off + 4 * (4 * (wave * TPW + tl) + (lane >> 4)))
                                    : f32x4{ 0.f, 0.f, 0.f, 0.f };
    // Dense(H,1) on the matrix cores (last layer): y = wd . h is one more 16-row tile whose row 0 is wd; its H/4
    // k-steps are dealt out TPW per wave, each wave leaves a partial sum per stream in LDS and wave 0 adds the NW
    // partials in a fixed order a tick later. (As VALU code — six LDS reads with bank conflicts, a DPP tree, twice per
    // SIMD — it cost ~1000 cycles per tick next to the MFMA stretch; this way it is TPW MFMAs per wave.)
    float dfrag[TPW];
#pragma unroll
    for (int i = 0; i < TPW; ++i)
        dfrag[i] = (last && (lane & 15) == 0) ? W[d.wd_off + 4 * (wave * TPW + i) + (lane >> 4)] : 0.f;
    float w_in0[TPW];
#pragma unroll
    for (int tl = 0; tl < TPW; ++tl) w_in0[tl] = first ? W[d.L[0].w_in_off + ((size_t)wave * kWave + lane) * TPW + tl] : 0.f;
    f32x4 wres[NRES];
    {
        const int g_tot = first ? G : 2 * G;
        const f32x4* ap = reinterpret_cast<const f32x4*>(W + L.w_big_off) + ((size_t)wave * g_tot * kWave + lane) * TPW;
        const f32x4* ap_up = reinterpret_cast<const f32x4*>(W + d.L[M > 0 ? 1 : 0].w_big_off) + ((size_t)wave * 2 * G * kWave + lane) * TPW;
#pragma unroll
        for (int g = 0; g < 2 * G; ++g)
#pragma unroll
            for (int q = 0; q < TPW; ++q) {
                // first layer: its G groups (own h) sit in the upper half, like the recurrent half of the others; with
                // M > 0 its lower half holds the layer ABOVE's input-half fragments (same wave, same lane): it starts
                // that layer's first M tiles
                const int gs = first ? g - G : g;
                if (gs >= 0) wres[g * TPW + q] = ap[(size_t)gs * kWave * TPW + q];
                else if (M > 0) wres[g * TPW + q] = ap_up[(size_t)g * kWave * TPW + q];
                else wres[g * TPW + q] = f32x4{ 0.f, 0.f, 0.f, 0.f };
            }
    }

    // ---- ring bookkeeping. Counters count frames since the buffers were allocated and are equal on both sides
    // between launches, so a workgroup starts from its own side's value.
    const size_t ring_stride = lp_ring_floats(H, NW, M);
    float* ring_out = last ? nullptr : ring + ((size_t)grp * (NL - 1) + l) * ring_stride;
    const float* ring_in = first ? nullptr : ring + ((size_t)grp * (NL - 1) + (l - 1)) * ring_stride;
    const size_t ring_bytes = ring_stride * sizeof(float);
    const __amdgpu_buffer_rsrc_t rs_out = lp_rsrc(last ? ring : ring_out, ring_bytes);
    const __amdgpu_buffer_rsrc_t rs_in = lp_rsrc(first ? ring : ring_in, ring_bytes);
    uint32_t* cnt_out = last ? nullptr : counters + ((size_t)grp * (NL - 1) + l) * kLpCounterStride;
    uint32_t* cnt_in = first ? nullptr : counters + ((size_t)grp * (NL - 1) + (l - 1)) * kLpCounterStride;
    auto give_up = [&]() { __hip_atomic_fetch_add(fault, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM); };
    if ((AIDAX_TUNE(a) & 16) && blk == 0 && tid == 0) give_up();      // test hook: report a give-up that did not happen
    // every thread needs the bases (they place a frame in the ring); the running counts are thread 0's business
    const uint32_t base_out = cnt_out ? __hip_atomic_load(cnt_out, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0u;
    const uint32_t base_in = cnt_in ? __hip_atomic_load(cnt_in + 16, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0u;
    uint32_t known_free = kLpRing;                         // frames of this launch the ring above is known to have room for
    uint32_t known_below = 0;                              // frames of this launch known to exist below
    __syncthreads();

    // Frame Fprev goes up the ring, one tick after it was computed (h_src = h(Fprev), stable in LDS for this tick):
    // h as 16-byte write-through stores, and (first layer, M > 0) the started tiles of the layer above:
    // W_in(above)[first M tiles] . h(Fprev) + bias.
    constexpr int kHVec = H * NS / 4;                       // f32x4 of one h tile
    auto ship_frame = [&](const float* h_src, int Fprev) {
        const uint32_t slot_off = (uint32_t)(((base_out + (uint32_t)Fprev) % kLpRing) * kSlot * sizeof(float));
        for (int i = tid; i < kHVec; i += NT)
            lp_store16(rs_out, slot_off + (uint32_t)i * 16u, reinterpret_cast<const f32x4*>(h_src)[i]);
        if constexpr (M > 0) {
            if (first) {
                f32x4 pacc[MA];
#pragma unroll
                for (int tl = 0; tl < M; ++tl) pacc[tl] = upx[tl];
                if constexpr (M == 2) {
                    if (mw == 2) lp_gates<TPW, G, 0, NRES, 0, 2, MA>(pacc, wres, h_src, lane);
                    else lp_gates<TPW, G, 0, NRES, 0, 1, MA>(pacc, wres, h_src, lane);
                } else {
                    lp_gates<TPW, G, 0, NRES, 0, M, MA>(pacc, wres, h_src, lane);
                }
#pragma unroll
                for (int tl = 0; tl < M; ++tl)
                    if (tl < mw)
                        lp_store16(rs_out, slot_off + (uint32_t)(H * NS * sizeof(float)) + (uint32_t)(((wave * M + tl) * kWave + lane) * 16), pacc[tl]);
            }
        }
    };
    // the cell state of this lane's (unit, stream) pairs — one per tile — lives in registers for the launch (cT is only how
    // it travels between the state records and the lanes)
    float creg[TPW];
#pragma unroll
    for (int tl = 0; tl < TPW; ++tl) creg[tl] = cT[(wave * TPW + tl) * 64 + lane];
    // frames [0, total) of this launch as the ring sees them
    int par = 0;                                           // parity of hT the next frame reads
    int done = 0;                                          // frames finished before this chunk
    for (int base = 0; base < n; base += kLpChunk) {
        const int cnt = n - base < kLpChunk ? n - base : kLpChunk;
        // what the layer below hands over: frame F of the launch sits in ring slot (base_in + F) % kLpRing
        auto wait_below = [&](int frames_needed) {        // thread 0 only: until `frames_needed` frames of the launch exist
            if (frames_needed > n) frames_needed = n;
            uint32_t spins = 0;
            uint64_t t0 = 0;
            while ((int)known_below < frames_needed) {
                known_below = __hip_atomic_load(cnt_in, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) - base_in;
                if ((int)known_below < frames_needed) {
                    if (lp_timed_out(spins, t0)) { give_up(); known_below = (uint32_t)n; break; }
                    __builtin_amdgcn_s_sleep(8);
                }
            }
        };
        // ---- audio rows of this chunk: the first layer reads them as input, the last for in_skip and to deliver
        if constexpr (chain && last && !first) {
            // one-launch form: the rows in a.out are the pre pass's, stored (write-through, drained) by the FIRST layer's
            // workgroup before it computed its first frame — once frames exist below, the rows are there
            if (tid == 0) wait_below(done + 2);
            __syncthreads();
            // ... and must come from L2: the rows of neighbouring stream groups can share a cache line (odd block lengths),
            // and another workgroup on this CU may have brought that line in before the pre pass stored into it
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        }
        if (first || last) {
            for (int sl = wave; sl < NS; sl += NW) {
                const int sg = s_base + sl;
                const bool lv = fused ? sg < (int)a.n_streams : livef[sl] != 0.f;     // one-launch form: every row, the chains run on net-off streams too
                float* row = xb + sl * nP;
                if (fused) {
                    const float* src = a.in + (size_t)(lv ? sg : 0) * n + base;
                    if (lv && ((n | base) & 3) == 0) load_block(row, src, cnt, lane);
                    else for (int t = lane; t < cnt; t += kWave) row[t] = lv ? src[t] : 0.f;
                } else if (lv && mode == MODE_CHAIN) {
                    const float* src = a.out + (size_t)sg * n + base;
                    if (((n | base) & 3) == 0) load_block(row, src, cnt, lane);
                    else for (int t = lane; t < cnt; t += kWave) row[t] = src[t];
                } else if (lv && mode == MODE_NN_ONLY) {
                    for (int t = lane; t < cnt; t += kWave) row[t] = a.in[(size_t)(base + t) * I];
                } else {
                    for (int t = lane; t < cnt; t += kWave) row[t] = 0.f;
                }
            }
        }
        __syncthreads();
        auto write_xin = [&](int parity, int f) {
            // lanes tid < NS: x * in_gain, PARAM1, PARAM2 of frame `f` (:171-181, :195-231)
            float q1 = 0.f, q2 = 0.f;
            if (mode == MODE_CHAIN) {
                if (I >= 2) q1 = pr.next1();
                if (I >= 3) q2 = pr.next2();
            } else if (mode == MODE_WARMUP) {             // constant params over the zero pre-buffer (:1077-1078)
                q1 = I >= 2 ? pr.mem[0] : 0.f;
                q2 = I >= 3 ? pr.mem[1] : 0.f;
            } else if (tid == 0) {
                q1 = I >= 2 ? a.in[(size_t)(base + f) * I + 1] : 0.f;
                q2 = I >= 3 ? a.in[(size_t)(base + f) * I + 2] : 0.f;
            }
            float* col = xin + parity * 64;
            col[tid] = xb[tid * nP + f] * a.in_gain;
            col[NS + tid] = q1;
            col[2 * NS + tid] = q2;
            col[3 * NS + tid] = 0.f;
        };
        constexpr int PER4 = (kHVec + NT - 1) / NT;        // f32x4 of a frame each thread moves
        f32x4 pre[PER4];
        f32x4 pcur[MA] = {};                               // started tiles of the current frame (layers >= 1, M > 0); the next frame's: upx
        auto fetch_below = [&](int F) {                    // all threads: frame F of the launch -> registers
            const uint32_t slot_off = (uint32_t)(((base_in + (uint32_t)F) % kLpRing) * kSlot * sizeof(float));
#pragma unroll
            for (int q = 0; q < PER4; ++q)
                if (q * NT + tid < kHVec) pre[q] = lp_load16(rs_in, slot_off + (uint32_t)(q * NT + tid) * 16u);
            if constexpr (M > 0) {                         // ... and this wave's started tiles straight into registers
#pragma unroll
                for (int tl = 0; tl < M; ++tl)
                    if (tl < mw)
                        upx[tl] = lp_load16(rs_in, slot_off + (uint32_t)(H * NS * sizeof(float)) + (uint32_t)(((wave * M + tl) * kWave + lane) * 16));
            }
        };
        auto stash_below = [&](int parity) {
#pragma unroll
            for (int q = 0; q < PER4; ++q)
                if (q * NT + tid < kHVec) reinterpret_cast<f32x4*>(below + parity * H * NS)[q * NT + tid] = pre[q];
        };

        if (first) {
            if (!fused && tid < NS) write_xin(0, 0);
        } else {
            if (tid == 0) wait_below(done + 2);            // frame 0 of the chunk for now, frame 1 for tick 0's prefetch
            __syncthreads();
            fetch_below(done);
            stash_below(0);
#pragma unroll
            for (int tl = 0; tl < MA; ++tl) pcur[tl] = upx[tl];
        }
        __syncthreads();

        const int ticks = last ? cnt + 2 : cnt;            // the Dense of a frame: partial sums one tick behind its h, the output two
        for (int tick = 0; tick < ticks; ++tick) {
            const int rd = par, wr = par ^ 1;
            const bool body = tick < cnt;
            const bool more = tick + 1 < cnt;              // another frame of this chunk follows
            const int F = done + tick;                     // frame of the launch this tick computes
            LP_STAMP(0);
            // ---- the next frame's input on its way: model inputs (first layer) / h of the layer below into
            // registers (others; thread 0 made sure of its existence before the previous barrier)
            if (first) {
                if (!fused && tid < NS && more) write_xin((tick + 1) & 1, tick + 1);
            } else if (more) {
                fetch_below(F + 1);
            }
            if (body && tid == 0) {
                // thread 0 looks ahead while the others compute: the frame AFTER next must exist below before the
                // next tick fetches it, and the slot of the next frame must be free above before the next tick
                // stores into it. Normally both are known already; otherwise this wave spins and the workgroup
                // waits for it at the barrier. (A counter read costs this wave ~1.5 us once per kLpBatch ticks — at the START
                // of the tick, where its SIMD partner has the matrix pipe to itself meanwhile. Reading the counters early
                // and looking at them just before the barrier was measured: 1 265 -> 1 305 us, nothing overlaps there.)
                if (!first && tick + 2 < cnt) wait_below(F + 3);
                if (!last && base + tick + 1 < n) {
                    uint32_t spins = 0;
                    uint64_t t0 = 0;
                    while ((int)known_free < F + 2) {
                        const uint32_t consumed = __hip_atomic_load(cnt_out + 16, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) - base_out;
                        known_free = consumed + kLpRing;
                        if ((int)known_free < F + 2) {
                            if (lp_timed_out(spins, t0)) { give_up(); known_free = (uint32_t)n + kLpRing; break; }
                            __builtin_amdgcn_s_sleep(8);
                        }
                    }
                }
            }

            // ---- Dense(H,1) of frame tick-1: this wave's k-steps against h(tick-1) (= hT[rd], stable for the whole tick).
            // At the head of the tick on purpose: its LDS reads and two MFMAs run while the gates' first operands are still on
            // their way from LDS. (Issued behind the gates, with the partial sum leaving after the cell update: cfg5 1 130 ->
            // 1 156 us, GRU-64 446 -> 466 us.)
            if (last && tick >= 1 && tick <= cnt) {
                f32x4 dacc = f32x4{ 0.f, 0.f, 0.f, 0.f };
                const float* hv = hT + rd * H * NS;
#pragma unroll
                for (int i = 0; i < TPW; ++i)
                    dacc = __builtin_amdgcn_mfma_f32_16x16x4f32(dfrag[i], hv[64 * (wave * TPW + i) + lane], dacc, 0, 0, 0);
                if (lane < NS) dpart[((tick & 1) * NW + wave) * NS + lane] = dacc.x;      // row 0, column = stream `lane`
            }
            // ---- ... and of frame tick-2: the NW partial sums, bias, skip, output gain (wave 0, one lane per stream)
            if (!fused && last && tick >= 2 && wave == 0 && lane < NS) {
                const int fd = tick - 2;
                float y = wdl[H];
#pragma unroll
                for (int w = 0; w < NW; ++w) y += dpart[(((tick - 1) & 1) * NW + w) * NS + lane];
                const float x = xb[lane * nP + fd] * a.in_gain;
                float o = a.input_skip ? x + y : y;
                o = o * a.out_gain;
                if (livef[lane] != 0.f) xb[lane * nP + fd] = o;
            }

            LP_STAMP(1);
            if (body) {
                float* h_rd = hT + rd * H * NS;
                float* h_wr = hT + wr * H * NS;
                f32x4 acc[TPW];
#pragma unroll
                for (int tl = 0; tl < TPW; ++tl) acc[tl] = bias_r[tl];
                if (!last && F >= 1) ship_frame(h_rd, F - 1);          // h_rd = h(F-1)
                if (first) {                               // the model inputs: one k-step (x, PARAM1, PARAM2, 0)
                    const float b = xin[(tick & 1) * 64 + lane];
#pragma unroll
                    for (int tl = 0; tl < TPW; ++tl)
                        acc[tl] = __builtin_amdgcn_mfma_f32_16x16x4f32(w_in0[tl], b, acc[tl], 0, 0, 0);
                } else {
                    if constexpr (M > 0) {                 // the first M tiles arrive started (bias + input half), the others start here
#pragma unroll
                        for (int tl = 0; tl < M; ++tl)
                            if (tl < mw) acc[tl] = pcur[tl];
                    }
                    if constexpr (M == 2) {
                        if (mw == 2) lp_gates<TPW, G, 0, NRES, 2, TPW>(acc, wres, below + (tick & 1) * H * NS, lane);
                        else lp_gates<TPW, G, 0, NRES, 1, TPW>(acc, wres, below + (tick & 1) * H * NS, lane);
                    } else {
                        lp_gates<TPW, G, 0, NRES, M, TPW>(acc, wres, below + (tick & 1) * H * NS, lane);
                    }
                }
                LP_STAMP(2);
                lp_gates<TPW, G, G, NRES>(acc, wres, h_rd, lane);
                LP_STAMP(3);

#pragma unroll
                for (int tl = 0; tl < TPW; ++tl) {
                    const int e = (wave * TPW + tl) * 64 + lane;          // unit 4T + (lane>>4), stream lane&15
                    float hn;
                    if (L.cell == 0) {
                        const float gi = sigmoid_pre(acc[tl].x), gf = sigmoid_pre(acc[tl].y);
                        const float gg = tanh_rat(acc[tl].z), go = sigmoid_pre(acc[tl].w);
                        const float cn = __builtin_fmaf(gf, creg[tl], gi * gg);
                        creg[tl] = cn;
                        hn = go * tanh_rat(cn);
                    } else {
                        const float gz = sigmoid_pre(acc[tl].x), gr = sigmoid_pre(acc[tl].y);
                        const float nn = tanh_exp_pre(__builtin_fmaf(gr, acc[tl].z, acc[tl].w));      // (GRU: see GruCell::step)
                        hn = __builtin_fmaf(gz, h_rd[e] - nn, nn);
                    }
                    h_wr[e] = hn;
                }
                par = wr;
                LP_STAMP(4);
                if (!first && more) {
                    stash_below((tick + 1) & 1);
#pragma unroll
                    for (int tl = 0; tl < MA; ++tl) pcur[tl] = upx[tl];
                }
                if (!last) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");     // this wave's ring stores have left before the barrier (G16)
            }
            __syncthreads();                               // h(t) in LDS, the next frame's input in LDS, ring stores of this frame done
            LP_STAMP(5);
            // ---- counters, by thread 0 after the barrier: every kLpBatch frames and at the end of the launch
            if (body && tid == 0) {
                if (!last) {
                    // frames complete in the ring: a frame goes up one tick after it was computed (the last one
                    // after the loop); its write-through stores were drained before the barrier above
                    const int produced = F;
                    if (produced > 0 && produced % kLpBatch == 0)
                        __hip_atomic_store(cnt_out, base_out + (uint32_t)produced, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                }
                if (!first) {
                    const int consumed = more ? F + 2 : F + 1;             // frames read out of the ring so far
                    if (consumed % kLpBatch == 0 || consumed == n)
                        __hip_atomic_store(cnt_in + 16, base_in + (uint32_t)consumed, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                }
            }
        }
        done += cnt;
        // ---- results of this chunk back to HBM (last layer)
        if (last && !fused) {
            for (int sl = wave; sl < NS; sl += NW) {
                const int sg = s_base + sl;
                if (livef[sl] == 0.f || mode == MODE_WARMUP) continue;
                float* dst = mode == MODE_CHAIN ? a.out + (size_t)sg * n + base : a.out + base;
                const float* row = xb + sl * nP;
                if (((n | base) & 3) == 0 && mode == MODE_CHAIN) store_block(dst, row, cnt, lane);
                else for (int t = lane; t < cnt; t += kWave) dst[t] = row[t];
            }
        }
        __syncthreads();
    }

    if (!last && n > 0) {                                  // the launch's last frame, then the final count
        ship_frame(hT + par * H * NS, n - 1);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if (tid == 0) __hip_atomic_store(cnt_out, base_out + (uint32_t)n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }

#ifdef AIDAX_LP_TRACE
    if ((int)blockIdx.x == ((AIDAX_TUNE(a) >> 16) & 0xff)) { __syncthreads(); for (int i = tid; i < 2 * 768; i += NT) fault[16 + i] = reinterpret_cast<const uint32_t*>(trace)[i]; }
#endif
    // ---- recurrent state and smoother memories back to HBM for the streams that ran
#pragma unroll
    for (int tl = 0; tl < TPW; ++tl) cT[(wave * TPW + tl) * 64 + lane] = creg[tl];
    __syncthreads();
    for (int i = tid; i < H * NS; i += NT) {
        const int u = i / NS, sn = i % NS, sg = s_base + sn;
        if (sg < (int)a.n_streams && u < Ht && livef[sn] != 0.f) {
            float* stp = a.nn + (size_t)sg * a.nn_stride + L.state_off;
            stp[u] = hT[par * H * NS + i];
            if (L.cell == 0) stp[Ht + u] = cT[i];
        }
    }
    if (!fused && first && tid < NS && mine_live && mode == MODE_CHAIN) {
        StreamState& st = a.st[s_base + tid];
        pr.store(st);
        if (!chain) st.pending = pending;
        else if (pending != st_pending0)                  // (the last layer's workgroup clears PEND_ACTIVATE in the same word)
            __hip_atomic_fetch_and(&st.pending, ~(uint32_t)PEND_PARAM_FIRST, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

template <int TPW, int NW, int M, int NHELP = 0, bool CHAIN = false>
__global__ __launch_bounds__((NW + NHELP) * kWave) void k_mfma_lp(LaunchArgs a, MfmaDesc d, float* ring, uint32_t* counters, uint32_t* fault)
{
    extern __shared__ __attribute__((aligned(16))) float smem[];
    if constexpr (NHELP > 0) {                             // one layer, the whole run() of its streams: workgroup = stream group
        const int n_groups = ((int)a.n_streams + kMfmaStreams - 1) / kMfmaStreams;
        if ((int)blockIdx.x < n_groups) lp_body<TPW, NW, 0, true, true, NHELP>(a, d, ring, counters, fault, smem, (int)blockIdx.x, 0);
        return;
    }
    // workgroup id -> (group, layer): ids of one group are 8 apart, lower layers first
    // (AIDAX_TUNE bit 2 lays a group's layers out on ADJACENT ids instead — different XCDs under b % 8 — so that the
    // tests can exercise the cross-XCD hand-over too.)
    const int NL = d.n_layers;
    const int blk = (int)blockIdx.x;
    const bool adjacent = (AIDAX_TUNE(a) & 2) != 0;
    const int grp = adjacent ? blk / NL : (blk / (8 * NL)) * 8 + (blk & 7);
    const int l = adjacent ? blk % NL : (blk / 8) % NL;
    const int n_groups = ((int)a.n_streams + kMfmaStreams - 1) / kMfmaStreams;
    if (grp >= n_groups) return;
    if constexpr (CHAIN) {                                 // stacked models, and one-layer ones without room for helper waves
        if (NL == 1) {
            lp_chain_rows<true>(a, smem, grp, true);
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
            lp_body<TPW, NW, M, true, true, 0, true>(a, d, ring, counters, fault, smem, grp, l);
            __syncthreads();
            lp_chain_rows<false>(a, smem, grp, true);
        } else if (l == 0) {
            lp_chain_rows<true>(a, smem, grp, true);
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");           // (the body's loads of the rows: from L2, see lp_body)
            lp_body<TPW, NW, M, true, false, 0, true>(a, d, ring, counters, fault, smem, grp, l);
        } else if (l == NL - 1) {
            if (AIDAX_TUNE(a) & 8192) {                                          // test hook: this workgroup starts 100 us late
                const uint64_t t0 = wall_clock64();
                while (wall_clock64() - t0 < 10000) __builtin_amdgcn_s_sleep(64);
            }
            lp_body<TPW, NW, M, false, true, 0, true>(a, d, ring, counters, fault, smem, grp, l);
            __syncthreads();
            lp_chain_rows<false>(a, smem, grp, true);
        } else {
            lp_body<TPW, NW, M, false, false, 0, true>(a, d, ring, counters, fault, smem, grp, l);
        }
        return;
    }
    if (NL == 1) lp_body<TPW, NW, M, true, true>(a, d, ring, counters, fault, smem, grp, l);      // one layer: no ring, nobody waits
    else if (l == 0) lp_body<TPW, NW, M, true, false>(a, d, ring, counters, fault, smem, grp, l);
    else if (l == NL - 1) lp_body<TPW, NW, M, false, true>(a, d, ring, counters, fault, smem, grp, l);
    else lp_body<TPW, NW, M, false, false>(a, d, ring, counters, fault, smem, grp, l);
}

// ---------------------------------------------------------------- host side
// Helper waves of the one-launch form: a third wave per SIMD must fit next to the main waves' registers (512 per SIMD
// lane: H <= 64 at <= 160 registers; H = 80 / 96 hold 256 / 233 and keep the three-launch form).
static int lp_helpers(int hidden) { return hidden == 16 || hidden == 32 || hidden == 48 || hidden == 64 ? kLpHelpers : 0; }
static LpFn lp_fn_fused(int hidden)
{
    switch (hidden) {
#define AIDAX_LP_FUSED_CASE(HID) case HID: { constexpr int T = HID / 4 / mfma_waves(HID), W_ = mfma_waves(HID); return k_mfma_lp<T, W_, 0, kLpHelpers>; }
    AIDAX_LP_FUSED_CASE(16) AIDAX_LP_FUSED_CASE(32) AIDAX_LP_FUSED_CASE(48) AIDAX_LP_FUSED_CASE(64)
#undef AIDAX_LP_FUSED_CASE
    default: return nullptr;
    }
}
static LpFn lp_fn_chain(int hidden, int n_layers)         // the DSP chain on waves 0 and 1 of the first / last layer's workgroup
{
    switch (hidden) {
#define AIDAX_LP_CHAIN_CASE(HID) case HID: { constexpr int T = HID / 4 / mfma_waves(HID), W_ = mfma_waves(HID);                    \
        return lp_moved_tiles(2, T, W_) > 0 && n_layers == 2 ? k_mfma_lp<T, W_, lp_moved_tiles(2, T, W_), 0, true> : k_mfma_lp<T, W_, 0, 0, true>; }
    AIDAX_LP_CHAIN_CASE(16) AIDAX_LP_CHAIN_CASE(32) AIDAX_LP_CHAIN_CASE(48) AIDAX_LP_CHAIN_CASE(64) AIDAX_LP_CHAIN_CASE(80) AIDAX_LP_CHAIN_CASE(96)
#undef AIDAX_LP_CHAIN_CASE
    default: return nullptr;
    }
}
static LpFn lp_fn(int hidden, int n_layers)
{
    switch (hidden) {
#define AIDAX_LP_CASE(HID) case HID: { constexpr int T = HID / 4 / mfma_waves(HID), W_ = mfma_waves(HID);                         \
        return lp_moved_tiles(2, T, W_) > 0 && n_layers == 2 ? k_mfma_lp<T, W_, lp_moved_tiles(2, T, W_)> : k_mfma_lp<T, W_, 0>; }
    AIDAX_LP_CASE(16) AIDAX_LP_CASE(32) AIDAX_LP_CASE(48) AIDAX_LP_CASE(64) AIDAX_LP_CASE(80) AIDAX_LP_CASE(96)
#undef AIDAX_LP_CASE
    default: return nullptr;                               // wider stacks keep the fragment-streaming kernel
    }
}
static int lp_m(const MfmaDesc& d) { return lp_moved_tiles(d.n_layers, d.hidden / 4 / mfma_waves(d.hidden), mfma_waves(d.hidden)); }

// (one-layer models too: a workgroup per 16 streams with the layer's fragments resident in registers — no ring, no waits)
bool mfma_lp_serves(const MfmaDesc& d) { return d.n_layers >= 1 && lp_fn(d.hidden, d.n_layers) != nullptr; }
// which one-launch form a model takes: helper waves (one layer, room for a third wave per SIMD) or the chain passes on two
// main waves around the body (everything else)
static bool lp_helper_form(const MfmaDesc& d) { return d.n_layers == 1 && lp_helpers(d.hidden) > 0; }
size_t mfma_lp_lds_bytes(const MfmaDesc& d, uint32_t n_frames, bool fused)
{
    if (fused && !lp_helper_form(d)) {                     // lp_chain_rows works in the body's LDS before and after it
        const size_t body = lp_lds_floats(d.hidden, (int)n_frames), rows = (size_t)kMfmaStreams * ((n_frames + 3) & ~3u) + 2 * kChainPackHandFloats;
        return (body > rows ? body : rows) * sizeof(float);
    }
    return lp_lds_floats(d.hidden, (int)n_frames, fused ? lp_helpers(d.hidden) : 0) * sizeof(float);
}
// the whole run() in the one launch (a.in -> a.out, MODE_CHAIN): one-layer models with room for the helper waves; all
// others (stacked, or one layer of 80 / 96 units) when their blocks fit one staging chunk (lp_chain_rows around the body)
bool mfma_lp_fused_serves(const MfmaDesc& d, uint32_t max_frames)
{
    return lp_helper_form(d) || (max_frames <= (uint32_t)kLpChunk && lp_fn_chain(d.hidden, d.n_layers) != nullptr);
}
size_t mfma_lp_ring_bytes(const MfmaDesc& d, uint32_t n_streams)
{
    const size_t groups = (n_streams + kMfmaStreams - 1) / kMfmaStreams;
    return 256 + groups * (size_t)(d.n_layers - 1) * lp_ring_floats(d.hidden, mfma_waves(d.hidden), lp_m(d)) * sizeof(float);
}
size_t mfma_lp_counter_bytes(const MfmaDesc& d, uint32_t n_streams)
{
    const size_t groups = (n_streams + kMfmaStreams - 1) / kMfmaStreams;
    return 256 + groups * (size_t)(d.n_layers - 1) * kLpCounterStride * sizeof(uint32_t);
}

hipError_t launch_mfma_lp_kernel(const LaunchArgs& a, const MfmaDesc& d, float* ring, uint32_t* counters, uint32_t* fault, hipStream_t stream, bool fused)
{
    if (fused && (!mfma_lp_fused_serves(d, a.n_frames) || a.mode != MODE_CHAIN || a.n_frames == 0)) return hipErrorInvalidValue;
    LpFn fn = !fused ? lp_fn(d.hidden, d.n_layers) : lp_helper_form(d) ? lp_fn_fused(d.hidden) : lp_fn_chain(d.hidden, d.n_layers);
    if (!fn || !ring || !counters || !fault) return hipErrorInvalidValue;
    const size_t lds = mfma_lp_lds_bytes(d, a.n_frames, fused);
    if (const hipError_t e = lp_allow_lds(fn, lds); e != hipSuccess) return e;
    const uint32_t groups = (a.n_streams + kMfmaStreams - 1) / kMfmaStreams;
    const uint32_t blocks = ((groups + 7) / 8) * 8 * (uint32_t)d.n_layers;
    const int waves = mfma_waves(d.hidden) + (fused && lp_helper_form(d) ? lp_helpers(d.hidden) : 0);
    return lp_launch(fn, blocks, (uint32_t)(waves * kWave), lds, stream, a, d, ring, counters, fault);
}

}  // namespace aidax
