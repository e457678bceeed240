// aidax_mfmals.h — the templates of k_mfma_ls / k_mfma_ls1. Two objects instantiate them: aidax_mfmals.hip (a lone layer, stacks of
// three and more, the host side) and aidax_mfmals2.hip (the two-layer stacks: the longest compile of the tree, so on its own).
#pragma once
#include "aidax_lp_device.h"

namespace aidax {

// ================================================================ k_mfma_ls: k_mfma_lp with the contractions on the bf16 matrix pipe
// k_mfma_lp's design (aidax_mfmalp.hip: one workgroup per (16 streams, layer), the layer's fragments resident in registers, h on
// its way up through a ring in global memory, every wait bounded) with every fp32 product W . h computed as NPROD bf16 term
// products of operands split exactly into three bf16 terms — see k_gru_gs for the arithmetic and why (profiles/r04_overlap.txt:
// the fp32 MFMAs run at the vector rate and stall the VALU; the bf16 ones are sixteen times denser and hide it).
//   * Weights: the packer's ls record, [wave][tile][segment][k-step of 32][term] fragments of 8 bf16 per lane. A wave keeps
//     only the tile segments it multiplies with: its TPW own-h segments plus, on the first layer, the input-half segments of
//     the mw tiles it starts for the layer above — on the others, the input-half segments of the TPW - mw tiles that do not
//     arrive started (LSTM-96 x 2: five segments of 36 registers).
//   * h(t-1) of a layer lives in LDS as B fragments [parity][term][k-step][lane][8 bf16]; a lane splits its own h values after
//     the cell update and writes the three 2-byte terms where the k-steps read them. A frame in the ring is the fragments
//     as they lie in LDS (plus the started tiles, as before): the layer above copies them in and multiplies.
//   * Dense(H,1): multiply-adds on the lane's own h and two permlane swaps, the waves' partial sums added a tick later as before.
//   * The first layer's model inputs stay one fp32 k-step.
// Hand-over protocol, counters, give-up, the chain passes around the body: k_mfma_lp's, line for line.
// Geometry: k_mfma_lp's eight (four) waves while a wave's resident fragments fit 150 of its 256 registers; wider layers run FOUR
// waves — one per SIMD, 512 registers each (the fragments are MFMA operands only and may live in AGPRs) — with half of the
// upper layer's tiles started below, so that both workgroups of a group issue the same number of MFMAs (LSTM-96 x 2: six
// tiles per wave, nine resident segments of 36 registers, 162 bf16 MFMAs per wave and frame in either layer).
struct LsGeo { int nw, tpw, m, nx; };      // nx: resident tile segments of a wave besides its own-h ones (the larger role's; none for a lone layer)
__host__ __device__ constexpr int ls_ks2(int hidden) { return (hidden + 31) / 32; }
__host__ __device__ constexpr int ls_frag_vecs(int hidden) { return 3 * ls_ks2(hidden) * 64; }      // 16-byte vectors of one h buffer
__host__ __device__ constexpr int ls_segments(int tpw, int m) { return tpw + (tpw - m > m ? tpw - m : m); }      // resident tile segments of a wave (the larger role)
// LSTM-96 x 2 on eight waves: tiles per wave the lower layer starts for the upper one (1: 32 / 40 tile segments per workgroup, 2: 40 / 32;
// no measurement of 1 is recorded)
constexpr int kLsMoved96 = 2;
__host__ __device__ constexpr LsGeo ls_geo(int n_layers, int hidden)
{
    if (hidden < 16 || hidden % 16 != 0 || n_layers < 1) return LsGeo{ 0, 0, 0, 0 };
    // registers a wave spends on resident fragments: all three terms of its own-h segments, term 0 of the others
    const int nw = mfma_waves(hidden), tpw = hidden / 4 / nw, m = lp_moved_tiles(n_layers, tpw, nw) == 2 ? kLsMoved96 : lp_moved_tiles(n_layers, tpw, nw);
    const int nx = n_layers == 1 ? 0 : ls_segments(tpw, m) - tpw;
    if (tpw * ls_ks2(hidden) * 12 + nx * ls_ks2(hidden) * 4 <= 140) return LsGeo{ nw, tpw, m, nx };
    const int tpw4 = hidden / 16, m4 = n_layers == 2 ? tpw4 / 2 : 0, nx4 = n_layers == 1 ? 0 : ls_segments(tpw4, m4) - tpw4;
    if (n_layers <= 2 && tpw4 * ls_ks2(hidden) * 12 + nx4 * ls_ks2(hidden) * 4 <= 330) return LsGeo{ 4, tpw4, m4, nx4 };
    return LsGeo{ 0, 0, 0, 0 };
}
__host__ __device__ inline size_t ls_lds_floats(int hidden, int n_frames, LsGeo g)
{
    const size_t nP = (size_t)(((n_frames < kLpChunk ? n_frames : kLpChunk) + 3) & ~3);
    return (size_t)kMfmaStreams * nP                          /* xb: audio rows (first and last layer)                     */
         + 2 * 64                                             /* xin[parity][4][n]  (first layer)                          */
         + (size_t)4 * ls_frag_vecs(hidden) * 4               /* below[parity], hT[parity]: B fragments                     */
         + (size_t)2 * hidden * 4                             /* bias rows [unit][4]: own layer, layer above (moved tiles)  */
         + (size_t)((hidden + 1 + 3) & ~3)                    /* Dense weights + bias (last layer)                         */
         + kMfmaStreams                                       /* live flags                                                */
         + 2 * 8 * kMfmaStreams                               /* Dense partial sums [parity][wave][n]                      */
         + (size_t)g.nw * g.nx * ls_ks2(hidden) * 2 * 64 * 4;      /* second- and third-term fragments of the segments nobody waits for */
}
// one frame in the ring: the h fragments, then (M > 0) the started tiles [wave][tile][lane] x 4 gate rows
__host__ __device__ constexpr size_t ls_slot_floats(int hidden, int waves, int m) { return (size_t)ls_frag_vecs(hidden) * 4 + (size_t)waves * m * kWave * 4; }
__host__ __device__ constexpr size_t ls_ring_floats(int hidden, int waves, int m) { return (size_t)kLpRing * ls_slot_floats(hidden, waves, m); }

// acc[tile] += A(segment of the tile) . B for the tiles [TL0, TL1) of one segment kind. The B fragments of one h buffer are read
// into registers ONCE (ls_load_frags: nine 16-byte reads for LSTM-96) and serve every phase of the tick that multiplies with
// that buffer — read one by one between the MFMAs, the three MFMAs of a fragment's first product do not cover its LDS latency
// and the wave stalls once per fragment. Term products grouped by the h term, the large ones first: (w0 w1 w2) h0 | (w0 w1) h1 |
// w0 h2; NPROD = 9: all three weight terms for every h term. `wfrag(tl, ks, term)` supplies the A fragment of a tile;
// `valu(step)` is called behind every MFMA group (the tiles of one product and k-step) with a running index — the caller's
// VALU work that issues in the MFMAs' shadow.
template <int KS2> struct LsFrags { bf16x8 v[3][KS2]; };       // one h buffer's B fragments in registers: [term][k-step]
template <int KS2>
__device__ __forceinline__ void ls_load_frags(LsFrags<KS2>& hb, const u32x4* frags, int lane, int tune = 0)
{
    if (tune & 2097152) {
        // (bit 2097152, test build: ONE 16-byte read instead of 3 KS2 — an upper bound on what fewer LDS bytes per tick could buy
        // (the round-5 review's item 6 a: the eight waves of a CU each read all nine h fragments, 72 KiB per tick); wrong output)
        const bf16x8 v = __builtin_bit_cast(bf16x8, frags[lane]);
#pragma unroll
        for (int th = 0; th < 3; ++th)
#pragma unroll
            for (int ks = 0; ks < KS2; ++ks) hb.v[th][ks] = v;
        return;
    }
#pragma unroll
    for (int th = 0; th < 3; ++th)                          // (term 0 first: it meets the most weight terms and is multiplied first)
#pragma unroll
        for (int ks = 0; ks < KS2; ++ks) hb.v[th][ks] = __builtin_bit_cast(bf16x8, frags[(th * KS2 + ks) * 64 + lane]);
}
template <int KS2, int NPROD, int TL0, int TL1, int NACC, typename WFrag, typename Valu>
__device__ __forceinline__ void ls_gates(f32x4 (&acc)[NACC], const LsFrags<KS2>& hb, WFrag wfrag, Valu valu)
{
    if constexpr (TL0 < TL1) {
        int step = 0;
#pragma unroll
        for (int th = 0; th < 3; ++th) {                    // h term 0, 1, 2: (w0 w1 w2) h0 | (w0 w1) h1 | w0 h2
            const int n_w = NPROD == 9 ? 3 : 3 - th;        // weight terms this h term meets: w0 .. w(n_w - 1)
#pragma unroll
            for (int ks = 0; ks < KS2; ++ks)
#pragma unroll
                for (int tw = 0; tw < n_w; ++tw) {
#pragma unroll
                    for (int tl = TL0; tl < TL1; ++tl)
                        acc[tl] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wfrag(tl, ks, tw), hb.v[th][ks], acc[tl], 0, 0, 0);
                    __builtin_amdgcn_sched_barrier(0);
                    valu(step++);
                    __builtin_amdgcn_sched_barrier(0);
                }
        }
    }
}
// MFMA groups ls_gates issues (= calls of `valu`) per call
__host__ __device__ constexpr int ls_gate_groups(int ks2, int nprod) { return nprod * ks2; }

#ifdef AIDAX_LP_TRACE
// measurement build (scratch/ls_trace.py): the workgroups of stream group (tune >> 16 & 0xff) stamp the shader clock at eight points
// of ticks 96..103 on every wave, straight into the pinned fault buffer: [layer is last][tick][wave][stamp] u64 behind word 16
#define LS_STAMP(k) do { if (grp == ((AIDAX_TUNE(a) >> 16) & 0xff) && tick >= 96 && tick < 104) {                                       \
        __builtin_amdgcn_sched_barrier(0); const unsigned long long t_ = clock64(); __builtin_amdgcn_sched_barrier(0);            \
        if (lane == 0) reinterpret_cast<unsigned long long*>(fault + 16)[(((last ? 1 : 0) * 8 + (tick - 96)) * 4 + (wave & 3)) * 8 + (k)] = t_; } } while (0)
#else
#define LS_STAMP(k) do {} while (0)
#endif

// M: tiles per wave the first layer starts for the layer above / that arrive started; CELL: 0 LSTM, 1 GRU (this layer's)
template <int TPW, int NW, int M, bool FIRST, bool LAST, bool CHAIN, int NPROD, int CELL>
__device__ __forceinline__ void ls_body(const LaunchArgs& a, const MfmaDesc& d, float* ring, uint32_t* counters, uint32_t* fault,
                                        float* smem, int grp, int l)
{
    constexpr int H = 4 * TPW * NW;
    constexpr int NT = NW * kWave;
    constexpr int NS = kMfmaStreams;
    constexpr int KS2 = ls_ks2(H);
    constexpr int kFrag = ls_frag_vecs(H);                  // 16-byte vectors of one h buffer
    constexpr int MW = M;
    constexpr int NSEG = FIRST ? TPW + MW : 2 * TPW - MW;   // resident tile segments of this wave
    constexpr int MA = MW > 0 ? MW : 1;
    constexpr size_t kSlot = ls_slot_floats(H, NW, M);      // floats of one ring frame
    constexpr bool chain = CHAIN, first = FIRST, last = LAST;
    static_assert(!(FIRST && LAST) || M == 0, "a lone layer starts no tiles for a layer above");
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int q = lane >> 4;
    const int n = (int)a.n_frames;
    const int NL = d.n_layers;
    const int Ht = d.hidden_true;
    const int I = a.input_size;
    const int blk = (int)blockIdx.x;
    const int s_base = grp * NS;
    const int chunk = n < kLpChunk ? n : kLpChunk;
    const int nP = (chunk + 3) & ~3;

    float* xb    = smem;                                    // [NS][nP]
    float* xin   = xb + NS * nP;                            // [2][4][NS]
    u32x4* below = reinterpret_cast<u32x4*>(xin + 2 * 64);  // [2][kFrag]  h of the layer below as B fragments
    u32x4* hT    = below + 2 * kFrag;                       // [2][kFrag]  own h(t-1) as B fragments
    float* hS    = reinterpret_cast<float*>(below);         // [H][NS]  h and c as fp32 on their way between the state records and the lanes:
    float* cT    = hS + H * NS;                             // [H][NS]  in `below`, before the first and after the last frame
    float* biasL = reinterpret_cast<float*>(hT + 2 * kFrag);// [H][4] own layer, then [H][4] of the layer above (first layer, MW > 0)
    float* wdl   = biasL + 2 * H * 4;                       // Dense weights, bias at [H]
    float* livef = wdl + ((H + 1 + 3) & ~3);                // [NS]
    float* dpart = livef + NS;                              // [2][NW][NS] Dense partial sums of the waves (last layer)

    const float* W = a.wpack;
    const MfmaLayer& L = d.L[l];

    // ---- per-stream bookkeeping: lanes tid < NS own stream s_base+tid (live flag; PARAM smoothers on the first layer)
    // (ParamRamps, aidax_device.h, by hand: with it k_mfma_ls1 measured 0.3 % slower at 16384 streams, profiles/chain_rules.txt)
    float p_mem[2] = { 0.f, 0.f }, p_tgt[2] = { 0.f, 0.f }, p_step[2] = { 0.f, 0.f };
    uint32_t pending = 0, st_pending0 = 0;
    bool mine_live = false;
    if (tid < NS) {
        const int sg = s_base + tid;
        const bool valid = sg < (int)a.n_streams;
        if (valid) {
            StreamState& st = a.st[sg];
            p_mem[0] = st.p_mem[0]; p_mem[1] = st.p_mem[1];
            p_tgt[0] = st.p_tgt[0]; p_tgt[1] = st.p_tgt[1];
            p_step[0] = st.p_step[0]; p_step[1] = st.p_step[1];
            pending = st_pending0 = st.pending;
            const StreamCtl& ctl = a.ctl[sg];
            const uint32_t flags = ctl.flags;
            mine_live = n != 0 && (flags & CTL_ENABLED) && (flags & CTL_NET_ON);      // :607-619, :631-632
            if (mine_live) {
#pragma unroll
                for (int i = 0; i < 2; ++i) {                // LinearValueSmoother::setTargetValue (:209-216)
                    const float nt = ctl.p_target[i];
                    if (__builtin_fabsf(p_tgt[i] - nt) >= FLT_EPSILON) {
                        p_tgt[i] = nt;
                        p_step[i] = (p_tgt[i] - p_mem[i]) / ctl.p_den;
                    }
                }
                if (pending & PEND_PARAM_FIRST) {            // paramFirstRun (:636-640)
                    pending &= ~PEND_PARAM_FIRST;
                    p_mem[0] = p_tgt[0];
                    p_mem[1] = p_tgt[1];
                }
            }
        }
        livef[tid] = mine_live ? 1.f : 0.f;
    }
    if (last) for (int i = tid; i < H + 1; i += NT) wdl[i] = W[d.wd_off + i];
    for (int i = tid; i < H * 4; i += NT) {
        biasL[i] = W[L.b_off + i];
        if (first && MW > 0) biasL[H * 4 + i] = W[d.L[1].b_off + i];
    }
    // this layer's recurrent state -> LDS as fp32; the fragment buffers start from zero (padded k-steps stay zero for good)
    for (int i = tid; i < H * NS; i += NT) {
        const int u = i / NS, sn = i % NS, sg = s_base + sn;
        const bool valid = sg < (int)a.n_streams;
        const float* stp = a.nn + (size_t)(valid ? sg : 0) * a.nn_stride + L.state_off;
        hS[i] = (valid && u < Ht) ? stp[u] : 0.f;           // padded units rest at 0
        cT[i] = (valid && u < Ht && L.cell == 0) ? stp[Ht + u] : 0.f;
    }
    for (int i = tid; i < 2 * kFrag; i += NT) hT[i] = u32x4{ 0u, 0u, 0u, 0u };

    // ---- resident fragments. The TPW own-h segments (every tick's critical path): all three terms in registers. The NX
    // others — the input half of the tiles started for the layer above (first layer) / of the tiles that start here (others),
    // MFMAs nobody waits for — keep term 0 in registers and terms 1 and 2 (three of the six products) in LDS, each wave its own.
    constexpr int NX = NSEG - TPW;
    constexpr int NXA = NX > 0 ? NX : 1;
    bf16x8 wq[TPW][KS2][3];
    bf16x8 wx[NXA][KS2];
    u32x4* w2x = reinterpret_cast<u32x4*>(dpart + 2 * 8 * NS) + (size_t)wave * NXA * KS2 * 2 * 64 + lane;      // [x][ks][term - 1] at stride 64
    {
        // the ls record: layer 0 holds one segment per tile (own h), the others two (h below | own h)
        const size_t per_seg = (size_t)KS2 * 3 * kWave;                     // u32x4 per (tile, segment)
        const u32x4* rec = reinterpret_cast<const u32x4*>(W + d.ls_off);
        auto seg_ptr = [&](int ll, int tl, int seg_in_rec) {
            return rec + (ll == 0 ? 0 : (size_t)NW * TPW * per_seg * (size_t)(1 + 2 * (ll - 1)))
                       + ((size_t)(wave * TPW + tl) * (ll == 0 ? 1 : 2) + seg_in_rec) * per_seg + lane;
        };
#pragma unroll
        for (int tl = 0; tl < TPW; ++tl) {                                  // own h(t-1)
            const u32x4* sp = seg_ptr(l, tl, first ? 0 : 1);
#pragma unroll
            for (int ks = 0; ks < KS2; ++ks)
#pragma unroll
                for (int t = 0; t < 3; ++t) wq[tl][ks][t] = __builtin_bit_cast(bf16x8, sp[(ks * 3 + t) * kWave]);
        }
#pragma unroll
        for (int x = 0; x < NX; ++x) {
            // first layer: the layer above's input half of the tiles this wave starts; others: h below, for the tiles that start here
            const u32x4* sp = first ? seg_ptr(1, x, 0) : seg_ptr(l, MW + x, 0);
#pragma unroll
            for (int ks = 0; ks < KS2; ++ks) {
                wx[x][ks] = __builtin_bit_cast(bf16x8, sp[(ks * 3 + 0) * kWave]);
                w2x[((x * KS2 + ks) * 2 + 0) * 64] = sp[(ks * 3 + 1) * kWave];
                w2x[((x * KS2 + ks) * 2 + 1) * 64] = sp[(ks * 3 + 2) * kWave];
            }
        }
    }
    float w_in0[TPW];                                       // (pack_mfma lays the input k-step out by ITS waves and tiles: d.waves x d.tpw)
#pragma unroll
    for (int tl = 0; tl < TPW; ++tl) {
        const int T = wave * TPW + tl;
        w_in0[tl] = first ? W[d.L[0].w_in_off + ((size_t)(T / d.tpw) * kWave + lane) * d.tpw + T % d.tpw] : 0.f;
    }
    float wdu[TPW];                                         // Dense weights of this lane's units (last layer)
#pragma unroll
    for (int tl = 0; tl < TPW; ++tl) wdu[tl] = last ? W[d.wd_off + 4 * (wave * TPW + tl) + q] : 0.f;

    // ---- ring bookkeeping (k_mfma_lp's): counters count frames since the buffers were allocated and are equal on both sides
    // between launches, so a workgroup starts from its own side's value
    const size_t ring_stride = ls_ring_floats(H, NW, M);
    float* ring_out = last ? nullptr : ring + ((size_t)grp * (NL - 1) + l) * ring_stride;
    const float* ring_in = first ? nullptr : ring + ((size_t)grp * (NL - 1) + (l - 1)) * ring_stride;
    const size_t ring_bytes = ring_stride * sizeof(float);
    const __amdgpu_buffer_rsrc_t rs_out = lp_rsrc(last ? ring : ring_out, ring_bytes);
    const __amdgpu_buffer_rsrc_t rs_in = lp_rsrc(first ? ring : ring_in, ring_bytes);
    uint32_t* cnt_out = last ? nullptr : counters + ((size_t)grp * (NL - 1) + l) * kLpCounterStride;
    uint32_t* cnt_in = first ? nullptr : counters + ((size_t)grp * (NL - 1) + (l - 1)) * kLpCounterStride;
    auto give_up = [&]() { __hip_atomic_fetch_add(fault, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM); };
    if ((AIDAX_TUNE(a) & 16) && blk == 0 && tid == 0) give_up();      // test hook: report a give-up that did not happen
    const uint32_t base_out = cnt_out ? __hip_atomic_load(cnt_out, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0u;
    const uint32_t base_in = cnt_in ? __hip_atomic_load(cnt_in + 16, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0u;
    uint32_t known_free = kLpRing;                         // frames of this launch the ring above is known to have room for
    uint32_t known_below = 0;                              // frames of this launch known to exist below
    __syncthreads();

    // ---- this lane's (unit, stream) pairs — one per tile: h and c in registers for the launch
    float hv[TPW], creg[TPW];
#pragma unroll
    for (int tl = 0; tl < TPW; ++tl) {
        hv[tl] = hS[(wave * TPW + tl) * 64 + lane];         // unit 4T + q, stream lane & 15
        creg[tl] = cT[(wave * TPW + tl) * 64 + lane];
    }
    __syncthreads();                                        // (the staging area becomes `below`)
    for (int i = tid; i < 2 * kFrag; i += NT) below[i] = u32x4{ 0u, 0u, 0u, 0u };
    // where a lane's h values go in the fragments: unit u = 4T + q -> k-step u / 32, lane row (u % 32) / 8, element u % 8
    auto publish_tile = [&](u32x4* dst, int tl) {
        const int u = 4 * (wave * TPW + tl) + q;
        uint16_t* p16 = reinterpret_cast<uint16_t*>(dst + (u >> 5) * 64 + ((u & 31) >> 3) * 16 + (lane & 15)) + (u & 7);
        float r = hv[tl];
#pragma unroll
        for (int t = 0; t < 3; ++t) {
            const __bf16 b = static_cast<__bf16>(r);         // round to nearest even
            p16[(size_t)t * KS2 * 64 * 8] = __builtin_bit_cast(uint16_t, b);
            if (t < 2) r -= static_cast<float>(b);           // exact
        }
    };
#pragma unroll
    for (int tl = 0; tl < TPW; ++tl) publish_tile(hT, tl);
    __syncthreads();

    // ---- the cell update of one tile in steps of three to five instructions, so that it can be dealt out behind the MFMA
    // groups of the NEXT tiles (bf16 MFMAs leave the VALU free while they run). Same operations in the same order as
    // sigmoid_pre / tanh_rat / tanh_exp_pre; the last step splits the new h and writes its fragments.
    // (What each part adds to the cfg5 launch of 720 us, from builds with the part switched off and wrong results: cell update 90, ring
    // stores 93, MFMAs 80, split + fragment writes 61, LDS-resident weight terms read at use 40 — profiles/r04_ls_parts8.txt.)
    struct CellTmp { float e0, e1, e2, x, u, p, qq, gg; };
    constexpr int NSTEP = CELL == 0 ? 12 : 5;
    CellTmp ct[TPW];
    auto cell_step = [&](int tl, int k, const f32x4& g, u32x4* h_dst) {
        CellTmp& t = ct[tl];
        if constexpr (CELL == 0) {                          // LSTM: g = (i, f, g, o), the sigmoid rows carrying -log2 e
            switch (k) {
            case 0: t.x = tanh_rat_clamp(g.z); t.u = t.x * t.x; t.e0 = __builtin_amdgcn_exp2f(g.x); break;
            case 1: t.p = __builtin_fmaf(kTanhP[6], t.u, kTanhP[5]); t.p = __builtin_fmaf(t.p, t.u, kTanhP[4]); t.e1 = __builtin_amdgcn_exp2f(g.y); break;
            case 2: t.p = __builtin_fmaf(t.p, t.u, kTanhP[3]); t.p = __builtin_fmaf(t.p, t.u, kTanhP[2]); t.e2 = __builtin_amdgcn_exp2f(g.w); break;
            case 3: t.p = __builtin_fmaf(t.p, t.u, kTanhP[1]); t.p = __builtin_fmaf(t.p, t.u, kTanhP[0]); t.qq = __builtin_fmaf(kTanhQ[3], t.u, kTanhQ[2]); break;
            case 4: t.qq = __builtin_fmaf(t.qq, t.u, kTanhQ[1]); t.qq = __builtin_fmaf(t.qq, t.u, kTanhQ[0]); t.e0 = __builtin_amdgcn_rcpf(1.0f + t.e0); break;      // i
            case 5: t.gg = (t.p * t.x) * __builtin_amdgcn_rcpf(t.qq); t.e1 = __builtin_amdgcn_rcpf(1.0f + t.e1); break;                                                // tanh(g), f
            case 6: creg[tl] = __builtin_fmaf(t.e1, creg[tl], t.e0 * t.gg); t.x = tanh_rat_clamp(creg[tl]); break;
            case 7: t.u = t.x * t.x; t.p = __builtin_fmaf(kTanhP[6], t.u, kTanhP[5]); t.p = __builtin_fmaf(t.p, t.u, kTanhP[4]); t.e2 = __builtin_amdgcn_rcpf(1.0f + t.e2); break;   // o
            case 8: t.p = __builtin_fmaf(t.p, t.u, kTanhP[3]); t.p = __builtin_fmaf(t.p, t.u, kTanhP[2]); t.p = __builtin_fmaf(t.p, t.u, kTanhP[1]); break;
            case 9: t.p = __builtin_fmaf(t.p, t.u, kTanhP[0]); t.qq = __builtin_fmaf(kTanhQ[3], t.u, kTanhQ[2]); t.qq = __builtin_fmaf(t.qq, t.u, kTanhQ[1]); t.qq = __builtin_fmaf(t.qq, t.u, kTanhQ[0]); break;
            case 10: hv[tl] = t.e2 * ((t.p * t.x) * __builtin_amdgcn_rcpf(t.qq)); break;
            case 11: publish_tile(h_dst, tl); break;
            default: break;
            }
        } else {                                            // GRU: g = (z, r, candidate's recurrent half, its input half)
            switch (k) {
            case 0: t.e0 = __builtin_amdgcn_exp2f(g.x); t.e1 = __builtin_amdgcn_exp2f(g.y); break;
            case 1: t.e0 = __builtin_amdgcn_rcpf(1.0f + t.e0); t.e1 = __builtin_amdgcn_rcpf(1.0f + t.e1); break;
            case 2: t.e2 = __builtin_amdgcn_exp2f(__builtin_fmaf(t.e1, g.z, g.w)); break;                  // (the candidate rows carry 2 log2 e: tanh_exp_pre)
            case 3: t.x = __builtin_fmaf(-2.0f, __builtin_amdgcn_rcpf(1.0f + t.e2), 1.0f); hv[tl] = __builtin_fmaf(t.e0, hv[tl] - t.x, t.x); break;
            case 4: publish_tile(h_dst, tl); break;
            default: break;
            }
        }
    };

    // A frame goes up the ring in two parts: its h fragments one tick after it was computed (16-byte write-through stores out
    // of LDS), the tiles started for the layer above another tick later — they are computed at the END of a tick (the MFMAs
    // whose shadow the cell update issues in) and leave at the head of the next one, so that every store has a whole tick to
    // drain before the barrier that precedes its publication.
    auto ship_h = [&](const u32x4* h_src, int Fprev) {
        const uint32_t slot_off = (uint32_t)(((base_out + (uint32_t)Fprev) % kLpRing) * kSlot * sizeof(float));
        for (int i = tid; i < kFrag; i += NT) lp_store16(rs_out, slot_off + (uint32_t)i * 16u, __builtin_bit_cast(f32x4, h_src[i]));
    };
    auto ship_started = [&](const f32x4 (&pacc)[MA], int Fprev) {
        const uint32_t slot_off = (uint32_t)(((base_out + (uint32_t)Fprev) % kLpRing) * kSlot * sizeof(float));
#pragma unroll
        for (int tl = 0; tl < MW; ++tl)
            lp_store16(rs_out, slot_off + (uint32_t)(kFrag * 16) + (uint32_t)(((wave * M + tl) * kWave + lane) * 16), pacc[tl]);
    };
    auto no_valu = [](int) {};
    auto own_w = [&](int tl, int ks, int tw) -> bf16x8 { return wq[tl][ks][tw]; };
    // the segments nobody waits for: x = tile (first layer: the tiles started for the layer above) / tile - MW (others)
    auto x_w = [&](int x, int ks, int tw) -> bf16x8 { return tw == 0 ? wx[x][ks] : __builtin_bit_cast(bf16x8, w2x[((x * KS2 + ks) * 2 + tw - 1) * 64]); };
    auto up_w = [&](int tl, int ks, int tw) -> bf16x8 { return x_w(tl, ks, tw); };
    auto below_w = [&](int tl, int ks, int tw) -> bf16x8 { return x_w(tl - MW, ks, tw); };
    auto bias_of = [&](int tl, bool above) { return *reinterpret_cast<const f32x4*>(biasL + (above ? H * 4 : 0) + 4 * (4 * (wave * TPW + tl) + q)); };

    constexpr int HALF = (TPW + 1) / 2;                    // tiles of the first own-h phase
    constexpr int G = ls_gate_groups(KS2, NPROD);          // MFMA groups of one ls_gates call
    f32x4 held[MA] = {};                                   // first layer: the started tiles of the frame before last, on their way out
    int par = 0;                                           // parity of hT the next frame reads
    int done = 0;                                          // frames finished before this chunk
    for (int base = 0; base < n; base += kLpChunk) {
        const int cnt = n - base < kLpChunk ? n - base : kLpChunk;
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
            if (tid == 0) wait_below(done + 3);
            __syncthreads();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        }
        if (first || last) {
            for (int sl = wave; sl < NS; sl += NW) {
                const int sg = s_base + sl;
                const bool lv = livef[sl] != 0.f;
                float* row = xb + sl * nP;
                if (lv) {
                    const float* src = a.out + (size_t)sg * n + base;
                    if (((n | base) & 3) == 0) load_block(row, src, cnt, lane);
                    else for (int t = lane; t < cnt; t += kWave) row[t] = src[t];
                } else {
                    for (int t = lane; t < cnt; t += kWave) row[t] = 0.f;
                }
            }
        }
        __syncthreads();
        auto write_xin = [&](int parity, int f) {
            // lanes tid < NS: x * in_gain, PARAM1, PARAM2 of frame `f` (:171-181, :195-231)
            float q1 = 0.f, q2 = 0.f;
            if (I >= 2) q1 = lin_next(p_mem[0], p_tgt[0], p_step[0]);
            if (I >= 3) q2 = lin_next(p_mem[1], p_tgt[1], p_step[1]);
            float* col = xin + parity * 64;
            col[tid] = xb[tid * nP + f] * a.in_gain;
            col[NS + tid] = q1;
            col[2 * NS + tid] = q2;
            col[3 * NS + tid] = 0.f;
        };
        constexpr int PER4 = (kFrag + NT - 1) / NT;        // 16-byte vectors of a frame each thread moves
        f32x4 pre[PER4];
        f32x4 upx[MA] = {};                                // started tiles on their way in (layers >= 1): fetched in one tick, the accumulators' start in the next
        constexpr int NB = TPW - MW > 0 ? TPW - MW : 1;
        f32x4 nacc[NB] = {};                               // layers >= 1: bias + input half of the tiles that start here, for the NEXT frame
        auto fetch_frags = [&](int F) {                    // all threads: the h fragments of frame F of the launch -> registers
            const uint32_t slot_off = (uint32_t)(((base_in + (uint32_t)F) % kLpRing) * kSlot * sizeof(float));
#pragma unroll
            for (int k = 0; k < PER4; ++k)
                if (k * NT + tid < kFrag) pre[k] = lp_load16(rs_in, slot_off + (uint32_t)(k * NT + tid) * 16u);
        };
        auto fetch_started = [&](int F) {                  // ... and this wave's started tiles of frame F
            const uint32_t slot_off = (uint32_t)(((base_in + (uint32_t)F) % kLpRing) * kSlot * sizeof(float));
#pragma unroll
            for (int tl = 0; tl < MW; ++tl)
                upx[tl] = lp_load16(rs_in, slot_off + (uint32_t)(kFrag * 16) + (uint32_t)(((wave * M + tl) * kWave + lane) * 16));
        };
        auto stash_below = [&](int parity) {
#pragma unroll
            for (int k = 0; k < PER4; ++k)
                if (k * NT + tid < kFrag) below[parity * kFrag + k * NT + tid] = __builtin_bit_cast(u32x4, pre[k]);
        };
        // the input half of the tiles that start here, for the frame whose fragments sit in below[parity]
        auto start_next = [&](int parity, auto valu) {
            f32x4 z[TPW];
#pragma unroll
            for (int tl = MW; tl < TPW; ++tl) z[tl] = bias_of(tl, false);
            LsFrags<KS2> hbn;
            ls_load_frags(hbn, below + parity * kFrag, lane, AIDAX_TUNE(a));
            ls_gates<KS2, NPROD, MW, TPW, TPW>(z, hbn, below_w, valu);
#pragma unroll
            for (int tl = MW; tl < TPW; ++tl) nacc[tl - MW] = z[tl];
        };

        if (first) {
            if (tid < NS) write_xin(0, 0);
        } else {
            // frames 0 and 1 of the chunk into both halves of `below`, frame 0's started tiles, frame 2 for tick 0's prefetch
            if (tid == 0) wait_below(done + 3);
            __syncthreads();
            fetch_frags(done);
            fetch_started(done);
            stash_below(0);
            if (cnt > 1) { fetch_frags(done + 1); stash_below(1); }
        }
        __syncthreads();
        if constexpr (!first && MW < TPW) start_next(0, no_valu);

        const int ticks = last ? cnt + 2 : cnt;            // the Dense of a frame: partial sums one tick behind its h, the output two
        for (int tick = 0; tick < ticks; ++tick) {
            const int rd = par, wr = par ^ 1;
            const bool body = tick < cnt;
            const bool more = tick + 1 < cnt;              // another frame of this chunk follows
            const bool more2 = tick + 2 < cnt;
            const int F = done + tick;                     // frame of the launch this tick computes
            LS_STAMP(0);
            f32x4 acc[TPW];
            if (first) {
                if (tid < NS && more) write_xin((tick + 1) & 1, tick + 1);
            } else {
                // bias + input half: the tiles that arrived started (fetched a tick ago) / the ones started here last tick
#pragma unroll
                for (int tl = 0; tl < TPW; ++tl) acc[tl] = tl < MW ? upx[tl < MW ? tl : 0] : nacc[tl < MW ? 0 : tl - MW];
                if (more) fetch_started(F + 1);
                if (more2) fetch_frags(F + 2);
            }
            if (body && tid == 0) {
                // thread 0 looks ahead while the others compute (see k_mfma_lp): what the NEXT tick fetches must exist below,
                // the slot the next tick stores into must be free above
                if (!first && tick + 3 < cnt) wait_below(F + 4);
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
            // (a lone layer: the tick's fragment reads are requested before the Dense, whose 340 cycles then pass while they arrive —
            // 48 KiB for the eight waves of LSTM-64, 384 cycles of the LDS port; the stacked roles have no registers to spare for that)
            constexpr bool early_frags = first && last;
            LsFrags<KS2> hb;                                // own h(t-1)
            if constexpr (early_frags) { if (body) ls_load_frags(hb, hT + rd * kFrag, lane, AIDAX_TUNE(a)); }
            // ---- Dense(H,1) of frame tick-1 from the lanes' own h(tick-1): this wave's units, summed in a fixed order
            if (last && tick >= 1 && tick <= cnt) {
                float y = wdu[0] * hv[0];
#pragma unroll
                for (int tl = 1; tl < TPW; ++tl) y = __builtin_fmaf(wdu[tl], hv[tl], y);
                const Pair r2 = share_rows(y);
                y = r2.lo + r2.hi;
                const Pair r4 = share_halves(y);
                y = r4.lo + r4.hi;
                if (lane < NS) dpart[((tick & 1) * NW + wave) * NS + lane] = y;
            }
            // ---- ... and of frame tick-2: the NW partial sums, bias, skip, output gain (wave 0, one lane per stream)
            if (last && tick >= 2 && wave == (early_frags && NW > 1 ? 1 : 0) && lane < NS) {      // (lone layer: not on the wave that writes the model inputs)
                const int fd = tick - 2;
                float y = wdl[H];
#pragma unroll
                for (int w = 0; w < NW; ++w) y += dpart[(((tick - 1) & 1) * NW + w) * NS + lane];
                const float x = xb[lane * nP + fd] * a.in_gain;
                float o = a.input_skip ? x + y : y;
                o = o * a.out_gain;
                if (livef[lane] != 0.f) xb[lane * nP + fd] = o;
            }

            LS_STAMP(1);
            if (body) {
                const u32x4* h_rd = hT + rd * kFrag;
                u32x4* h_wr = hT + wr * kFrag;
                if constexpr (!early_frags) ls_load_frags(hb, h_rd, lane, AIDAX_TUNE(a));      // requested first, on its way while the frame before goes up the ring
                if (!last && F >= 1) ship_h(h_rd, F - 1);              // h_rd = h(F-1)
                if constexpr (first) {
                    if (MW > 0 && F >= 2) ship_started(held, F - 2);
#pragma unroll
                    for (int tl = 0; tl < TPW; ++tl) acc[tl] = bias_of(tl, false);
                    const float b = xin[(tick & 1) * 64 + lane];      // the model inputs: one fp32 k-step (x, PARAM1, PARAM2, 0)
#pragma unroll
                    for (int tl = 0; tl < TPW; ++tl)
                        acc[tl] = __builtin_amdgcn_mfma_f32_16x16x4f32(w_in0[tl], b, acc[tl], 0, 0, 0);
                }
                // the cell steps of the tiles [T0, T1), dealt out over the G groups of a phase (the tiles advance together; one tile's
                // update after the other has eight temporaries fewer and less to overlap — tried, no result recorded)
                auto deal = [&](int T0, int T1, int g) {
                    const int nt = T1 - T0, S = nt * NSTEP;
#pragma unroll
                    for (int sidx = g * S / G; sidx < (g + 1) * S / G; ++sidx)
                        cell_step(T0 + sidx % nt, sidx / nt, acc[T0 + sidx % nt], h_wr);
                };
                // phase A: own h(t-1) against the first half of the tiles
                LS_STAMP(2);
                ls_gates<KS2, NPROD, 0, HALF, TPW>(acc, hb, own_w, no_valu);
                LS_STAMP(3);
                if constexpr (!first) {
                    // frame F+2's fragments (requested at the head of the tick) go where frame F's were: their product was taken
                    // a tick ago, and the registers they travelled in are free for the phases below. (At the END of the tick
                    // the load has the whole tick to arrive: measured the same for LSTM-96 x 2, 712.5 against 713.3 us
                    // — profiles/r04_ls_parts8.txt — and 3 % slower for LSTM-64 x 2.)
                    if (more2) stash_below(tick & 1);
                }
                // phase B: ... the second half, the first half's cell update in its shadow
                if constexpr (HALF < TPW) ls_gates<KS2, NPROD, HALF, TPW, TPW>(acc, hb, own_w, [&](int g) { deal(0, HALF, g); });
                else {
#pragma unroll
                    for (int g = 0; g < G; ++g) deal(0, HALF, g);
                }
                LS_STAMP(4);
                // phase C: MFMAs nobody waits for — the tiles started for the layer above (first layer) / the input half of the
                // next frame (others) — with the second half's cell update in their shadow
                bool c_done = false;
                if constexpr (first) {
                    if constexpr (MW > 0) {
                        if (F >= 1) {
                            f32x4 pacc[MA];
#pragma unroll
                            for (int tl = 0; tl < MW; ++tl) pacc[tl] = bias_of(tl, true);
                            ls_gates<KS2, NPROD, 0, MW, MA>(pacc, hb, up_w, [&](int g) { if constexpr (HALF < TPW) deal(HALF, TPW, g); });
#pragma unroll
                            for (int tl = 0; tl < MA; ++tl) held[tl] = pacc[tl];
                            c_done = true;
                        }
                    }
                } else if constexpr (MW < TPW) {
                    if (more) {
                        start_next((tick + 1) & 1, [&](int g) { if constexpr (HALF < TPW) deal(HALF, TPW, g); });
                        c_done = true;
                    }
                }
                if (!c_done) {
                    if constexpr (HALF < TPW) {
#pragma unroll
                        for (int g = 0; g < G; ++g) deal(HALF, TPW, g);
                    }
                }
                LS_STAMP(5);
                par = wr;
                if (!last) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");     // this wave's ring stores (issued at the head of the tick) have left before the barrier (G16)
                LS_STAMP(6);
            }
            __syncthreads();                               // h(t) in LDS, the next frames' input in LDS, ring stores of this tick done
            LS_STAMP(7);
            // ---- counters, by thread 0 after the barrier: every kLpBatch frames and at the end of the launch
            if (body && tid == 0) {
                if (!last) {
                    // complete in the ring: frames whose h left by the last tick and whose started tiles left in this one
                    const int produced = first && MW > 0 ? F - 1 : F;
                    if (produced > 0 && produced % kLpBatch == 0)
                        __hip_atomic_store(cnt_out, base_out + (uint32_t)produced, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                }
                if (!first) {
                    const int consumed = more ? F + 2 : F + 1;             // frames read out of the ring so far (fragments AND started tiles)
                    if (consumed % kLpBatch == 0 || consumed == n)
                        __hip_atomic_store(cnt_in + 16, base_in + (uint32_t)consumed, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                }
            }
        }
        done += cnt;
        // ---- results of this chunk back to HBM (last layer)
        if (last) {
            for (int sl = wave; sl < NS; sl += NW) {
                const int sg = s_base + sl;
                if (livef[sl] == 0.f) continue;
                float* dst = a.out + (size_t)sg * n + base;
                const float* row = xb + sl * nP;
                if (((n | base) & 3) == 0) store_block(dst, row, cnt, lane);
                else for (int t = lane; t < cnt; t += kWave) dst[t] = row[t];
            }
        }
        __syncthreads();
    }

    if (!last && n > 0) {                                  // the launch's last frame (and the started tiles still held), then the final count
        ship_h(hT + par * kFrag, n - 1);
        if constexpr (first && MW > 0) {
            if (n >= 2) ship_started(held, n - 2);
            f32x4 pacc[MA];
#pragma unroll
            for (int tl = 0; tl < MW; ++tl) pacc[tl] = bias_of(tl, true);
            LsFrags<KS2> hbl;
            ls_load_frags(hbl, hT + par * kFrag, lane);
            ls_gates<KS2, NPROD, 0, MW, MA>(pacc, hbl, up_w, no_valu);
            ship_started(pacc, n - 1);
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if (tid == 0) __hip_atomic_store(cnt_out, base_out + (uint32_t)n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }

    // ---- recurrent state and smoother memories back to HBM for the streams that ran
#pragma unroll
    for (int tl = 0; tl < TPW; ++tl) {
        hS[(wave * TPW + tl) * 64 + lane] = hv[tl];
        cT[(wave * TPW + tl) * 64 + lane] = creg[tl];
    }
    __syncthreads();
    for (int i = tid; i < H * NS; i += NT) {
        const int u = i / NS, sn = i % NS, sg = s_base + sn;
        if (sg < (int)a.n_streams && u < Ht && livef[sn] != 0.f) {
            float* stp = a.nn + (size_t)sg * a.nn_stride + L.state_off;
            stp[u] = hS[i];
            if (L.cell == 0) stp[Ht + u] = cT[i];
        }
    }
    if (first && tid < NS && mine_live) {
        StreamState& st = a.st[s_base + tid];
        st.p_mem[0] = p_mem[0]; st.p_mem[1] = p_mem[1];
        st.p_tgt[0] = p_tgt[0]; st.p_tgt[1] = p_tgt[1];
        st.p_step[0] = p_step[0]; st.p_step[1] = p_step[1];
        if (!chain) st.pending = pending;
        else if (pending != st_pending0)                  // (the last layer's workgroup clears PEND_ACTIVATE in the same word)
            __hip_atomic_fetch_and(&st.pending, ~(uint32_t)PEND_PARAM_FIRST, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

template <int TPW, int NW, int M, bool CHAIN, int NPROD>
__global__ __launch_bounds__(NW * kWave) void k_mfma_ls(LaunchArgs a, MfmaDesc d, float* ring, uint32_t* counters, uint32_t* fault)
{
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int NL = d.n_layers;
    const int blk = (int)blockIdx.x;
    const bool adjacent = (AIDAX_TUNE(a) & 2) != 0;
    const int grp = adjacent ? blk / NL : (blk / (8 * NL)) * 8 + (blk & 7);
    const int l = adjacent ? blk % NL : (blk / 8) % NL;
    const int n_groups = ((int)a.n_streams + kMfmaStreams - 1) / kMfmaStreams;
    if (grp >= n_groups) return;
    // (measurement, AIDAX_TUNE bit 4096: where this workgroup ran and when — XCC_ID, HW_ID, the 100 MHz clock at its start and end — into
    // the pool's pinned fault page behind the fault word; scratch/r05_modes.py reads it)
    const bool stamp = (AIDAX_TUNE(a) & 4096) && blk < 500 && threadIdx.x == 0;
    if (stamp) {
        fault[16 + 3 * blk] = (__builtin_amdgcn_s_getreg((31 << 11) | 20) & 15u) | (__builtin_amdgcn_s_getreg((31 << 11) | 4) << 4);
        fault[17 + 3 * blk] = (uint32_t)wall_clock64();
    }
    if (l == 0) {
        if constexpr (CHAIN) {
            lp_chain_rows<true>(a, smem, grp, true);
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        }
        if (d.L[l].cell == 0) ls_body<TPW, NW, M, true, false, CHAIN, NPROD, 0>(a, d, ring, counters, fault, smem, grp, l);
        else ls_body<TPW, NW, M, true, false, CHAIN, NPROD, 1>(a, d, ring, counters, fault, smem, grp, l);
    } else if (l == NL - 1) {
        if constexpr (CHAIN) {
            if (AIDAX_TUNE(a) & 8192) {                                          // test hook: this workgroup starts 100 us late
                const uint64_t t0 = wall_clock64();
                while (wall_clock64() - t0 < 10000) __builtin_amdgcn_s_sleep(64);
            }
        }
        if (d.L[l].cell == 0) ls_body<TPW, NW, M, false, true, CHAIN, NPROD, 0>(a, d, ring, counters, fault, smem, grp, l);
        else ls_body<TPW, NW, M, false, true, CHAIN, NPROD, 1>(a, d, ring, counters, fault, smem, grp, l);
        if constexpr (CHAIN) {
            __syncthreads();
            lp_chain_rows<false>(a, smem, grp, true);
        }
    } else {
        if (d.L[l].cell == 0) ls_body<TPW, NW, M, false, false, CHAIN, NPROD, 0>(a, d, ring, counters, fault, smem, grp, l);
        else ls_body<TPW, NW, M, false, false, CHAIN, NPROD, 1>(a, d, ring, counters, fault, smem, grp, l);
    }
    if (stamp) fault[18 + 3 * blk] = (uint32_t)wall_clock64();
}

// A LONE layer on the same body (first and last role at once: no ring, nobody waits, a workgroup per 16 streams): the one-layer
// models of the reference's table at stream counts where a matrix-core form pays — LSTM-64 / 80, GRU-80, ... (GRU-40 / 64 have
// k_gru_gs). CHAIN: the DSP chain passes on waves 0 and 1 around the body, the whole run() in the launch.
template <int TPW, int NW, bool CHAIN, int NPROD>
__global__ __launch_bounds__(NW * kWave) void k_mfma_ls1(LaunchArgs a, MfmaDesc d, float* ring, uint32_t* counters, uint32_t* fault)
{
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int grp = (int)blockIdx.x;
    if constexpr (CHAIN) {
        lp_chain_rows<true>(a, smem, grp, true);
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    }
    if (d.L[0].cell == 0) ls_body<TPW, NW, 0, true, true, CHAIN, NPROD, 0>(a, d, ring, counters, fault, smem, grp, 0);
    else ls_body<TPW, NW, 0, true, true, CHAIN, NPROD, 1>(a, d, ring, counters, fault, smem, grp, 0);
    if constexpr (CHAIN) {
        __syncthreads();
        lp_chain_rows<false>(a, smem, grp, true);
    }
}

// k_mfma_ls: the stacked models k_mfma_lp serves whose resident split fragments fit the register file (ls_geo)
template <int HID, int NL>
static LpFn ls_fn_for(bool chain, int nprod)
{
    constexpr LsGeo g = ls_geo(NL, HID);
    if constexpr (g.nw == 0) return nullptr;
    else if constexpr (NL == 1) {
        if constexpr (g.tpw * ls_ks2(HID) * 12 > 150) return chain ? k_mfma_ls1<g.tpw, g.nw, true, 6> : k_mfma_ls1<g.tpw, g.nw, false, 6>;
        else return chain ? (nprod == 9 ? k_mfma_ls1<g.tpw, g.nw, true, 9> : k_mfma_ls1<g.tpw, g.nw, true, 6>)
                          : (nprod == 9 ? k_mfma_ls1<g.tpw, g.nw, false, 9> : k_mfma_ls1<g.tpw, g.nw, false, 6>);
    }
    else if constexpr ((g.tpw + g.nx) * ls_ks2(HID) * 12 > 150)      // the 512-register geometries: six products only (nine spill)
        return chain ? k_mfma_ls<g.tpw, g.nw, g.m, true, 6> : k_mfma_ls<g.tpw, g.nw, g.m, false, 6>;
    else return chain ? (nprod == 9 ? k_mfma_ls<g.tpw, g.nw, g.m, true, 9> : k_mfma_ls<g.tpw, g.nw, g.m, true, 6>)
                      : (nprod == 9 ? k_mfma_ls<g.tpw, g.nw, g.m, false, 9> : k_mfma_ls<g.tpw, g.nw, g.m, false, 6>);
}
LpFn ls_fn_two_layers(int hidden, bool chain, int nprod);      // (an object of its own: aidax_mfmals2.hip)

}  // namespace aidax
