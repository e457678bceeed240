// aidax_tick.hip — the tick kernels k_gru_gm, k_gru_gs and k_lstm_gs: one-layer models, the whole run() in one launch.
//
// One design: k_gru_gs and k_lstm_gs are cells of one frame; k_gru_gm, their fp32 partner, follows the same protocol in a loop of its own. A workgroup serves 16 streams. A MAIN wave owns 16 units: their weights stay in its registers for the
// launch, and so do h(t-1) (and c) of its lane's four units (16 wave + 4q + e) of stream c = lane & 15. NHELP HELPER waves
// (lp_helper, aidax_lp_device.h) carry the DSP chain, the model inputs of the next frame and the Dense's tail. A frame is one tick
// of a loop paced by one __syncthreads; the main waves publish h(t) in LDS for each other's products of the next tick.
//   tick_frame   what the kernels share: the indices, the LDS carve-up, the hand-off to lp_helper, the staging of the audio rows, the
//                barrier protocol, the Dense window and the state write-back.
//   the cells    what a main wave holds and does in a tick (GruGs, LstmGs): load the record, load and publish h(t-1), one
//                frame's products, cell update and h(t) into LDS, the Dense steps.
#include "aidax_lp_device.h"

namespace aidax {

// ---------------------------------------------------------------- LDS of a workgroup
// xb [NS][nP] audio rows | xin [2][4][NS] model inputs of a frame | h: the cell's h(t-1), two parities (Cell::kHFloats) |
// wdl: Dense weights, bias at [H] | livef [NS] | dpart [2][8][NS] Dense partial sums of the waves | hands: the helpers' hand-over slots
struct TickLds { float *xb, *xin, *h, *wdl, *livef, *dpart, *hands; };
__host__ __device__ inline size_t tick_lds_floats(int hidden, int n_frames, int n_helpers, size_t h_floats)
{
    const size_t nP = (size_t)(((n_frames < kLpChunk ? n_frames : kLpChunk) + 3) & ~3);
    return (size_t)kMfmaStreams * nP + 2 * 64 + h_floats + (size_t)((hidden + 1 + 3) & ~3) + kMfmaStreams
         + 2 * 8 * kMfmaStreams + (size_t)n_helpers * 2 * kChainHandFloats
#ifdef AIDAX_LP_TRACE
         + 2048                                             /* time stamps of eight ticks, every wave (scratch/gs_trace.py) */
#endif
         ;
}
__device__ __forceinline__ TickLds tick_lds(float* smem, int hidden, int nP, int h_floats)
{
    TickLds m;
    m.xb    = smem;
    m.xin   = m.xb + kMfmaStreams * nP;
    m.h     = m.xin + 2 * 64;
    m.wdl   = m.h + h_floats;
    m.livef = m.wdl + ((hidden + 1 + 3) & ~3);
    m.dpart = m.livef + kMfmaStreams;
    m.hands = m.dpart + 2 * 8 * kMfmaStreams;
    return m;
}
constexpr size_t gm_h_floats(int hidden) { return (size_t)2 * hidden * kMfmaStreams; }              // [parity][unit][stream] fp32
constexpr size_t gs_h_floats(int hidden) { return (size_t)2 * 3 * ((hidden + 31) / 32) * 64 * 4; }  // [parity][term][k-step][lane] 16-byte B fragments

#ifdef AIDAX_LP_TRACE
constexpr int kTraceT0 = 96;             // LP_STAMP: the selected workgroup stamps ticks 96..103
#endif
// a main wave's lane: where it stands, and h(t-1) of its four units
struct TickLane {
    int tid, lane, wave, q, c;
    float hreg[4];
#ifdef AIDAX_LP_TRACE
    unsigned long long* trace;           // (LP_STAMP reads `trace`, `tick` and `a` from the scope it expands in)
#endif
};

// ================================================================ the frame
// The barrier protocol. Main waves (here) and helper waves (lp_helper) must execute the SAME number of __syncthreads on every
// path — a slip is not a wrong number but a hung workgroup:
//   (1)  once: set-up done — the Dense row, h(t-1) and the live flags are in LDS
//   per chunk of kLpChunk frames:
//   (2)  the chunk's audio rows are in LDS
//   (3)  the helpers have run the head of the pre pass and written frame 0's inputs
//   one per tick, cnt + 2 ticks: h(t), the next frame's inputs and the Dense's partial sums are in LDS (the Dense of a frame
//        trails its h by one tick, its output by two)
//   (4)  the helpers have stored the rows, which may be overwritten
//   once more in the AIDAX_LP_TRACE build, in the selected workgroup only
//   (5)  once: the helpers are through, state goes back to memory
// Nothing between (1) and (5) may return, and no barrier may sit in a branch that a cell decides.
template <class Cell, int NHELP>
__device__ __forceinline__ void tick_frame(const LaunchArgs& a, const MfmaDesc& d, float* smem)
{
    constexpr int H = Cell::H, NW = Cell::NW, NS = kMfmaStreams, NT = NW * kWave;
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int n = (int)a.n_frames;
    const int grp = (int)blockIdx.x;
    const int s_base = grp * NS;
    const int Ht = d.hidden_true;
    const int chunk = n < kLpChunk ? n : kLpChunk;
    const int nP = (chunk + 3) & ~3;
    const TickLds m = tick_lds(smem, H, nP, (int)Cell::kHFloats);
#ifdef AIDAX_LP_TRACE
    // measurement build (scratch/gs_trace.py): the selected workgroup stamps the shader clock at six points of ticks 96..103 on
    // every wave (the helpers in lp_helper) and leaves the stamps in the first floats of its output rows
    unsigned long long* trace = reinterpret_cast<unsigned long long*>(m.hands + NHELP * 2 * kChainHandFloats);
#endif
    if (wave >= NW) {
        lp_helper<H, NW, NHELP>(a, m.xb, m.xin, m.wdl, m.livef, m.dpart, m.hands, grp, nP);
        return;
    }
    const float* W = a.wpack;
    const MfmaLayer& L = d.L[0];
    Cell cell;
    cell.tid = tid; cell.lane = lane; cell.wave = wave;
    cell.q = lane >> 4;
    const int c = cell.c = lane & 15;
#ifdef AIDAX_LP_TRACE
    cell.trace = trace;
#endif
    for (int i = tid; i < H + 1; i += NT) m.wdl[i] = W[d.wd_off + i];
    cell.load_record(W, d);
    // h(t-1) of this lane's four units of stream s_base + c: registers for the launch
    const int sg = s_base + c;
    const bool valid = sg < (int)a.n_streams;
    const float* stp = a.nn + (size_t)(valid ? sg : 0) * a.nn_stride + L.state_off;
    cell.load_state(a, d, m, stp, valid, Ht);
    cell.publish(a, m, 0);
    __syncthreads();                                        // (1)

    int par = 0;                                            // parity of h the next frame reads
    for (int base = 0; base < n; base += kLpChunk) {
        const int cnt = n - base < kLpChunk ? n - base : kLpChunk;
        for (int sl = wave; sl < NS; sl += NW) {            // every valid row: the chains run on net-off streams too
            const int s2 = s_base + sl;
            const bool lv = s2 < (int)a.n_streams;
            float* row = m.xb + sl * nP;
            const float* src = a.in + (size_t)(lv ? s2 : 0) * n + base;
            if (lv && ((n | base) & 3) == 0) load_block(row, src, cnt, lane);
            else for (int t = lane; t < cnt; t += kWave) row[t] = lv ? src[t] : 0.f;
        }
        __syncthreads();                                    // (2)
        __syncthreads();                                    // (3)
        const int ticks = cnt + 2;
        for (int tick = 0; tick < ticks; ++tick) {
            LP_STAMP(0);
            const bool body = tick < cnt;                   // a frame to compute
            const bool dense_on = tick >= 1 && tick <= cnt; // the Dense of frame tick-1
            if (body) {
                cell.frame(a, m, tick, dense_on, par);      // products against h(tick-1) in parity par, cell update, h(tick) into par ^ 1
                par ^= 1;
            } else if (dense_on) {
                cell.dense_only(m, tick, par);              // the Dense of the last frame
            }
            __syncthreads();                                // the tick's barrier
            LP_STAMP(5);
        }
        __syncthreads();                                    // (4)
    }
#ifdef AIDAX_LP_TRACE
    if ((int)blockIdx.x == ((AIDAX_TUNE(a) >> 16) & 0xff)) __syncthreads();      // (lp_helper's extra barrier of the measurement build)
#endif
    __syncthreads();                                        // (5)
#ifdef AIDAX_LP_TRACE
    if ((int)blockIdx.x == ((AIDAX_TUNE(a) >> 16) & 0xff))
        for (int i = tid; i < 2 * 768; i += NT) a.out[(size_t)s_base * n + i] = reinterpret_cast<const float*>(trace)[i];
#endif
    if (valid && m.livef[c] != 0.f) cell.store_state(a.nn + (size_t)sg * a.nn_stride + L.state_off, Ht);
}

// ================================================================ the bf16 x 3 cells (k_gru_gs, k_lstm_gs)
// What round 4 measured (scratch/uoverlap2.hip, uoverlap3.hip, profiles/r04_overlap.txt): v_mfma_f32_16x16x4_f32 runs at the
// VECTOR rate (32 cycles for 1024 MACs) and nothing else of the SIMD issues beside it — a VALU instruction behind an fp32 MFMA
// costs its full issue time whatever accumulator it touches, one wave or two; v_mfma_f32_16x16x32_bf16 does 8192 MACs in ~17
// cycles and hides up to six VALU instructions in its shadow. So the recurrent product U . h(t-1) is computed here from
// operands split EXACTLY into three bf16 terms each (w = w0 + w1 + w2, h = h0 + h1 + h2; 8 + 8 + 8 significant bits,
// round-to-nearest remainders): every bf16 x bf16 product is exact in fp32, the accumulation is fp32 as before, and of the
// nine term products NPROD are issued, smallest first — 9: the fp32 product to the last bit of its operands; 6: without
// w1 h2, w2 h1, w2 h2 (together <= 2^-23 |w h|: below the rounding of the fp32 accumulation that follows).
// The weights arrive split from the packer (pack_mfma, gs record); a lane splits its own four h values after the cell update
// (v_cvt_pk_bf16_f32 rounds to nearest even; the remainders are exact) and writes them where the k-steps read them: h lives
// in LDS as B fragments [parity][term][k-step][lane][8 bf16], one ds_read_b128 per (term, k-step). The model inputs stay one
// fp32 k-step (x, PARAM1, PARAM2 are not products of h), Dense(H,1) is four FMAs on the lane's own h and two permlane swaps.
//
// term products, smallest first: (weight term, h term)
__device__ __forceinline__ constexpr int gs_term(int product, int side)
{
    constexpr int P9[9][2] = { {2, 2}, {1, 2}, {2, 1}, {0, 2}, {1, 1}, {2, 0}, {0, 1}, {1, 0}, {0, 0} };
    return P9[product][side];
}
struct GsDense { float dy; Pair dp; };                      // the Dense of a frame on its way through dense_step

// What the two cells share: NGATE gate tiles of split weights, the lane's Dense weights, its place in the fragments.
template <int UT, int NPROD, int NGATE>
struct GsCell : TickLane {
    static constexpr int H = 16 * UT, NW = UT, NS = kMfmaStreams;
    static constexpr int KS2 = (H + 31) / 32;               // bf16 k-steps (32 columns each; 48 units: the second one half empty)
    static constexpr int kFrag = 3 * KS2 * 64;              // 16-byte B fragments of one parity: [term][k-step][lane]
    static constexpr size_t kHFloats = gs_h_floats(H);
    static_assert(NPROD == 6 || NPROD == 9, "six products (to fp32 rounding) or all nine");
    bf16x8 wq[NGATE][KS2][3];                               // the recurrent weights as split bf16 A fragments: [gate][k-step][term]
    float dw[4];                                            // Dense weights of this lane's four units
    // where this lane's four values sit in the fragments: k = 16 wave + 4q + e -> k-step wave / 2, lane row 2 (wave & 1) + q / 2,
    // elements 4 (q & 1) .. + 3 of that lane's eight: the upper or lower 8 bytes of its 16
    int my_slot, my_half;

    __device__ __forceinline__ void load_wq(const u32x4* sp)      // sp: this lane's first fragment, [gate][k-step][term][lane]
    {
#pragma unroll
        for (int g = 0; g < NGATE; ++g)
#pragma unroll
            for (int ks = 0; ks < KS2; ++ks)
#pragma unroll
                for (int t = 0; t < 3; ++t) wq[g][ks][t] = __builtin_bit_cast(bf16x8, sp[((g * KS2 + ks) * 3 + t) * kWave]);
    }
    template <typename Extra>
    __device__ __forceinline__ void load_lane(const float* W, const MfmaDesc& d, const float* stp, bool valid, int Ht, Extra extra)
    {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int u = 16 * wave + 4 * q + e;
            hreg[e] = (valid && u < Ht) ? stp[u] : 0.f;     // padded units rest at 0
            extra(e, u);
            dw[e] = W[d.wd_off + u];                        // (zero for padded units)
        }
        my_slot = (wave >> 1) * 64 + (2 * (wave & 1) + (q >> 1)) * 16 + c;
        my_half = q & 1;
    }
    __device__ __forceinline__ u32x4* frags(const TickLds& m, int parity) const { return reinterpret_cast<u32x4*>(m.h) + parity * kFrag; }
    // the lane's four new h values, split, to where the k-steps of the next tick read them
    __device__ __forceinline__ void publish(const TickLds& m, int parity)
    {
        u32x2 t[3];
        gs_split4(hreg, t);
#pragma unroll
        for (int k = 0; k < 3; ++k)
            reinterpret_cast<u32x2*>(frags(m, parity) + k * KS2 * 64 + my_slot)[my_half] = t[k];
    }
    __device__ __forceinline__ void zero_tail(const TickLds& m)
    {
        if constexpr (H % 32 != 0) {                        // columns H .. 32 KS2 - 1 of the last k-step (lane rows 2, 3) are nobody's: zero, for good
            for (int i = tid; i < 2 * 3 * 32; i += NW * kWave)
                frags(m, 0)[(i / 32) * KS2 * 64 + (KS2 - 1) * 64 + 32 + (i & 31)] = u32x4{ 0u, 0u, 0u, 0u };
        }
    }
    // h(t-1) as B fragments, requested in the order of their use
    __device__ __forceinline__ void load_frags(bf16x8 (&hb)[KS2][3], const TickLds& m, int parity) const
    {
        const u32x4* h_rd = frags(m, parity) + lane;
#pragma unroll
        for (int t = 2; t >= 0; --t)
#pragma unroll
            for (int ks = 0; ks < KS2; ++ks) hb[ks][t] = __builtin_bit_cast(bf16x8, h_rd[(t * KS2 + ks) * 64]);
    }
    // Dense of frame tick-1 from the lane's own h(tick-1), in nine steps (four multiply-adds over the lane's units in a fixed
    // order, two permlane swaps over the lane rows, the store) — issued one behind every second MFMA of the first product
    // loop: bf16 MFMAs leave the VALU free while they run (profiles/r04_overlap.txt)
    __device__ __forceinline__ void dense_step(int k, GsDense& y, const TickLds& m, int tick, bool dense_on) const
    {
        switch (k) {
        case 0: y.dy = dw[0] * hreg[0]; break;
        case 1: y.dy = __builtin_fmaf(dw[1], hreg[1], y.dy); break;
        case 2: y.dy = __builtin_fmaf(dw[2], hreg[2], y.dy); break;
        case 3: y.dy = __builtin_fmaf(dw[3], hreg[3], y.dy); break;
        case 4: y.dp = share_rows(y.dy); break;             // rows q and q ^ 1
        case 5: y.dy = y.dp.lo + y.dp.hi; break;
        case 6: y.dp = share_halves(y.dy); break;           // ... and the other half of the wave
        case 7: y.dy = y.dp.lo + y.dp.hi; break;
        case 8: if (dense_on && lane < NS) m.dpart[((tick & 1) * NW + wave) * NS + lane] = y.dy; break;
        default: break;
        }
    }
    __device__ __forceinline__ void dense_only(const TickLds& m, int tick, int) const
    {
        GsDense y = { 0.f, { 0.f, 0.f } };
#pragma unroll
        for (int k = 0; k < 9; ++k) dense_step(k, y, m, tick, true);
    }
    // the NPROD x KS2 MFMA groups of gates GA and GB (GB < 0: GA alone), `valu(j)` in the shadow of group j
    template <int GA, int GB, int NACC, typename Valu>
    __device__ __forceinline__ void products(f32x4 (&acc)[NACC], const bf16x8 (&hb)[KS2][3], Valu valu) const
    {
#pragma unroll
        for (int j = 0; j < NPROD * KS2; ++j) {
            const int pi = 9 - NPROD + j / KS2, ks = j % KS2;
            acc[GA] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wq[GA][ks][gs_term(pi, 0)], hb[ks][gs_term(pi, 1)], acc[GA], 0, 0, 0);
            if constexpr (GB >= 0)
                acc[GB] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wq[GB][ks][gs_term(pi, 0)], hb[ks][gs_term(pi, 1)], acc[GB], 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
            valu(j);
            __builtin_amdgcn_sched_barrier(0);
        }
    }
};

// ---------------------------------------------------------------- k_gru_gs: k_gru_gm with the recurrent product on the bf16 matrix pipe
// Per wave and frame: 3 gates x 2 k-steps x NPROD bf16 MFMAs (36 x 17 cycles for NPROD = 6) instead of 48 fp32 MFMAs x 32.
// The fp32 pieces (input k-step, bias rows) come from the gate-major record, the split weights from the gs record.
template <int UT, int NPROD>
struct GruGs : GsCell<UT, NPROD, 3> {
    using Base = GsCell<UT, NPROD, 3>;
    using Base::KS2; using Base::kFrag; using Base::H;
    using Base::lane; using Base::wave; using Base::hreg;
#ifdef AIDAX_LP_TRACE
    using Base::trace;
#endif
    float w_in[3];
    f32x4 bias[4];

    __device__ __forceinline__ void load_record(const float* W, const MfmaDesc& d)
    {
        constexpr int KS = H / 4;
        const float* rec = W + d.gm_off + (size_t)wave * kWave * (3 + 3 * KS + 16);
#pragma unroll
        for (int g = 0; g < 3; ++g) w_in[g] = rec[g * kWave + lane];
#pragma unroll
        for (int g = 0; g < 4; ++g) bias[g] = *reinterpret_cast<const f32x4*>(rec + (3 + 3 * KS) * kWave + (g * kWave + lane) * 4);
        this->load_wq(reinterpret_cast<const u32x4*>(W + d.gs_off) + (size_t)wave * 3 * KS2 * 3 * kWave + lane);
    }
    __device__ __forceinline__ void load_state(const LaunchArgs& a, const MfmaDesc& d, const TickLds& m, const float* stp, bool valid, int Ht)
    {
        this->load_lane(a.wpack, d, stp, valid, Ht, [](int, int) {});
        this->zero_tail(m);
    }
    __device__ __forceinline__ void publish([[maybe_unused]] const LaunchArgs& a, const TickLds& m, int parity)
    {
        if (AIDAX_TUNE(a) & 1048576) {
            // (bit 1048576, test build: term 0 of h only — an upper bound on what taking terms 1 and 2 of the split off the tick's critical
            // path could buy, the round-5 review's item 8; wrong output)
            u32x2 t0 = { gs_pack_bf16(hreg[0], hreg[1]), gs_pack_bf16(hreg[2], hreg[3]) };
            reinterpret_cast<u32x2*>(this->frags(m, parity) + this->my_slot)[this->my_half] = t0;
            return;
        }
        Base::publish(m, parity);
    }
    __device__ __forceinline__ void frame([[maybe_unused]] const LaunchArgs& a, const TickLds& m, int tick, bool dense_on, int par)
    {
        GsDense y = { 0.f, { 0.f, 0.f } };
        bf16x8 hb[KS2][3];
        this->load_frags(hb, m, par);
        f32x4 acc[3] = { bias[0], bias[1], bias[2] };
        f32x4 ax = bias[3];
        const float bx = m.xin[(tick & 1) * 64 + lane];
        LP_STAMP(1);
        acc[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(w_in[0], bx, acc[0], 0, 0, 0);
        acc[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(w_in[1], bx, acc[1], 0, 0, 0);
        // z and r first, two accumulators in turn, the Dense's steps behind them ...
        this->template products<0, 1>(acc, hb, [&](int j) { this->dense_step(j, y, m, tick, dense_on); });
        // ... then the candidate's chain, with the sigmoids of z and r in its shadow: 2^v for the eight values behind
        // the first four MFMAs, 1 / (1 + .) behind the next eight
        float sg8[8];
        this->template products<2, -1>(acc, hb, [&](int j) {
            if (j < 4) {
                sg8[2 * j] = __builtin_amdgcn_exp2f(acc[(2 * j) >> 2][(2 * j) & 3]);
                sg8[2 * j + 1] = __builtin_amdgcn_exp2f(acc[(2 * j + 1) >> 2][(2 * j + 1) & 3]);
            } else if (j < 12) {
                sg8[j - 4] = __builtin_amdgcn_rcpf(1.0f + sg8[j - 4]);      // sigmoid_pre: the rows carry -log2 e
            }
        });
        // The candidate's input half last, next to its only use. The sched_barriers above fix the order of the bf16 MFMAs and the VALU
        // steps between them; they do NOT pin this MFMA: it has no operand in common with the loops, and written ahead of them
        // (where bias and bx are at hand) the optimizer either sinks it down here before the loops are unrolled or leaves it ahead of
        // the z / r products, depending on unrelated code. Ahead, cfg3's frame measured 1 % longer (profiles/tick_frame.txt): an fp32
        // MFMA holds the VALU for its whole issue time. So the source says where it goes.
        ax = __builtin_amdgcn_mfma_f32_16x16x4f32(w_in[2], bx, ax, 0, 0, 0);
        LP_STAMP(2);
        // the cell update two units per instruction (v_pk_fma_f32 / v_pk_add_f32 around the two exponentials and reciprocals: the
        // same operations per unit, the same bits): 18 instructions for 28 between the last MFMA and the publish — with gs_split4's
        // packed subtractions cfg3 192.6 -> 188.0 us against one unit per instruction (profiles/r05_DESIGN_archive.md).
        // (Also tried: issue priority 3 for this tail — cell update, split, publish — ahead of the helpers. No result is recorded.)
#pragma unroll
        for (int e = 0; e < 4; e += 2) {
            const gs_f32x2 gz = { sg8[e], sg8[e + 1] }, gr = { sg8[4 + e], sg8[5 + e] };
            const gs_f32x2 pre = __builtin_elementwise_fma(gr, gs_f32x2{ acc[2][e], acc[2][e + 1] }, gs_f32x2{ ax[e], ax[e + 1] });      // (the record's candidate rows carry 2 log2 e)
            const gs_f32x2 ex = { __builtin_amdgcn_exp2f(pre.x), __builtin_amdgcn_exp2f(pre.y) };
            const gs_f32x2 sm = ex + gs_f32x2{ 1.0f, 1.0f };
            const gs_f32x2 rc = { __builtin_amdgcn_rcpf(sm.x), __builtin_amdgcn_rcpf(sm.y) };
            const gs_f32x2 nn = __builtin_elementwise_fma(gs_f32x2{ -2.0f, -2.0f }, rc, gs_f32x2{ 1.0f, 1.0f });     // tanh_exp_pre
            const gs_f32x2 hh = __builtin_elementwise_fma(gz, gs_f32x2{ hreg[e], hreg[e + 1] } - nn, nn);
            hreg[e] = hh.x; hreg[e + 1] = hh.y;
        }
        LP_STAMP(3);
        publish(a, m, par ^ 1);
        LP_STAMP(4);
    }
    __device__ __forceinline__ void store_state(float* dst, int Ht) const
    {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int u = 16 * wave + 4 * this->q + e;
            if (u < Ht) dst[u] = hreg[e];
        }
    }
};

// ---------------------------------------------------------------- k_lstm_gs: the same for one-layer LSTMs
// The four gate tiles i | f | g | o of a wave's 16 units: a lane's accumulator quads are the four gates of four ADJACENT units of
// one stream. Per frame and main wave: 4 fp32 MFMAs (the model inputs' k-step), 4 x KS2 x NPROD bf16 MFMAs (48 for 64 units) — i
// and g first, two accumulators in turn with the Dense's steps behind them, then f and o with sigmoid(i), tanh(g) and their
// product dealt out in their shadow — then the rest of the cell update (the same operations in the same order as k_mfma_ls's
// cell_step: sigmoid_pre, tanh_rat), the split of the four new h values and three 8-byte fragment writes, one barrier.
// The record: pack_mfma, gs_off.
template <int UT, int NPROD>
struct LstmGs : GsCell<UT, NPROD, 4> {
    using Base = GsCell<UT, NPROD, 4>;
    using Base::KS2; using Base::lane; using Base::wave; using Base::hreg;
    float w_in[4], creg[4];
    f32x4 bias[4];

    __device__ __forceinline__ void load_record(const float* W, const MfmaDesc& d)
    {
        constexpr size_t kRecFloats = 4 * kWave + 4 * kWave * 4 + (size_t)4 * KS2 * 3 * kWave * 4;      // per wave: input k-step, bias quads, split fragments
        const float* rec = W + d.gs_off + (size_t)wave * kRecFloats;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            w_in[g] = rec[g * kWave + lane];
            bias[g] = *reinterpret_cast<const f32x4*>(rec + 4 * kWave + (g * kWave + lane) * 4);
        }
        this->load_wq(reinterpret_cast<const u32x4*>(rec + 4 * kWave + 4 * kWave * 4) + lane);
    }
    __device__ __forceinline__ void load_state(const LaunchArgs& a, const MfmaDesc& d, const TickLds& m, const float* stp, bool valid, int Ht)
    {
        this->load_lane(a.wpack, d, stp, valid, Ht, [&](int e, int u) { creg[e] = (valid && u < Ht) ? stp[Ht + u] : 0.f; });
        this->zero_tail(m);
    }
    __device__ __forceinline__ void publish(const LaunchArgs&, const TickLds& m, int parity) { Base::publish(m, parity); }
    __device__ __forceinline__ void frame(const LaunchArgs&, const TickLds& m, int tick, bool dense_on, int par)
    {
        GsDense y = { 0.f, { 0.f, 0.f } };
        bf16x8 hb[KS2][3];
        this->load_frags(hb, m, par);
        f32x4 acc[4] = { bias[0], bias[1], bias[2], bias[3] };
        const float bx = m.xin[(tick & 1) * 64 + lane];
#pragma unroll
        for (int g = 0; g < 4; ++g) acc[g] = __builtin_amdgcn_mfma_f32_16x16x4f32(w_in[g], bx, acc[g], 0, 0, 0);
        // i and g first, two accumulators in turn, the Dense's steps behind them ...
        this->template products<0, 2>(acc, hb, [&](int j) { this->dense_step(j, y, m, tick, dense_on); });
        // ... then f and o, with sigmoid(i) * tanh(g) of the four units in their shadow: six steps per unit (sigmoid_pre: the
        // sigmoid rows carry -log2 e; tanh_rat: the odd rational x P(x^2) / Q(x^2))
        float ig[4], tx[4], tu[4], tp[4], tq[4], te[4];
        auto ig_step = [&](int e, int k) {
            switch (k) {
            case 0: tx[e] = tanh_rat_clamp(acc[2][e]); tu[e] = tx[e] * tx[e]; te[e] = __builtin_amdgcn_exp2f(acc[0][e]); break;
            case 1: tp[e] = __builtin_fmaf(kTanhP[6], tu[e], kTanhP[5]); tp[e] = __builtin_fmaf(tp[e], tu[e], kTanhP[4]); tp[e] = __builtin_fmaf(tp[e], tu[e], kTanhP[3]); break;
            case 2: tp[e] = __builtin_fmaf(tp[e], tu[e], kTanhP[2]); tp[e] = __builtin_fmaf(tp[e], tu[e], kTanhP[1]); tp[e] = __builtin_fmaf(tp[e], tu[e], kTanhP[0]); break;
            case 3: tq[e] = __builtin_fmaf(kTanhQ[3], tu[e], kTanhQ[2]); tq[e] = __builtin_fmaf(tq[e], tu[e], kTanhQ[1]); tq[e] = __builtin_fmaf(tq[e], tu[e], kTanhQ[0]); break;
            case 4: te[e] = __builtin_amdgcn_rcpf(1.0f + te[e]); tq[e] = __builtin_amdgcn_rcpf(tq[e]); break;
            case 5: ig[e] = te[e] * ((tp[e] * tx[e]) * tq[e]); break;
            default: break;
            }
        };
        this->template products<1, 3>(acc, hb, [&](int j) {
            if (j < 12) { ig_step((2 * j) & 3, (2 * j) >> 2); ig_step((2 * j + 1) & 3, (2 * j + 1) >> 2); }      // 24 steps: the units advance together
        });
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float f = __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(acc[1][e]));
            const float o = __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(acc[3][e]));
            creg[e] = __builtin_fmaf(f, creg[e], ig[e]);
            hreg[e] = o * tanh_rat(creg[e]);
        }
        Base::publish(m, par ^ 1);
    }
    __device__ __forceinline__ void store_state(float* dst, int Ht) const
    {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int u = 16 * wave + 4 * this->q + e;
            if (u < Ht) { dst[u] = hreg[e]; dst[Ht + u] = creg[e]; }
        }
    }
};

// ================================================================ the kernels
// ================================================================ k_gru_gm: one-layer GRU, gate-major tiles
// The tiles of k_mfma / k_mfma_lp hold four gate rows per unit; a GRU has three that contract over h (z, r and the
// candidate's recurrent half) and one that only sees the model inputs, so a quarter of the recurrent MFMAs multiply zeros.
// Here a wave owns 16 units as three recurrent tiles of their own (z, r, recurrent half: H/4 k-steps each) plus the
// input half as a fourth accumulator that takes the input k-step only: 3 H/4 + 3 MFMAs per wave and frame instead of
// 4 (H/4 + 1) — GRU-64: 51 against 68 per SIMD. A lane then holds the four gates of FOUR units (rows 4q .. 4q+3 of each
// tile) for its stream, and one main wave per SIMD does it (H / 16 of them) next to one helper wave.
// Same weights and the same accumulation order per row as pack_mfma's other record: the recurrent state is
// bit-identical to k_mfma's (which warms the model up) and k_mfma_lp's.
// h lives in LDS as [parity][unit][stream] floats, and the Dense is an MFMA against it (this wave's k-steps).
// This kernel is NOT on tick_frame: it is the fp32 partner that k_gru_gs is measured against (AIDAX_GRU_GM=f32, hooks builds), and as a
// cell of the frame it ran 1.8 - 2.4 % slower than before with the same MFMA and LDS-read sequence (profiles/tick_frame.txt). It keeps
// its own tick loop; the indices, the LDS carve-up (tick_lds), the staging loop and barriers (1) .. (5) follow tick_frame's protocol
// line by line, and a change there has to be made here too.
template <int UT, int NHELP>
__global__ __launch_bounds__((UT + NHELP) * kWave) void k_gru_gm(LaunchArgs a, MfmaDesc d)
{
    extern __shared__ __attribute__((aligned(16))) float smem[];
    constexpr int H = 16 * UT, NW = UT, NS = kMfmaStreams, KS = H / 4, NT = NW * kWave;
    constexpr int DK = KS / NW;                             // Dense k-steps per wave (= 4)
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int n = (int)a.n_frames;
    const int grp = (int)blockIdx.x;
    const int s_base = grp * NS;
    const int Ht = d.hidden_true;
    const int chunk = n < kLpChunk ? n : kLpChunk;
    const int nP = (chunk + 3) & ~3;
    // (tick_lds's carve-up, written out: taken through the function, the last h k-step read of the frame loop gets an address of its
    // own and the MFMA group behind it is split by a wait — isa_seq shows it, and nothing in the source explains it)
    TickLds m;
    m.xb = smem; m.xin = m.xb + NS * nP; m.h = m.xin + 2 * 64; m.wdl = m.h + 2 * H * NS; m.livef = m.wdl + ((H + 1 + 3) & ~3); m.dpart = m.livef + NS; m.hands = m.dpart + 2 * 8 * NS;
    float *xb = m.xb, *xin = m.xin, *hT = m.h /* [2][H][NS] */, *wdl = m.wdl, *livef = m.livef, *dpart = m.dpart, *hands = m.hands;
    if (wave >= NW) {
        lp_helper<H, NW, NHELP>(a, xb, xin, wdl, livef, dpart, hands, grp, nP);
        return;
    }
    const float* W = a.wpack;
    const MfmaLayer& L = d.L[0];
    const int q = lane >> 4, c = lane & 15;
    for (int i = tid; i < H + 1; i += NT) wdl[i] = W[d.wd_off + i];
    // this wave's record (pack_mfma: gate-major)
    const float* rec = W + d.gm_off + (size_t)wave * kWave * (3 + 3 * KS + 16);
    float w_in[3], w_rec[KS][3];
#pragma unroll
    for (int g = 0; g < 3; ++g) w_in[g] = rec[g * kWave + lane];
#pragma unroll
    for (int kk = 0; kk < KS; ++kk)
#pragma unroll
        for (int g = 0; g < 3; ++g) w_rec[kk][g] = rec[(3 + 3 * kk + g) * kWave + lane];
    f32x4 bias[4];
#pragma unroll
    for (int g = 0; g < 4; ++g) bias[g] = *reinterpret_cast<const f32x4*>(rec + (3 + 3 * KS) * kWave + (g * kWave + lane) * 4);
    float dfrag[DK];
#pragma unroll
    for (int i = 0; i < DK; ++i) dfrag[i] = c == 0 ? W[d.wd_off + 4 * (wave * DK + i) + q] : 0.f;
    // h(t-1) of this lane's four units (16 wave + 4q + e) of stream s_base + c: registers for the launch, LDS for the others
    const int sg = s_base + c;
    const bool valid = sg < (int)a.n_streams;
    const float* stp = a.nn + (size_t)(valid ? sg : 0) * a.nn_stride + L.state_off;
    float hreg[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int u = 16 * wave + 4 * q + e;
        hreg[e] = (valid && u < Ht) ? stp[u] : 0.f;         // padded units rest at 0
        hT[u * NS + c] = hreg[e];
    }
    __syncthreads();                                        // (1)

    int par = 0;
    for (int base = 0; base < n; base += kLpChunk) {
        const int cnt = n - base < kLpChunk ? n - base : kLpChunk;
        for (int sl = wave; sl < NS; sl += NW) {            // every valid row: the chains run on net-off streams too
            const int s2 = s_base + sl;
            const bool lv = s2 < (int)a.n_streams;
            float* row = xb + sl * nP;
            const float* src = a.in + (size_t)(lv ? s2 : 0) * n + base;
            if (lv && ((n | base) & 3) == 0) load_block(row, src, cnt, lane);
            else for (int t = lane; t < cnt; t += kWave) row[t] = lv ? src[t] : 0.f;
        }
        __syncthreads();                                    // (2)
        __syncthreads();                                    // (3) the helpers have run the head of the pre pass and written frame 0's inputs
        const int ticks = cnt + 2;
        for (int tick = 0; tick < ticks; ++tick) {
            const float* h_rd = hT + par * H * NS;
            float* h_wr = hT + (par ^ 1) * H * NS;
            if (tick >= 1 && tick <= cnt) {                 // Dense of frame tick-1: this wave's k-steps against h(tick-1)
                f32x4 dacc = f32x4{ 0.f, 0.f, 0.f, 0.f };
#pragma unroll
                for (int i = 0; i < DK; ++i)
                    dacc = __builtin_amdgcn_mfma_f32_16x16x4f32(dfrag[i], h_rd[64 * (wave * DK + i) + lane], dacc, 0, 0, 0);
                if (lane < NS) dpart[((tick & 1) * NW + wave) * NS + lane] = dacc.x;
            }
            if (tick < cnt) {
                f32x4 az = bias[0], ar = bias[1], an = bias[2], ax = bias[3];
                const float bx = xin[(tick & 1) * 64 + lane];
                az = __builtin_amdgcn_mfma_f32_16x16x4f32(w_in[0], bx, az, 0, 0, 0);
                ar = __builtin_amdgcn_mfma_f32_16x16x4f32(w_in[1], bx, ar, 0, 0, 0);
                ax = __builtin_amdgcn_mfma_f32_16x16x4f32(w_in[2], bx, ax, 0, 0, 0);
                // h k-steps, the B values a group of four ahead of the MFMAs that use them
                float b0[4], b1[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) b0[j] = h_rd[64 * j + lane];
#pragma unroll
                for (int g = 0; g < KS / 4; ++g) {
                    if (g + 1 < KS / 4) {
#pragma unroll
                        for (int j = 0; j < 4; ++j) (g & 1 ? b0 : b1)[j] = h_rd[64 * (4 * (g + 1) + j) + lane];
                    }
                    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const float bh = (g & 1 ? b1 : b0)[j];
                        az = __builtin_amdgcn_mfma_f32_16x16x4f32(w_rec[4 * g + j][0], bh, az, 0, 0, 0);
                        ar = __builtin_amdgcn_mfma_f32_16x16x4f32(w_rec[4 * g + j][1], bh, ar, 0, 0, 0);
                        an = __builtin_amdgcn_mfma_f32_16x16x4f32(w_rec[4 * g + j][2], bh, an, 0, 0, 0);
                    }
                    __builtin_amdgcn_sched_barrier(0);
                }
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float gz = sigmoid_pre(az[e]), gr = sigmoid_pre(ar[e]);
                    const float nn = tanh_exp_pre(__builtin_fmaf(gr, an[e], ax[e]));      // (the record's candidate rows carry 2 log2 e)
                    const float hn = __builtin_fmaf(gz, hreg[e] - nn, nn);
                    hreg[e] = hn;
                    h_wr[(16 * wave + 4 * q + e) * NS + c] = hn;
                }
                par ^= 1;
            }
            __syncthreads();                                // the tick's barrier
        }
        __syncthreads();                                    // (4) the helpers have stored the rows
    }
#ifdef AIDAX_LP_TRACE
    if ((int)blockIdx.x == ((AIDAX_TUNE(a) >> 16) & 0xff)) __syncthreads();      // (lp_helper's extra barrier of the measurement build)
#endif
    __syncthreads();                                        // (5)
    if (valid && livef[c] != 0.f) {
        float* dst = a.nn + (size_t)sg * a.nn_stride + L.state_off;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int u = 16 * wave + 4 * q + e;
            if (u < Ht) dst[u] = hreg[e];
        }
    }
}
template <int UT, int NHELP, int NPROD>
__global__ __launch_bounds__((UT + NHELP) * kWave) void k_gru_gs(LaunchArgs a, MfmaDesc d)
{
    extern __shared__ __attribute__((aligned(16))) float smem[];
    tick_frame<GruGs<UT, NPROD>, NHELP>(a, d, smem);
}
template <int UT, int NHELP, int NPROD>
__global__ __launch_bounds__((UT + NHELP) * kWave) void k_lstm_gs(LaunchArgs a, MfmaDesc d)
{
    extern __shared__ __attribute__((aligned(16))) float smem[];
    tick_frame<LstmGs<UT, NPROD>, NHELP>(a, d, smem);
}

// ---------------------------------------------------------------- host side
static hipError_t tick_launch(GmFn fn, int main_waves, int helpers, size_t lds, const LaunchArgs& a, const MfmaDesc& d, hipStream_t stream)
{
    if (!fn || a.mode != MODE_CHAIN || a.n_frames == 0) return hipErrorInvalidValue;
    if (const hipError_t e = lp_allow_lds(fn, lds); e != hipSuccess) return e;
    const uint32_t groups = (a.n_streams + kMfmaStreams - 1) / kMfmaStreams;
    hipLaunchKernelGGL(fn, dim3(groups), dim3((main_waves + helpers) * kWave), lds, stream, a, d);
    return hipGetLastError();
}

// k_gru_gm: one-layer GRU models with three or four main waves (48 / 64 units after rounding up to 16). Narrower ones would
// leave SIMDs without a main wave — GRU-32 at 4096 streams: 245 us here against 197 us on k_mfma_lp's one-launch form,
// whose eight waves share one tile row each.
static GmFn gm_fn(int hidden)
{
    switch (hidden) {
    case 48: return k_gru_gm<3, kLpHelpers>;
    case 64: return k_gru_gm<4, kLpHelpers>;
    default: return nullptr;
    }
}
bool gru_gm_serves(const MfmaDesc& d) { return d.n_layers == 1 && d.L[0].cell == 1 && d.gm_off != 0 && gm_fn(d.hidden) != nullptr; }
size_t gru_gm_lds_bytes(const MfmaDesc& d, uint32_t n_frames) { return tick_lds_floats(d.hidden, (int)n_frames, kLpHelpers, gm_h_floats(d.hidden)) * sizeof(float); }
hipError_t launch_gru_gm_kernel(const LaunchArgs& a, const MfmaDesc& d, hipStream_t stream)
{
    return tick_launch(gru_gm_serves(d) ? gm_fn(d.hidden) : nullptr, d.hidden / 16, kLpHelpers, gru_gm_lds_bytes(d, a.n_frames), a, d, stream);
}

// k_gru_gs: the same models as k_gru_gm, recurrent product on the bf16 matrix pipe (operands split into three bf16 terms)
static GmFn gs_fn(int hidden, int nprod)
{
    switch (hidden) {
    case 48: return nprod == 9 ? k_gru_gs<3, kLpHelpers, 9> : k_gru_gs<3, kLpHelpers, 6>;
    case 64: return nprod == 9 ? k_gru_gs<4, kLpHelpers, 9> : k_gru_gs<4, kLpHelpers, 6>;
    // 80 units: five main waves and TWO helpers (eight streams each) — seven waves, two per SIMD at most, 256 registers each;
    // one SIMD carries two main waves (no fp32 twin: k_gru_gm stays with 48 / 64 units)
    case 80: return nprod == 9 ? k_gru_gs<5, 2, 9> : k_gru_gs<5, 2, 6>;
    default: return nullptr;
    }
}
static int gs_helpers(int hidden) { return hidden == 80 ? 2 : kLpHelpers; }
static size_t gs_lds_bytes(const MfmaDesc& d, uint32_t n_frames) { return tick_lds_floats(d.hidden, (int)n_frames, gs_helpers(d.hidden), gs_h_floats(d.hidden)) * sizeof(float); }
bool gru_gs_serves(const MfmaDesc& d) { return d.n_layers == 1 && d.L[0].cell == 1 && d.gm_off != 0 && d.gs_off != 0 && gs_fn(d.hidden, 6) != nullptr; }
size_t gru_gs_lds_bytes(const MfmaDesc& d, uint32_t n_frames) { return gs_lds_bytes(d, n_frames); }
hipError_t launch_gru_gs_kernel(const LaunchArgs& a, const MfmaDesc& d, int n_products, hipStream_t stream)
{
    return tick_launch(gru_gs_serves(d) ? gs_fn(d.hidden, n_products) : nullptr, d.hidden / 16, gs_helpers(d.hidden), gs_lds_bytes(d, a.n_frames), a, d, stream);
}

// k_lstm_gs: one-layer LSTMs of 48 (LSTM-40 padded) / 64 units — as many main waves as a CU has SIMDs or one fewer, 256 registers each
static GmFn lgs_fn(int hidden, int nprod)
{
    switch (hidden) {
    case 48: return nprod == 9 ? k_lstm_gs<3, kLpHelpers, 9> : k_lstm_gs<3, kLpHelpers, 6>;
    case 64: return nprod == 9 ? k_lstm_gs<4, kLpHelpers, 9> : k_lstm_gs<4, kLpHelpers, 6>;
    case 80: return k_lstm_gs<5, 2, 6>;                      // (five main waves, two helpers: as k_gru_gs for 80 units; nine products do not fit the registers)
    default: return nullptr;
    }
}
bool lstm_gs_serves(const MfmaDesc& d) { return d.n_layers == 1 && d.L[0].cell == 0 && d.gs_off != 0 && lgs_fn(d.hidden, 6) != nullptr; }
size_t lstm_gs_lds_bytes(const MfmaDesc& d, uint32_t n_frames) { return gs_lds_bytes(d, n_frames); }
hipError_t launch_lstm_gs_kernel(const LaunchArgs& a, const MfmaDesc& d, int n_products, hipStream_t stream)
{
    return tick_launch(lstm_gs_serves(d) ? lgs_fn(d.hidden, n_products) : nullptr, d.hidden / 16, gs_helpers(d.hidden), gs_lds_bytes(d, a.n_frames), a, d, stream);
}

}  // namespace aidax
