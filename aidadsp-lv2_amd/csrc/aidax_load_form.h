// aidax_load_form.h — which kind of slot and which SlotForm a model gets in a pool: the ONE statement of it. choose_form
// (aidax_pool_model.cpp) packs the weights, asks the kernels' own *_serves / *_lds_bytes functions for the facts, calls the functions below and
// copies the answer into the slot; aidax_pass_form.h turns that SlotForm into the form of each pass. A new kernel form is one fact, one line
// of a rule here and one row of tests/form_harness.cpp. No HIP header, no lock, no allocation, no environment: a plain host program can
// include this file (tests/form_harness.cpp does).
#pragma once

#include <cstddef>
#include <cstdint>

#include "aidax.h"
#include "aidax_pass_form.h"

namespace aidax {

// The test switches of this decision, parsed once per load and per ABI call (read_form_hooks, aidax_pool_model.cpp: tests switch forms within
// one process). The shipped library compiles every one of them to "unset", which is what a default-constructed FormHooks says.
struct FormHooks {
    int ls1 = -1;                     // AIDAX_LS1: a lone layer on k_mfma_ls1 — -1 unset (lone_split_pays), 0 never, 1 wherever it serves
    int lstm_gs = -1;                 // AIDAX_LSTM_GS: -1 unset (lstm_gs_pays' rule), 0 never, 1 wherever it serves
    char gru_gm = 0;                  // AIDAX_GRU_GM: 0 none, '0' the four-rows-per-unit kernels, 'f' k_gru_gm with fp32 MFMAs (=f32) — A/B runs
    int mfma_lp = -1;                 // AIDAX_MFMA_LP: the chained kernels -1 where they pay, 0 never, 1 wherever they serve (and never in ranges)
    char lp_split = 0;                // AIDAX_LP_SPLIT: 0 none, '0' the fp32 kernel (no k_mfma_ls), '9' every term product instead of six
    bool lp_fused_off = false;        // AIDAX_LP_FUSED=0: packed k_chain launches around the chained kernel
    bool round_groups_set = false;    // AIDAX_LP_ROUND_GROUPS (tests: ranges of this many stream groups, so that a small pool goes out in several):
    int round_groups = 0;             // ... set at all, and its number (<= 0: the device's own range)
    int gs_products = 6;              // AIDAX_GS_PRODUCTS=9: every term product of the split operands instead of six
    bool conv_ms_off = false;         // AIDAX_CONV_MS=0: k_conv_mfma, the fp32 partner
    bool conv_st_off = false;         // AIDAX_CONV_ST=0: k_conv_ms for every block
    int conv_fused = -1;              // AIDAX_CONV_FUSED: -1 unset (by pool size), 0 / 1 force the form
};

enum ManyForm { MANY_NONE = 0, MANY_QUAD = 1, MANY_MFMA = 2 };

// ---- the one-layer rule: which many-streams form serves a model of the reference's table best at a given stream count ----
// Measured (scratch/perf_table_mfma.py, 256-frame blocks, MI355X): k_quad (4 streams per workgroup on
// mfma_4x4x1, weights in registers) wins for <= 32 units from 4096 streams (1.15-1.5x over the split form) and
// for the wide cells at every stream count below that (LSTM-64 1.3-1.6x, LSTM-80 1.3-1.75x, GRU-80 1.2-1.4x);
// k_mfma (16 streams per workgroup on mfma_16x16x4) takes over for the wide cells from 4096-8192 streams
// (LSTM-80 @ 16384: 2.3 ms against 4.3 ms for k_quad and 8.4 ms for the one-wave kernel). GRU-64 ties with
// its register kernel up to 8192 streams and stays there.
// Round 3 (scratch/perf_lp1.py, profiles/r03_cfg3_forms.txt): the one-launch form of k_mfma_lp (one workgroup per 16
// streams, the DSP chain on its helper waves) costs the same whatever the stream count while its workgroups fit the
// machine in one round, and beats every other form when that round is (nearly) full — LSTM-32 209 us against 231,
// GRU-32 197 / 211, LSTM-40 338 / 346, GRU-64 434 / 468 at 4096 streams on 256 CUs; at 3072 streams the others win.
// One-layer models on k_mfma_ls1 (k_mfma_ls's body for a lone layer: the recurrent product as bf16 term products, a workgroup per
// 16 streams): where it beats every other form at 256-frame blocks on 256 CUs (scratch/ls1_ab.py, profiles/r04_ls1_ab.txt) —
// LSTM-64 from 2048 streams (4096: 306 us against 417 on k_mfma_lp, 16 384: 1 228 against 1 609 on k_mfma), LSTM-80 / GRU-80 from
// 1024 (4096: 540 / 458 against 716 / 669), LSTM-40 beyond 4096 (8192: 427 against 526), 32 units beyond 6144 (8192: 286 / 248
// against 345 / 289 on k_quad). GRU-40 / 64 have k_gru_gs (190 us per round of 4096 streams against 244 .. 275 here); 16 units never.
// (A GRU-80 pool this rule sends to the matrix-core forms runs k_gru_gs<5, 2> — 324 us per 4096 streams against 436 here — and LSTM-40 / 64
// have k_lstm_gs, below; k_mfma_ls1 then serves LSTM-80, 32 units at many streams, and the A/B runs.)
// Round 5 (profiles/r05_blocklen_forms*.txt: the table re-measured at 64- and 128-frame blocks, what a host's period really is): the
// crossovers hold at every block length but two, both wrong at 256 frames too — see many_streams_form — and ONE moves with the block:
// LSTM-32 at 5632 .. 6144 streams is k_mfma_ls1's from 192-frame blocks (268 against 278 us on k_nn), k_nn's below (84 / 149 us at 64 /
// 128 frames against 93 / 152). `max_frames` is the pool's block length.
inline bool lone_split_pays(int cell, int hidden, uint32_t n, int cus, uint32_t max_frames, const FormHooks& h)
{
    if (h.lp_split == '0' || cus <= 0) return false;
    const bool lstm = cell == AIDAX_CELL_LSTM;
    const uint32_t groups = (n + kMfmaStreams - 1) / kMfmaStreams, c = static_cast<uint32_t>(cus);
    switch (hidden) {
    case 32: return groups * 2 > c * 3 || (lstm && max_frames >= 192 && groups * 8 >= c * 11);
    case 40: return lstm && groups > c;
    case 64: return lstm && groups * 2 > c;
    case 80: return groups * 4 > c;
    default: return false;
    }
}

// ... and k_lstm_gs (k_gru_gs's structure for one-layer LSTMs: unit-major tiles, a main wave per 16 units, the chain on helper
// waves): LSTM-64 265 us per round of 4096 streams — ahead of k_quad from 1025 streams on (289 us at 2048) and of k_mfma_ls1
// throughout (308 / 616 / 1 234 us at 4096 / 8192 / 16 384 against 265 / 528 / 1 057); LSTM-40 265 us, between k_quad (223 us at
// 2048) and k_mfma_ls1 (two workgroups per CU: 418 us at 8192 against 527) — profiles/r04_ls1_ab.txt. AIDAX_LSTM_GS=0 / 1: never / wherever it serves
// (LSTM-80 is served too — five main waves, two helpers — but only 4 % ahead of k_mfma_ls1, 483 against 503 us per 4096 streams: not in the rule).
// (The block length moves nothing here; the argument keeps the three rules' signatures alike.)
inline bool lstm_gs_pays(int cell, int hidden, uint32_t n, int cus, uint32_t /*max_frames*/, const FormHooks& h)
{
    if (cell != AIDAX_CELL_LSTM || (hidden != 40 && hidden != 64 && hidden != 80) || h.lstm_gs == 0 || h.gru_gm == 'f') return false;
    if (h.lstm_gs == 1) return true;
    if (cus <= 0) return false;
    const uint32_t groups = (n + kMfmaStreams - 1) / kMfmaStreams, c = static_cast<uint32_t>(cus);
    return hidden == 64 ? groups * 4 > c : hidden == 80 ? false : groups * 2 > c && groups <= c;
}

inline ManyForm many_streams_form(int cell, int hidden, uint32_t n, int cus, uint32_t max_frames, const FormHooks& h)
{
    if (lstm_gs_pays(cell, hidden, n, cus, max_frames, h)) return MANY_MFMA;
    const bool lstm = cell == AIDAX_CELL_LSTM;
    const uint32_t groups = (n + kMfmaStreams - 1) / kMfmaStreams, c = static_cast<uint32_t>(cus);      // (c is read behind cus > 0 only)
    if (h.ls1 != 0 && lone_split_pays(cell, hidden, n, cus, max_frames, h)) return MANY_MFMA;
    // Round 5: LSTM-32 between one and one and a half rounds of stream groups (4097 .. 6144 streams on 256 CUs) was k_quad's by the
    // rule below — which nothing measured there ever supported: k_nn (the split form) is 5 .. 16 % ahead of it at every block length
    // (5120 streams: 77 / 135 / 249 us at 64 / 128 / 256 frames against 84 / 146 / 271), and k_mfma_ls1 takes over above (lone_split_pays).
    if (lstm && hidden == 32 && cus > 0 && groups > c && groups * 2 <= c * 3) return MANY_NONE;
    const bool full_round = cus > 0 && groups <= c && groups * 8 > c * 7;
    if (full_round && (hidden == 32 || hidden == 64 || (hidden == 40 && lstm))) return MANY_MFMA;
    // One-layer GRUs of 40 (run as 48) / 64 units have k_gru_gm (gate-major tiles: three quarters of the matrix-core work,
    // the whole run() in one launch; up to two workgroups per CU): GRU-64 326 us flat up to 4096 streams, 595 us at 8192,
    // 1 140 us at 16384 against 257 / 408 / 859 us for k_nn at 2048 / 3072 / 8192; GRU-40 277-287 us up to 4096 against
    // 300 (k_nn) / 278 (k_quad) at 3072 and 303 (k_quad) at 4096, 492 / 562 at 8192.
    // Round 4: with the recurrent product on the bf16 matrix pipe (k_gru_gs) the kernel costs 190 us (GRU-64) / 186 us (GRU-40) per
    // 256-frame block whatever the stream count up to a full round, and the crossovers moved (scratch/gs_threshold.py,
    // profiles/r04_gs_threshold.txt): GRU-64 wins from 256 streams on (k_quad 197 us at 256 - 1024, k_nn 225 at 1536 - 2048);
    // GRU-40 from the point where k_nn needs a second round of waves (2048 streams: 174 us; 2560: 279). AIDAX_GRU_GM=f32 (the
    // fp32 MFMA kernel, 305 us) keeps round 3's thresholds.
    // Round 5: GRU-64 is k_gru_gs's at EVERY pool size, the one-stream pool of an LV2 instance included — 49.9 / 93.1 / 179 us per block
    // of 64 / 128 / 256 frames at one stream against 55.4 / 99.1 / 187 on k_quad, 54 / 99 / 188 against 64 / 108 / 197 at 16 .. 192 streams
    // (the 256-stream threshold of round 4 was measured at 256 frames only, where the gap is 4 %; at a 64-frame period it is 19 %).
    // Round 6 (advisor): that evidence is blocks of 64 frames and more; a pool created for shorter blocks than any measured (hub mode's
    // four-frame placeholder pool) keeps round 4's threshold — a sixteenth of a round of stream groups (256 streams on 256 CUs).
    if (!lstm && cus > 0 && h.gru_gm != 'f' && ((hidden == 64 && (max_frames >= 64 || groups * 16 >= c)) || (hidden == 40 && groups * 2 > c))) return MANY_MFMA;
    if (!lstm && cus > 0 && ((hidden == 64 && groups * 8 >= c * 5) || (hidden == 40 && groups * 8 >= c * 7))) return MANY_MFMA;
    // What is left of the table, in ROUNDS of stream groups like the rules above (round 6: these were stream counts measured on 256 CUs —
    // 4096 streams = one round of sixteen-stream workgroups there; a partition with 32 or 64 CUs reaches its round at 512 or 1024
    // streams). A device whose CU count is unknown (cus <= 0) is taken for the one the table was measured on.
    const uint32_t round = static_cast<uint32_t>(kMfmaStreams) * (cus > 0 ? c : 256u);      // streams of one round of workgroups
    if (hidden <= 32) return n >= round ? MANY_QUAD : MANY_NONE;
    if (hidden == 40) return n >= 2 * round ? MANY_MFMA : n >= (lstm ? round / 8 : round) ? MANY_QUAD : MANY_NONE;
    if (hidden == 64 && !lstm) return n >= 4 * round ? MANY_MFMA : n <= round / 4 ? MANY_QUAD : MANY_NONE;
    // LSTM-64, LSTM-80, GRU-80: their one-wave kernels hold 250-500 weight registers; k_quad is 1.35-1.75x
    // faster already at 64 streams, k_mfma takes over from a full round of stream groups
    return n >= round ? MANY_MFMA : MANY_QUAD;
}

// ---- the per-load decision, in two stages: the descriptors of stage 2 come out of the packers, which stage 1 chooses ----
struct LoadPool {
    uint32_t n_streams, max_frames;
    int cus;
    Force force;
    bool packed_fits;            // the packed chains' eight rows of max_frames fit their LDS (chain_lds_bytes <= kChainLdsLimit)
};
struct ModelShape {
    int cell, hidden, n_rnn;
    bool conv, stack;            // is_conv_model, is_stack_model
    bool table_kernel;           // the kernel table has the (cell, hidden) pair
    bool mfma_fits;              // mfma_form_fits: recurrent layers of one width <= 128
};
enum class LoadKind : uint8_t { Table, Stack, Conv, Mfma, Quad };      // (ModelSlot::Kind, by name)

// Stage 1, the kind of slot. Models of the reference's table go to the matrix-core kernels by many_streams_form; AIDAX_KERNEL=quad|mfma
// force one, every other forced form none. quad_lds_ok: k_quad's LDS for the pool's block fits a CU.
inline LoadKind load_kind(const LoadPool& p, const FormHooks& h, const ModelShape& m, bool quad_lds_ok)
{
    if (m.conv) return LoadKind::Conv;
    const ManyForm many = p.force == Force::Quad ? MANY_QUAD : p.force == Force::Mfma ? MANY_MFMA
                        : p.force == Force::None ? many_streams_form(m.cell, m.hidden, p.n_streams, p.cus, p.max_frames, h) : MANY_NONE;
    if (m.n_rnn == 1 && m.table_kernel && many == MANY_QUAD && p.packed_fits && quad_lds_ok) return LoadKind::Quad;
    if (m.mfma_fits && p.packed_fits && (m.stack ? p.force != Force::Valu : many == MANY_MFMA)) return LoadKind::Mfma;
    return m.stack ? LoadKind::Stack : LoadKind::Table;
}

// Stage 2, conv stacks: the family first ...
struct ConvFamily {
    bool mfma, ms;               // on the matrix cores at all; as bf16 term products (k_conv_ms: the stream's state is in ITS layout — ConvDesc::ms_state_floats)
    bool clear_st;               // ConvDesc::st_ok goes to 0: no k_conv_st for this load
    bool refused;                // k_conv it would be, and the pool's max_frames is too large for its LDS activation planes
    bool by_size;                // neither the block length nor a hook settles `fused`: conv_form reads the family's resident-stream count
};
// convm_lds_ok: k_conv_mfma's LDS for a block of the extension kernels' chunk fits a CU; ms_ok: k_conv_ms admits the stack; conv_lds_ok: k_conv's
// planes for max_frames fit. The stacks k_conv_ms admits run there (the contraction as bf16 term products: BASELINE cfg4 60 -> see
// profiles/r05_cfg4_*); its per-layer histories live in the stream's state in ITS layout, so the choice holds for the life of the model in
// this pool (warm-up, bare-model modes and passes all run the one kernel). Of those, the stacks with a compiled geometry (conv_st_shape)
// take fused blocks of 64 / 128 / 256 frames through k_conv_st, the streaming form on the same state.
inline ConvFamily conv_family(const LoadPool& p, const FormHooks& h, bool convm_lds_ok, bool ms_ok, bool conv_lds_ok)
{
    ConvFamily f{};
    f.mfma = p.force != Force::Valu && convm_lds_ok;
    f.ms = f.mfma && ms_ok && !h.conv_ms_off;
    f.clear_st = h.conv_st_off;
    f.refused = !f.mfma && !conv_lds_ok;
    f.by_size = f.mfma && p.max_frames <= 256 && h.conv_fused < 0;
    return f;
}
// ... then whether the chain passes run inside the conv launch: while every workgroup of the pool is resident at once (their serial
// latency is then paid once per block; in a second round of workgroups it would be paid again, and the packed k_chain launches around
// the kernel are cheaper). Long blocks go through in time slices: the one-launch form only. AIDAX_CONV_FUSED=1 / 0 forces the form.
// resident_streams: workgroups of the family's fused form (k_conv_ms with the stack's k_conv_st, or k_conv_mfma) resident at once — an
// occupancy query, asked where f.by_size only.
inline SlotForm conv_form(const ConvFamily& f, const LoadPool& p, const FormHooks& h, int resident_streams)
{
    const bool fused = f.mfma && (p.max_frames > 256 || (h.conv_fused >= 0 ? h.conv_fused != 0 : static_cast<int>(p.n_streams) <= resident_streams));
    return f.ms ? SlotForm::conv_ms(fused) : f.mfma ? SlotForm::conv_mfma(fused) : SlotForm::conv();
}

// Stage 2, the matrix-core forms of recurrent models. *_serves: the kernel has an instantiation for the descriptor; *_lds_ok: its LDS for the
// pool's block fits a CU (160 KiB) — asked of the kernels it serves only.
struct MfmaFacts {
    int n_layers, hidden, cell0;      // MfmaDesc: layers, the padded width, layer 0's cell
    bool lp_serves, lp_fused_serves, ls_serves, ls_fused_serves, gru_gm_serves, gru_gs_serves, lstm_gs_serves;
    bool lp_lds_ok, lp_fused_lds_ok, ls_lds_ok, ls_fused_lds_ok, gru_gm_lds_ok, gru_gs_lds_ok, lstm_gs_lds_ok;
};
// lp: the model gets a hand-over ring (and, stacked, a hold on the device's LpGate) — k_mfma_ls's for ring_streams streams where ls, else k_mfma_lp's
struct MfmaChoice { SlotForm form; bool lp, ls; uint32_t ring_streams; };

inline MfmaChoice mfma_form(const LoadPool& p, const FormHooks& h, const ModelShape& m, const MfmaFacts& f)
{
    // Stacked model: one workgroup per (16 streams, layer), chained through a ring in global memory — where that adds
    // parallelism, i.e. while every (group, layer) workgroup gets a CU of its own (2048 streams for two layers on 256
    // CUs: 1.9x over one workgroup per group; beyond, where the CUs are full either way, a second round of workgroups
    // costs what the resident weights save: 4096 streams 2.49 against 2.45 ms). AIDAX_MFMA_LP=1 / 0 forces it on / off.
    const size_t groups = (p.n_streams + kMfmaStreams - 1) / kMfmaStreams, cus = static_cast<size_t>(p.cus), layers = static_cast<size_t>(f.n_layers > 0 ? f.n_layers : 1);
    // (one-layer models of <= 48 units in the one-launch form: also in several rounds of workgroups — nothing waits for anything,
    // and LSTM-40 at 8192 streams measures 521 us against 583 us for k_mfma; profiles/r03_cfg3_forms.txt)
    const bool lp_rounds_ok = f.n_layers == 1 && f.hidden <= 48 && f.lp_fused_serves;
    // (a one-layer model has no hand-over and nothing to wait for: no hold on the device's gate needed)
    const bool chained = f.n_layers >= 2;
    // Round 4: k_mfma_ls is fast enough to pay in SEVERAL rounds too — a pass over more streams than one resident grid holds goes
    // out as one launch per range of streams (each a resident, cooperative grid; same ring, the counters are per group):
    // LSTM-96 x 2 at 4096 streams 2 x 0.71 ms against 2.48 ms on k_mfma, at 16 384 streams 8 x 0.71 against 9.42 ms.
    // (a lone layer on k_mfma_ls: AIDAX_LS1=1 / 0 forces it on / off)
    const bool ls1 = !chained && (h.ls1 >= 0 ? h.ls1 != 0 : lone_split_pays(m.cell, m.hidden, p.n_streams, p.cus, p.max_frames, h));
    const bool ls_ok = (chained || ls1) && f.ls_serves && h.lp_split != '0' && f.ls_lds_ok;
    const size_t round_groups = h.round_groups > 0 ? static_cast<size_t>(h.round_groups) : cus / layers / 8 * 8;      // workgroup ids come in eights
    // ... where k_mfma_ls's time per resident grid beats k_mfma's rate on a full chip (profiles/r04_ls_rounds_ab.txt): 64 units and
    // more — LSTM-96 x 2 x1.65 / GRU-96 x 2 x1.64, 64 units x 2 x1.17..1.19, x 3 x1.10..1.16, GRU-80 x1.03; below 64 units k_mfma
    // wins by x1.4..1.65, and LSTM-80 (the four-wave geometry) pays up to two grids' worth of streams only
    const bool ranges_pay = h.round_groups_set || (f.hidden >= 64 && (f.hidden != 80 || f.cell0 != 0 || groups <= cus));
    const bool ls_rounds = ls_ok && ranges_pay && round_groups >= (h.round_groups_set ? 1u : 8u) && groups > round_groups && h.mfma_lp != 1;
    // (the grid a chained launch asks for: workgroup ids come in eights, so the group count is rounded up — the padded workgroups return
    // at once, but a cooperative launch counts them: 85 groups x 3 layers are 264 workgroups, not 255)
    const size_t lp_blocks = (groups + 7) / 8 * 8 * static_cast<size_t>(f.n_layers);
    const bool lp_pays = h.mfma_lp >= 0 ? h.mfma_lp != 0 : (lp_rounds_ok || ls_rounds || (ls_ok && !chained) || lp_blocks <= cus);
    MfmaChoice r{};
    r.lp = f.lp_serves && lp_pays && f.lp_lds_ok;
    // stacked models whose split fragments fit the register file: the same hand-over with the contractions on the bf16 matrix
    // pipe (k_mfma_ls; AIDAX_LP_SPLIT=0: the fp32 kernel, =9: every term product instead of six — A/B runs)
    r.ls = r.lp && ls_ok;
    r.ring_streams = r.ls && ls_rounds ? static_cast<uint32_t>(round_groups) * kMfmaStreams : p.n_streams;
    const bool fused = !h.lp_fused_off && (r.ls ? f.ls_fused_serves && f.ls_fused_lds_ok : f.lp_fused_serves && f.lp_fused_lds_ok);
    // one-layer models, the whole run() in one launch: k_lstm_gs; k_gru_gs (80 units: the split kernel only) ahead of the fp32 k_gru_gm
    // (such a slot still gets the ring and counters of `lp`, which no pass of its form can use — a one-layer GRU on k_gru_gs is one:
    // allocation as it was, left for a change of its own)
    if (f.lstm_gs_serves && lstm_gs_pays(m.cell, m.hidden, p.n_streams, p.cus, p.max_frames, h) && f.lstm_gs_lds_ok) r.form = SlotForm::lstm_gs(h.gs_products);
    else if (f.gru_gs_serves && h.gru_gm == 0 && f.gru_gs_lds_ok) r.form = SlotForm::gru_gs(h.gs_products);
    else if (f.gru_gm_serves && h.gru_gm != '0' && f.gru_gm_lds_ok) r.form = SlotForm::gru_gm();
    else r.form = r.ls ? SlotForm::ls(h.lp_split == '9' ? 9 : 6, fused, ls_rounds ? r.ring_streams : 0u) : r.lp ? SlotForm::lp(fused) : SlotForm::mfma();
    return r;
}

}  // namespace aidax
