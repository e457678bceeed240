// form_harness.cpp — the two form decisions as a plain host program, built with ASan + UBSan by `make asan_form` and run by
// tests/test_pass_form_host.py: the pass-form decision (csrc/aidax_pass_form.h: resolve_pass) and the load-form decision
// (csrc/aidax_load_form.h: load_kind, conv_family / conv_form, mfma_form). Each in two parts:
//   (a) a literal table of rows, facts -> decision. Every row restates what the hand-written code did before it became one function; the
//       comment on a row names the lines it was read from. Pass form: facts -> (kernel, chains around, carries event / word, pieces, in place,
//       name), from commit 784ca42. Load form: facts -> (kind; SlotForm fields, lp, ls, ring_streams; refusal), from commit 65d3f83.
//       (pool.h = csrc/aidax_pool.h, pool.cpp = csrc/aidax_pool.cpp, model.cpp = csrc/aidax_pool_model.cpp of the commit named.)
//   (b) properties over the whole product of small inputs (pass form: on the 18 cells of the kernel table with their presence bits restated here).
// It reads no oracle of itself: every expectation is written out below.
#include <cstdio>
#include <cstring>
#include <initializer_list>

#include "aidax_load_form.h"
#include "aidax_pass_form.h"

using namespace aidax;
using K = PassKern;

namespace {

int failures = 0;
long checks = 0;

// The kernel table's 18 cells, restated: which optional forms exist (csrc/aidax_kernels.hip, kTable). LSTM-64 has the split form only,
// LSTM-80 nothing but its one-wave kernel; k_*_pipe4 serves plain models of the cells it measured ahead on, conditioned ones up to 32 units.
struct Cell { int cell, hidden; CellKernels has; };
#define NAMES(c, H) "k_" #c "<" #H ">", "k_" #c "_pipe<" #H ">", "k_chain+k_nn<" #c #H ">", "k_" #c "_pipe4<" #H ">", "k_" #c "_pipe_bank<" #H ">"
const Cell kCells[18] = {
    { 0, 8, { true, true, true, true, true, NAMES(lstm, 8) } },    { 0, 12, { true, true, true, true, true, NAMES(lstm, 12) } },
    { 0, 16, { true, true, true, true, true, NAMES(lstm, 16) } },  { 0, 20, { true, true, true, true, true, NAMES(lstm, 20) } },
    { 0, 24, { true, true, false, true, true, NAMES(lstm, 24) } }, { 0, 32, { true, true, true, true, true, NAMES(lstm, 32) } },
    { 0, 40, { true, true, false, false, true, NAMES(lstm, 40) } },
    { 0, 64, { false, true, false, false, false, "k_lstm<64>", "-", "k_chain+k_nn<lstm64>", "-", "-" } },
    { 0, 80, { false, false, false, false, false, "k_lstm<80>", "-", "-", "-", "-" } },
    { 1, 8, { true, true, true, true, true, NAMES(gru, 8) } },     { 1, 12, { true, true, true, true, true, NAMES(gru, 12) } },
    { 1, 16, { true, true, true, true, true, NAMES(gru, 16) } },   { 1, 20, { true, true, false, true, true, NAMES(gru, 20) } },
    { 1, 24, { true, true, true, true, true, NAMES(gru, 24) } },   { 1, 32, { true, true, false, true, true, NAMES(gru, 32) } },
    { 1, 40, { true, true, false, false, true, NAMES(gru, 40) } }, { 1, 64, { true, true, false, false, true, NAMES(gru, 64) } },
    { 1, 80, { true, true, false, false, true, NAMES(gru, 80) } },
};
const CellKernels* cell(int c, int hidden)
{
    for (const Cell& e : kCells)
        if (e.cell == c && e.hidden == hidden) return &e.has;
    return nullptr;
}
const CellKernels *LSTM24 = cell(0, 24), *LSTM32 = cell(0, 32), *LSTM64 = cell(0, 64), *LSTM80 = cell(0, 80), *GRU20 = cell(1, 20);

PoolFacts pool(uint32_t streams, uint32_t max_frames = 256, int cus = 256, Force force = Force::None)
{
    return PoolFacts{ streams, max_frames, cus, force, false, -1, false, false, true };
}
// a MODE_CHAIN pass over the whole pool unless said
PassFacts pass(const PoolFacts& p, SlotForm slot, const CellKernels* has, uint32_t n_frames, int input_size = 1, int mode = MODE_CHAIN)
{
    return PassFacts{ slot, has, mode, n_frames, p.n_streams, input_size, true, false, false, false };
}
PoolFacts with_bank(PoolFacts p) { p.bank = true; return p; }
PoolFacts with_lp_off(PoolFacts p) { p.lp_off = true; return p; }
PoolFacts unpacked(PoolFacts p) { p.packed_fits = false; return p; }
PoolFacts pipe4_off(PoolFacts p) { p.pipe4_off = true; return p; }
PoolFacts pipe4_min(PoolFacts p, int n) { p.pipe4_min = n; return p; }
PassFacts ring(PassFacts f, bool hand_over) { f.ring_ready = true; f.hand_over = hand_over; return f; }
PassFacts st(PassFacts f) { f.conv_st = true; return f; }
PassFacts of_streams(PassFacts f, uint32_t n) { f.n_streams = n; return f; }

const SlotForm kNone;
const SlotForm kPipeTable = SlotForm::table(512, true, false);      // 512 streams resident on the pipeline, the split form pays beyond
const SlotForm kWaveTable = SlotForm::table(0, false, false);

struct Want { K kern; bool chains, event, word; PassForm::Pieces pieces; bool in_place; const char* name; };      // name nullptr: the old code had no name for it
void row(int line, const PoolFacts& p, const PassFacts& f, const Want& w)
{
    const PassForm r = resolve_pass(p, f);
    ++checks;
    const bool ok = r.kern == w.kern && r.chains == w.chains && r.carries_event == w.event && r.carries_word == w.word && r.pieces == w.pieces &&
                    r.host_in_place == w.in_place && r.name && (!w.name || std::strcmp(r.name, w.name) == 0);
    if (ok) return;
    ++failures;
    std::printf("row at line %d: got kern %d chains %d event %d word %d pieces %d in_place %d name %s\n", line, (int)r.kern, r.chains, r.carries_event, r.carries_word,
                (int)r.pieces, r.host_in_place, r.name ? r.name : "(null)");
}
#define ROW(p, f, ...) row(__LINE__, p, f, Want{ __VA_ARGS__ })
constexpr PassForm::Pieces WHOLE = PassForm::WHOLE, SLICES = PassForm::TIME_SLICES, RANGES = PassForm::STREAM_RANGES;

void rows()
{
    // ---- no model
    { const PoolFacts p = pool(3);      // pool.h:260 (fewer than 64 streams: form 0), pool.cpp:311 (k_nomodel), pool.h:285, model.cpp:524
      ROW(p, pass(p, kNone, nullptr, 256), K::NoModel, false, false, false, WHOLE, true, "k_nomodel"); }
    { const PoolFacts p = pool(64);     // the split form needs no model — pool.h:261 (form 2), pool.cpp:310, pool.h:285 (not in place); model.cpp:524 still says k_nomodel
      ROW(p, pass(p, kNone, nullptr, 256), K::Nn, true, false, false, WHOLE, false, "k_nomodel");
      ROW(unpacked(p), pass(p, kNone, nullptr, 256), K::NoModel, false, false, false, WHOLE, true, "k_nomodel");      // pool.h:260 (!packed_fits)
      ROW(p, pass(p, kNone, nullptr, 2048, 1, MODE_WARMUP), K::NoModel, false, false, false, WHOLE, true, nullptr); }  // pool.cpp:298 (form 0 outside MODE_CHAIN)
    { const PoolFacts p = pool(3, 256, 256, Force::Split);      // pool.h:258 (forced split, no model: form 2)
      ROW(p, pass(p, kNone, nullptr, 64), K::Nn, true, false, false, WHOLE, false, "k_nomodel"); }
    // ---- table slots: one wave, the pipeline, pipe4
    { const PoolFacts p = pool(8);      // pool.h:279 (pipe_capacity 0), :260; pool.cpp:311; model.cpp:536 (name)
      ROW(p, pass(p, kWaveTable, LSTM64, 256), K::Wave, false, false, false, WHOLE, true, "k_lstm<64>"); }
    { const PoolFacts p = pool(3);      // pool.h:259 (pipeline), :311 (fewer than four streams of a plain model: no pipe4); pool.cpp:304-307: event yes, word no (three streams, :284)
      ROW(p, pass(p, kPipeTable, LSTM32, 256), K::Pipe, false, true, false, WHOLE, true, "k_lstm_pipe<32>");
      ROW(pipe4_min(p, 1), pass(p, kPipeTable, LSTM32, 256), K::Pipe4, false, true, false, WHOLE, true, "k_lstm_pipe4<32>"); }      // pool.h:307 (AIDAX_PIPE4_MIN)
    { const PoolFacts p = pool(8);      // pool.h:311-312, pool.cpp:308, model.cpp:535
      ROW(p, pass(p, kPipeTable, LSTM32, 256), K::Pipe4, false, true, false, WHOLE, true, "k_lstm_pipe4<32>");
      ROW(p, pass(p, kPipeTable, LSTM32, 33), K::Pipe, false, true, false, WHOLE, true, "k_lstm_pipe<32>");            // pool.h:311 (n % 16)
      ROW(p, pass(p, kPipeTable, LSTM32, 0), K::Pipe, false, true, false, WHOLE, true, "k_lstm_pipe<32>");             // pool.h:311 (n == 0: pipe4 never)
      ROW(pipe4_off(p), pass(p, kPipeTable, LSTM32, 256), K::Pipe, false, true, false, WHOLE, true, "k_lstm_pipe<32>"); // pool.h:310 (AIDAX_PIPE4=0)
      ROW(p, pass(p, kPipeTable, LSTM24, 256), K::Pipe, false, true, false, WHOLE, true, "k_lstm_pipe<24>");           // pool.h:311 (a plain LSTM-24 has no fn_pipe4)
      ROW(p, pass(p, kPipeTable, LSTM24, 256, 2), K::Pipe4, false, true, false, WHOLE, true, "k_lstm_pipe4<24>");      // ... a conditioned one has fn_pipe4c
      ROW(p, pass(p, kPipeTable, LSTM32, 256, 1, MODE_WARMUP), K::Wave, false, false, false, WHOLE, true, nullptr);     // pool.cpp:298, :311 (one-wave kernel, lds_bytes(m, 0))
      ROW(p, pass(p, kPipeTable, LSTM32, 256, 1, MODE_NN_ONLY), K::Wave, false, false, false, WHOLE, true, nullptr);
      PassFacts small_lds = pass(p, kPipeTable, LSTM32, 256); small_lds.pipe4_lds_ok = false;                           // pool.h:312 (LDS)
      ROW(p, small_lds, K::Pipe, false, true, false, WHOLE, true, "k_lstm_pipe<32>"); }
    { const PoolFacts p = pool(2048, 256, 256);      // pool.h:312: 512 workgroups on 256 CUs — no pipe4; (capacity 4096: still the pipeline)
      ROW(p, pass(p, SlotForm::table(4096, true, false), LSTM32, 256), K::Pipe, false, true, false, WHOLE, true, "k_lstm_pipe<32>"); }
    { const PoolFacts p = pool(1);      // the LV2 instance's pool. pool.cpp:284: the word goes with a one-stream pass of n > 0
      ROW(p, pass(p, kPipeTable, LSTM32, 64), K::Pipe, false, true, true, WHOLE, true, "k_lstm_pipe<32>");             // pool.h:307 (a plain model: four streams at least)
      ROW(p, pass(p, kPipeTable, GRU20, 64, 3), K::Pipe4, false, true, true, WHOLE, true, "k_gru_pipe4<20>");          // ... a conditioned model: any pool
      ROW(p, pass(p, kPipeTable, GRU20, 0, 3), K::Pipe, false, true, false, WHOLE, true, "k_gru_pipe<20>");            // pool.cpp:284 (n == 0: the word is never handed down)
      ROW(p, pass(p, kWaveTable, LSTM80, 64), K::Wave, false, false, false, WHOLE, true, "k_lstm<80>"); }
    // ---- the bank
    { const PoolFacts p = with_bank(pool(8));      // pool.cpp:291-296, pool.h:284, model.cpp:532
      ROW(p, pass(p, kPipeTable, LSTM32, 256), K::PipeBank, false, true, false, WHOLE, true, "k_lstm_pipe_bank<32>");
      ROW(with_bank(pool(2048)), pass(pool(2048), kPipeTable, LSTM32, 256), K::PipeBank, false, true, false, WHOLE, true, "k_lstm_pipe_bank<32>");      // (whatever form the pool model alone would take)
      ROW(with_bank(pool(1)), pass(pool(1), kPipeTable, LSTM32, 64), K::PipeBank, false, true, true, WHOLE, true, "k_lstm_pipe_bank<32>"); }
    // ---- the bank and a slot that is no table slot: the kind's own kernel and name (pool.cpp:201-276 and model.cpp:526-531 come before the bank's
    // lines, pool.cpp:291 and model.cpp:532), and in place all the same (pool.h:284 comes first). No model: model.cpp:524 comes first too.
    { const PoolFacts p = with_bank(pool(8));
      ROW(p, pass(p, SlotForm::mfma(), nullptr, 256), K::Mfma, true, false, false, WHOLE, true, "k_chain+k_mfma");
      ROW(p, pass(p, SlotForm::gru_gs(6), nullptr, 256), K::GruGs, false, false, false, WHOLE, true, "k_gru_gs");
      ROW(p, ring(pass(p, SlotForm::ls(6, true, 0), nullptr, 256), true), K::MfmaLs, false, false, false, WHOLE, true, "k_mfma_ls");
      ROW(p, pass(p, SlotForm::quad(), nullptr, 256), K::Quad, true, false, false, WHOLE, true, "k_chain+k_quad");
      ROW(p, pass(p, SlotForm::stack(), nullptr, 256), K::Stack, false, false, false, WHOLE, true, "k_stack");
      ROW(p, pass(p, SlotForm::conv_mfma(false), nullptr, 256), K::ConvMfma, true, false, false, WHOLE, true, "k_chain+k_conv_mfma");
      ROW(p, pass(p, kNone, nullptr, 256), K::NoModel, false, false, false, WHOLE, true, "k_nomodel");
      ROW(with_bank(pool(64)), pass(pool(64), kNone, nullptr, 256), K::Nn, true, false, false, WHOLE, true, "k_nomodel"); }
    // ---- many streams
    { const PoolFacts p = pool(1024);   // pool.h:259-261
      ROW(p, pass(p, kPipeTable, LSTM32, 256), K::Nn, true, false, false, WHOLE, false, "k_chain+k_nn<lstm32>");       // pool.h:287 (not in place)
      ROW(p, pass(p, SlotForm::table(512, false, false), LSTM32, 256), K::Wave, false, false, false, WHOLE, true, "k_lstm<32>");
      ROW(unpacked(p), pass(p, kPipeTable, LSTM32, 256), K::Wave, false, false, false, WHOLE, true, "k_lstm<32>"); }
    { const PoolFacts p = pool(63);     // pool.h:260 (fewer than 64 streams), beyond the pipeline's capacity
      ROW(p, pass(p, SlotForm::table(32, true, false), LSTM32, 256), K::Wave, false, false, false, WHOLE, true, "k_lstm<32>"); }
    // ---- AIDAX_KERNEL
    { ROW(pool(8, 256, 256, Force::Wave), pass(pool(8), kPipeTable, LSTM32, 256), K::Wave, false, false, false, WHOLE, true, "k_lstm<32>");                // pool.h:255
      ROW(pool(1024, 256, 256, Force::Pipe), pass(pool(1024), kPipeTable, LSTM32, 256), K::Pipe, false, true, false, WHOLE, true, "k_lstm_pipe<32>");      // pool.h:256, :311 (forced: no pipe4)
      ROW(pool(8, 256, 256, Force::Pipe), pass(pool(8), kPipeTable, LSTM32, 256), K::Pipe, false, true, false, WHOLE, true, "k_lstm_pipe<32>");
      ROW(pool(8, 256, 256, Force::Pipe), pass(pool(8), kWaveTable, LSTM64, 256), K::Wave, false, false, false, WHOLE, true, "k_lstm<64>");                // pool.h:256 (no fn_pipe)
      ROW(pool(8, 256, 256, Force::Split), pass(pool(8), kPipeTable, LSTM32, 256), K::Nn, true, false, false, WHOLE, false, "k_chain+k_nn<lstm32>");       // pool.h:258
      ROW(pool(8, 256, 256, Force::Split), pass(pool(8), kWaveTable, LSTM80, 256), K::Wave, false, false, false, WHOLE, true, "k_lstm<80>");               // pool.h:258 (no fn_nn)
      ROW(unpacked(pool(8, 4096, 256, Force::Split)), pass(pool(8), kPipeTable, LSTM32, 256), K::Wave, false, false, false, WHOLE, true, "k_lstm<32>");    // pool.h:257-258
      ROW(pool(8, 256, 256, Force::Q4), pass(pool(8), SlotForm::table(512, true, true), LSTM32, 256), K::Q4, false, false, false, WHOLE, true, "k_lstm_q4<32>");      // pool.h:254, pool.cpp:299-303, model.cpp:536
      ROW(pool(8, 256, 256, Force::Q4), pass(pool(8), SlotForm::table(512, true, true), LSTM32, 0), K::Q4, false, false, false, WHOLE, true, "k_lstm_q4<32>");
      ROW(pool(8, 256, 256, Force::Q4), pass(pool(8), kPipeTable, GRU20, 256), K::Pipe, false, true, false, WHOLE, true, "k_gru_pipe<20>");                // pool.h:254 (no record), :259, :311
      ROW(pool(8, 256, 256, Force::Q4), pass(pool(8), SlotForm::table(512, true, true), LSTM32, 2048, 1, MODE_WARMUP), K::Wave, false, false, false, WHOLE, true, nullptr);      // pool.cpp:298
      ROW(pool(8, 256, 256, Force::Valu), pass(pool(8), kPipeTable, LSTM32, 256), K::Pipe, false, true, false, WHOLE, true, "k_lstm_pipe<32>"); }          // pool.h:259 (valu / mfma / quad: the heuristic), :311
    // ---- k_quad
    { const PoolFacts p = pool(1024);   // pool.cpp:249-252, pool.h:290 (never in place), model.cpp:529
      ROW(p, pass(p, SlotForm::quad(), nullptr, 256), K::Quad, true, false, false, WHOLE, false, "k_chain+k_quad");
      ROW(p, pass(p, SlotForm::quad(), nullptr, 0), K::Quad, true, false, false, WHOLE, false, "k_chain+k_quad");      // pool.cpp:197 (no frames: the two chains, no model kernel)
      ROW(p, pass(p, SlotForm::quad(), nullptr, 2048, 1, MODE_WARMUP), K::Quad, false, false, false, WHOLE, false, nullptr); }      // pool.cpp:250
    // ---- the matrix-core forms of recurrent models
    { const PoolFacts p = pool(1024);
      ROW(p, pass(p, SlotForm::mfma(), nullptr, 256), K::Mfma, true, false, false, WHOLE, false, "k_chain+k_mfma");    // pool.cpp:238, :247; model.cpp:528; pool.h:290
      ROW(p, pass(p, SlotForm::mfma(), nullptr, 256, 1, MODE_NN_ONLY), K::Mfma, false, false, false, WHOLE, false, nullptr);        // pool.cpp:240
      // k_mfma_lp, one launch (a one-layer model) — one launch, and still not in place: pool.cpp:243-244, model.cpp:528, pool.h:290
      ROW(p, ring(pass(p, SlotForm::lp(true), nullptr, 256), false), K::MfmaLp, false, false, false, WHOLE, false, "k_mfma_lp");
      ROW(p, ring(pass(p, SlotForm::lp(true), nullptr, 0), false), K::MfmaLp, true, false, false, WHOLE, false, nullptr);          // pool.cpp:243 (n == 0: not the fused launch), :247, :197
      ROW(p, ring(pass(p, SlotForm::lp(false), nullptr, 256), true), K::MfmaLp, true, false, false, WHOLE, false, "k_chain+k_mfma_lp");      // pool.cpp:234-235
      ROW(p, pass(p, SlotForm::lp(true), nullptr, 256), K::Mfma, true, false, false, WHOLE, false, "k_chain+k_mfma");             // pool.h:294 (no ring, or refused)
      ROW(p, ring(pass(p, SlotForm::lp(true), nullptr, 2048, 1, MODE_WARMUP), true), K::Mfma, false, false, false, WHOLE, false, nullptr);   // pool.cpp:234, :240 (never a chained kernel)
      ROW(with_lp_off(p), ring(pass(p, SlotForm::lp(false), nullptr, 256), true), K::Mfma, true, false, false, WHOLE, false, "k_chain+k_mfma");      // pool.h:294 (lp_off: stacked models)
      ROW(with_lp_off(p), ring(pass(p, SlotForm::lp(true), nullptr, 256), false), K::MfmaLp, false, false, false, WHOLE, false, "k_mfma_lp");       // ... a lone layer keeps it
      // k_mfma_ls: model.cpp:528 (the four spellings, ls1 for a lone layer), pool.cpp:219-232 (ranges)
      ROW(p, ring(pass(p, SlotForm::ls(6, true, 0), nullptr, 256), true), K::MfmaLs, false, false, false, WHOLE, false, "k_mfma_ls");
      ROW(p, ring(pass(p, SlotForm::ls(6, false, 0), nullptr, 256), true), K::MfmaLs, true, false, false, WHOLE, false, "k_chain+k_mfma_ls");
      ROW(p, ring(pass(p, SlotForm::ls(9, true, 0), nullptr, 256), false), K::MfmaLs, false, false, false, WHOLE, false, "k_mfma_ls1");
      ROW(p, ring(pass(p, SlotForm::ls(6, false, 0), nullptr, 256), false), K::MfmaLs, true, false, false, WHOLE, false, "k_chain+k_mfma_ls1");
      ROW(p, ring(pass(p, SlotForm::ls(6, true, 512), nullptr, 256), true), K::MfmaLs, false, false, false, RANGES, false, "k_mfma_ls");    // pool.cpp:220 (1024 streams in ranges of 512)
      ROW(p, of_streams(ring(pass(p, SlotForm::ls(6, true, 512), nullptr, 256), true), 512), K::MfmaLs, false, false, false, WHOLE, false, "k_mfma_ls");      // ... a prefix pass of one range
      // the one-launch kernels of one-layer models: pool.cpp:241-242, model.cpp:527-528, pool.h:290 — one launch, and not in place
      ROW(p, pass(p, SlotForm::gru_gm(), nullptr, 256), K::GruGm, false, false, false, WHOLE, false, "k_gru_gm");
      ROW(p, pass(p, SlotForm::gru_gs(6), nullptr, 256), K::GruGs, false, false, false, WHOLE, false, "k_gru_gs");
      ROW(p, pass(p, SlotForm::lstm_gs(9), nullptr, 256), K::LstmGs, false, false, false, WHOLE, false, "k_lstm_gs");
      ROW(pool(1), pass(pool(1), SlotForm::gru_gs(6), nullptr, 64), K::GruGs, false, false, false, WHOLE, false, "k_gru_gs");   // (the LV2 instance's GRU-64: no event, no word)
      ROW(p, pass(p, SlotForm::gru_gs(6), nullptr, 0), K::Mfma, true, false, false, WHOLE, false, nullptr);                     // pool.cpp:242 (n == 0), :247, :197
      ROW(p, pass(p, SlotForm::lstm_gs(6), nullptr, 0), K::Mfma, true, false, false, WHOLE, false, nullptr);                    // pool.cpp:241
      ROW(p, pass(p, SlotForm::lstm_gs(6), nullptr, 2048, 1, MODE_WARMUP), K::Mfma, false, false, false, WHOLE, false, nullptr); }      // pool.cpp:240 (never a tick kernel)
    // ---- k_stack, and the conv stacks
    { const PoolFacts p = pool(16);
      ROW(p, pass(p, SlotForm::stack(), nullptr, 256), K::Stack, false, false, false, WHOLE, true, "k_stack");                  // pool.cpp:253, pool.h:288, model.cpp:526
      ROW(p, pass(p, SlotForm::stack(), nullptr, 256, 1, MODE_WARMUP), K::Stack, false, false, false, WHOLE, true, nullptr);
      ROW(p, pass(p, SlotForm::conv(), nullptr, 256), K::Conv, false, false, false, WHOLE, true, "k_conv");                     // pool.cpp:276, pool.h:289, model.cpp:531
      ROW(p, pass(p, SlotForm::conv_mfma(true), nullptr, 256), K::ConvMfma, false, false, false, WHOLE, true, "k_conv_mfma");   // pool.cpp:259-263
      ROW(p, pass(p, SlotForm::conv_mfma(true), nullptr, 0), K::ConvMfma, false, false, false, WHOLE, true, "k_conv_mfma");     // pool.cpp:263 (fused: launched also for no frames)
      ROW(p, pass(p, SlotForm::conv_mfma(false), nullptr, 256), K::ConvMfma, true, false, false, WHOLE, false, "k_chain+k_conv_mfma");      // pool.cpp:274, pool.h:289
      ROW(p, pass(p, SlotForm::conv_mfma(false), nullptr, 0), K::ConvMfma, true, false, false, WHOLE, false, "k_chain+k_conv_mfma");        // pool.cpp:197
      ROW(p, pass(p, SlotForm::conv_mfma(true), nullptr, 256, 1, MODE_WARMUP), K::ConvMfma, false, false, false, WHOLE, true, nullptr);     // pool.cpp:258 (unfused, no chains)
      ROW(p, pass(p, SlotForm::conv_ms(true), nullptr, 256), K::ConvMs, false, false, false, WHOLE, true, "k_conv_ms");         // model.cpp:531
      ROW(p, st(pass(p, SlotForm::conv_ms(true), nullptr, 256)), K::ConvMs, false, false, false, WHOLE, true, "k_conv_st");     // model.cpp:530
      ROW(p, st(pass(p, SlotForm::conv_ms(true), nullptr, 33)), K::ConvMs, false, false, false, WHOLE, true, "k_conv_st");      // ... by max_frames, not by the pass
      ROW(p, st(pass(p, SlotForm::conv_ms(false), nullptr, 256)), K::ConvMs, true, false, false, WHOLE, false, "k_chain+k_conv_ms");
      ROW(p, st(pass(p, SlotForm::conv_mfma(true), nullptr, 256)), K::ConvMfma, false, false, false, WHOLE, true, "k_conv_mfma"); }      // (AIDAX_CONV_MS=0 on such a stack)
    { const PoolFacts p = pool(16, 100);    // model.cpp:530: max_frames >= 64, not conv_st_block_ok(100)
      ROW(p, st(pass(p, SlotForm::conv_ms(true), nullptr, 100)), K::ConvMs, false, false, false, WHOLE, true, "k_conv_st");
      ROW(pool(16, 32), st(pass(pool(16, 32), SlotForm::conv_ms(true), nullptr, 32)), K::ConvMs, false, false, false, WHOLE, true, "k_conv_ms"); }
    { const PoolFacts p = pool(16, 512);    // pool.cpp:260-272 (time slices of 256 frames)
      ROW(p, st(pass(p, SlotForm::conv_ms(true), nullptr, 512)), K::ConvMs, false, false, false, SLICES, true, "k_conv_st");
      ROW(p, st(pass(p, SlotForm::conv_ms(true), nullptr, 256)), K::ConvMs, false, false, false, WHOLE, true, "k_conv_st");
      ROW(p, pass(p, SlotForm::conv_mfma(true), nullptr, 257), K::ConvMfma, false, false, false, SLICES, true, "k_conv_mfma");
      ROW(pool(16, 100), pass(pool(16, 100), SlotForm::conv_mfma(true), nullptr, 100), K::ConvMfma, false, false, false, WHOLE, true, "k_conv_mfma"); }
}

void expect(bool ok, const char* what, const PoolFacts& p, const PassFacts& f, const PassForm& r)
{
    ++checks;
    if (ok) return;
    if (++failures <= 20)
        std::printf("property \"%s\": streams %u max_frames %u cus %d force %d bank %d | serve %d mode %d n %u input %d -> kern %d\n", what, p.n_streams, p.max_frames, p.cus,
                    (int)p.force, p.bank, (int)f.slot.serve(), f.mode, f.n_frames, f.input_size, (int)r.kern);
}

void properties()
{
    const Force forces[] = { Force::None, Force::Wave, Force::Pipe, Force::Split, Force::Valu, Force::Mfma, Force::Quad, Force::Q4 };
    for (const Cell& c : kCells)
    for (const Force force : forces)
    for (int mode = 0; mode <= 2; ++mode)
    for (const uint32_t n : { 0u, 15u, 16u, 33u, 64u, 100u, 256u, 2048u })
    for (const uint32_t streams : { 1u, 3u, 4u, 63u, 64u, 1024u, 4096u })
    for (const int cus : { 64, 256 })
    for (int input = 1; input <= 3; ++input)
    for (int bank = 0; bank <= (c.has.bank ? 1 : 0); ++bank)      // (the bank is in force only on a pool model whose cell has its kernel: ModelSlot::arch)
    for (int variant = 0; variant < 4; ++variant) {               // what choose_form may have found: the pipeline's capacity, whether the split form pays, a q4 record
        const SlotForm slot = SlotForm::table(!c.has.pipe ? 0 : variant & 1 ? 8192 : 48, c.has.nn && (variant & 2), c.cell == 0 && c.hidden == 32 && force == Force::Q4 && (variant & 1));
        PoolFacts p = pool(streams, n > 256 ? n : 256, cus, force);
        p.bank = bank != 0;
        p.packed_fits = p.max_frames <= 2048;
        const PassFacts f = pass(p, slot, &c.has, n, input, mode);
        const PassForm r = resolve_pass(p, f);
        const bool has = r.kern == K::Wave || (r.kern == K::Pipe && c.has.pipe) || (r.kern == K::Pipe4 && (input > 1 ? c.has.pipe4c : c.has.pipe4)) ||
                         (r.kern == K::PipeBank && c.has.bank) || (r.kern == K::Nn && c.has.nn) || (r.kern == K::Q4 && slot.q4());
        expect(has, "the kernel is one the entry has", p, f, r);
        expect(r.kern != K::Pipe4 || (n % 16u == 0 && n > 0 && force == Force::None), "pipe4: whole tiles, n > 0, nothing forced", p, f, r);
        expect(!r.host_in_place || !r.chains, "in place implies no chains around", p, f, r);
        expect(!r.carries_word || (streams == 1 && n > 0 && (r.kern == K::Pipe || r.kern == K::Pipe4 || r.kern == K::PipeBank)), "the word: a one-stream pass of n > 0 on pipe, pipe4 or the bank", p, f, r);
        expect(!r.carries_word || r.carries_event, "the word goes with the event", p, f, r);
        expect(r.name != nullptr && r.name[0] == 'k', "a name", p, f, r);
        expect(mode == MODE_CHAIN || bank || r.kern == K::Wave, "outside MODE_CHAIN: the one-wave kernel", p, f, r);
        expect(r.chains == (r.kern == K::Nn) && r.pieces == PassForm::WHOLE, "table slots: chains around the split form only, never in pieces", p, f, r);
    }
    // ... and the same pools without a model
    for (const Force force : forces)
    for (int mode = 0; mode <= 2; ++mode)
    for (const uint32_t n : { 0u, 15u, 16u, 33u, 64u, 100u, 256u, 2048u })
    for (const uint32_t streams : { 1u, 3u, 4u, 63u, 64u, 1024u, 4096u })
    for (const int cus : { 64, 256 }) {
        PoolFacts p = pool(streams, n > 256 ? n : 256, cus, force);
        p.packed_fits = p.max_frames <= 2048;
        const PassFacts f = pass(p, kNone, nullptr, n, 1, mode);
        const PassForm r = resolve_pass(p, f);
        expect(r.kern == K::NoModel || (r.kern == K::Nn && mode == MODE_CHAIN && p.packed_fits), "no model: k_nomodel, or the split form's two chains", p, f, r);
        expect(r.name && std::strcmp(r.name, "k_nomodel") == 0, "no model: the name", p, f, r);
        expect(r.host_in_place == !r.chains && !r.carries_event && !r.carries_word, "no model: in place unless split, no end markers", p, f, r);
    }
}


// ================================================ the load-form decision (aidax_load_form.h) ================================================
// Lines named below are those of commit 65d3f83: model.cpp:39-170 is choose_form, pool.cpp:52-126 the one-layer rule.
using S = SlotForm::Serve;
using LK = LoadKind;

LoadPool lpool(uint32_t streams, uint32_t max_frames = 64, int cus = 256, Force force = Force::None) { return LoadPool{ streams, max_frames, cus, force, true }; }
LoadPool unpacked(LoadPool p) { p.packed_fits = false; return p; }
constexpr int LSTM = AIDAX_CELL_LSTM, GRU = AIDAX_CELL_GRU;
ModelShape one_layer(int cell, int hidden) { return ModelShape{ cell, hidden, 1, false, false, true, true }; }         // a model of the kernel table
ModelShape stacked(int cell, int hidden, int layers) { return ModelShape{ cell, hidden, layers, false, true, false, true }; }
ModelShape wide_layer(int cell, int hidden) { return ModelShape{ cell, hidden, 1, false, true, false, true }; }         // one layer wider than the table: a "stack"
ModelShape conv_stack() { return ModelShape{ AIDAX_CELL_CONV, 16, 8, true, false, false, false }; }
ModelShape unfit(ModelShape m) { m.mfma_fits = false; return m; }

struct Hk {      // FormHooks with one field set
    static FormHooks none() { return FormHooks{}; }
    static FormHooks ls1(int v) { FormHooks h; h.ls1 = v; return h; }
    static FormHooks lstm_gs(int v) { FormHooks h; h.lstm_gs = v; return h; }
    static FormHooks gru_gm(char v) { FormHooks h; h.gru_gm = v; return h; }
    static FormHooks mfma_lp(int v) { FormHooks h; h.mfma_lp = v; return h; }
    static FormHooks lp_split(char v) { FormHooks h; h.lp_split = v; return h; }
    static FormHooks lp_fused_off() { FormHooks h; h.lp_fused_off = true; return h; }
    static FormHooks round_groups(int v) { FormHooks h; h.round_groups_set = true; h.round_groups = v; return h; }
    static FormHooks gs_products(int v) { FormHooks h; h.gs_products = v; return h; }
    static FormHooks conv_ms_off() { FormHooks h; h.conv_ms_off = true; return h; }
    static FormHooks conv_st_off() { FormHooks h; h.conv_st_off = true; return h; }
    static FormHooks conv_fused(int v) { FormHooks h; h.conv_fused = v; return h; }
};
FormHooks also_gru_gm(FormHooks h, char v) { h.gru_gm = v; return h; }
FormHooks also_lp_split(FormHooks h, char v) { h.lp_split = v; return h; }

void kind_row(int line, const LoadPool& p, const FormHooks& h, const ModelShape& m, bool quad_lds_ok, LK want)
{
    ++checks;
    const LK got = load_kind(p, h, m, quad_lds_ok);
    if (got == want) return;
    ++failures;
    std::printf("kind row at line %d: got %d\n", line, (int)got);
}
#define KIND(p, h, m, quad_ok, want) kind_row(__LINE__, p, h, m, quad_ok, want)

struct ConvWant { S serve; bool fused, clear_st, ms_layout, refused, by_size; };
void conv_row(int line, const LoadPool& p, const FormHooks& h, bool convm_lds_ok, bool ms_ok, bool conv_lds_ok, int resident, const ConvWant& w)
{
    ++checks;
    const ConvFamily f = conv_family(p, h, convm_lds_ok, ms_ok, conv_lds_ok);
    const SlotForm s = conv_form(f, p, h, resident);
    if (s.serve() == w.serve && s.fused() == w.fused && f.clear_st == w.clear_st && f.ms == w.ms_layout && f.refused == w.refused && f.by_size == w.by_size &&
        s.products() == 0 && s.round_streams() == 0 && f.mfma == (w.serve != S::Conv)) return;
    ++failures;
    std::printf("conv row at line %d: got serve %d fused %d clear_st %d ms %d refused %d by_size %d\n", line, (int)s.serve(), s.fused(), f.clear_st, f.ms, f.refused, f.by_size);
}
#define CONV(p, h, convm_ok, ms_ok, conv_ok, resident, ...) conv_row(__LINE__, p, h, convm_ok, ms_ok, conv_ok, resident, ConvWant{ __VA_ARGS__ })

// the descriptor of a model that k_mfma_lp and k_mfma_ls serve, fused too, with room in the LDS; none of the one-launch kernels of one-layer models
MfmaFacts chained_facts(int n_layers, int hidden, int cell0) { return MfmaFacts{ n_layers, hidden, cell0, true, true, true, true, false, false, false, true, true, true, true, false, false, false }; }
MfmaFacts with_lstm_gs(MfmaFacts f) { f.lstm_gs_serves = f.lstm_gs_lds_ok = true; return f; }
MfmaFacts with_gru_kernels(MfmaFacts f) { f.gru_gm_serves = f.gru_gm_lds_ok = f.gru_gs_serves = f.gru_gs_lds_ok = true; return f; }
MfmaFacts without(MfmaFacts f, bool MfmaFacts::*fact) { f.*fact = false; return f; }

struct MfmaWant { S serve; bool fused; int products; uint32_t round_streams; bool lp, ls; uint32_t ring_streams; };
void mfma_row(int line, const LoadPool& p, const FormHooks& h, const ModelShape& m, const MfmaFacts& f, const MfmaWant& w)
{
    ++checks;
    const MfmaChoice c = mfma_form(p, h, m, f);
    if (c.form.serve() == w.serve && c.form.fused() == w.fused && c.form.products() == w.products && c.form.round_streams() == w.round_streams && c.lp == w.lp &&
        c.ls == w.ls && c.ring_streams == w.ring_streams && c.form.pipe_capacity() == 0 && !c.form.split_pays() && !c.form.q4()) return;
    ++failures;
    std::printf("mfma row at line %d: got serve %d fused %d products %d round_streams %u lp %d ls %d ring_streams %u\n", line, (int)c.form.serve(), c.form.fused(),
                c.form.products(), c.form.round_streams(), c.lp, c.ls, c.ring_streams);
}
#define MFMA(p, h, m, f, ...) mfma_row(__LINE__, p, h, m, f, MfmaWant{ __VA_ARGS__ })

void kind_rows()
{
    const FormHooks none = Hk::none();
    // ---- stage 1, the kind (model.cpp:44-46 `many`, :47, :71-72, :77-78, :81, :87)
    KIND(lpool(16), none, conv_stack(), true, LK::Conv);                                         // model.cpp:47-48
    KIND(lpool(16, 64, 256, Force::Mfma), none, conv_stack(), true, LK::Conv);                   // ... whatever is forced
    KIND(lpool(64), none, one_layer(LSTM, 64), true, LK::Quad);                                  // pool.cpp:125 (below a round: k_quad), model.cpp:71-73
    KIND(lpool(64), none, one_layer(LSTM, 64), false, LK::Table);                                // model.cpp:72 (quad_lds_bytes > 160 KiB), :77 (not MANY_MFMA), :87
    KIND(unpacked(lpool(64)), none, one_layer(LSTM, 64), true, LK::Table);                       // model.cpp:72 (chain_lds_bytes)
    KIND(lpool(4096), none, one_layer(LSTM, 64), true, LK::Mfma);                                // pool.cpp:81, :86 (k_lstm_gs pays), model.cpp:77-79
    KIND(unpacked(lpool(4096)), none, one_layer(LSTM, 64), true, LK::Table);                     // model.cpp:77 (chain_lds_bytes)
    KIND(lpool(4096), none, unfit(one_layer(LSTM, 64)), true, LK::Table);                        // model.cpp:77 (mfma_form_fits)
    KIND(lpool(8), none, one_layer(LSTM, 32), true, LK::Table);                                  // pool.cpp:120 (MANY_NONE), model.cpp:87-88
    KIND(lpool(4096), none, one_layer(LSTM, 16), true, LK::Quad);                                // pool.cpp:120 (a round: k_quad)
    KIND(lpool(1024, 64, 64), none, one_layer(LSTM, 16), true, LK::Quad);                        // ... of 64 CUs: p.cus, which model.cpp:45 handed to the rule
    KIND(lpool(4096), none, one_layer(GRU, 32), true, LK::Mfma);                                 // pool.cpp:95-96 (a full round: the one-launch k_mfma_lp)
    KIND(lpool(5120, 256), none, one_layer(LSTM, 32), true, LK::Table);                          // pool.cpp:94 (between one and one and a half rounds: the split form)
    KIND(lpool(5632, 256), none, one_layer(LSTM, 32), true, LK::Mfma);                           // pool.cpp:59 (from 192-frame blocks), :90
    KIND(lpool(5632, 64), none, one_layer(LSTM, 32), true, LK::Table);                           // pool.cpp:59 (below them), :94
    KIND(lpool(1), none, one_layer(GRU, 64), true, LK::Mfma);                                    // pool.cpp:112 (k_gru_gs at every pool size, blocks of 64 frames and more)
    KIND(lpool(1, 4), none, one_layer(GRU, 64), true, LK::Quad);                                 // pool.cpp:112 (a four-frame pool keeps round 4's threshold), :122
    // AIDAX_KERNEL (model.cpp:45): quad / mfma force the form, every other word none
    KIND(lpool(8, 64, 256, Force::Quad), none, one_layer(LSTM, 32), true, LK::Quad);
    KIND(lpool(8, 64, 256, Force::Quad), none, one_layer(LSTM, 32), false, LK::Table);           // model.cpp:72 still holds
    KIND(lpool(8, 64, 256, Force::Mfma), none, one_layer(LSTM, 32), true, LK::Mfma);
    for (const Force f : { Force::Wave, Force::Pipe, Force::Split, Force::Valu, Force::Q4 }) {
        KIND(lpool(4096, 64, 256, f), none, one_layer(LSTM, 64), true, LK::Table);               // (MANY_NONE where the rule says MANY_MFMA ...
        KIND(lpool(64, 64, 256, f), none, one_layer(LSTM, 64), true, LK::Table);                 // ... and where it says MANY_QUAD)
    }
    // stacked models (model.cpp:78 the stack arm: anything but valu; :81-83)
    KIND(lpool(16), none, stacked(LSTM, 64, 2), true, LK::Mfma);
    KIND(lpool(16, 64, 256, Force::Valu), none, stacked(LSTM, 64, 2), true, LK::Stack);
    KIND(lpool(16, 64, 256, Force::Wave), none, stacked(LSTM, 64, 2), true, LK::Mfma);
    KIND(lpool(16, 64, 256, Force::Quad), none, stacked(LSTM, 64, 2), true, LK::Mfma);           // model.cpp:71 (n_rnn == 1 only)
    KIND(lpool(16, 64, 256, Force::Quad), none, wide_layer(LSTM, 96), true, LK::Mfma);           // model.cpp:71 (find_kernel)
    KIND(unpacked(lpool(16)), none, stacked(LSTM, 64, 2), true, LK::Stack);                      // model.cpp:77
    KIND(lpool(16), none, unfit(stacked(LSTM, 20, 2)), true, LK::Stack);                         // model.cpp:77 (mfma_form_fits), :81
    // the hooks the kind reads through the one-layer rule (pool.cpp:54, :75-76, :89, :106)
    KIND(lpool(2048), none, one_layer(LSTM, 64), true, LK::Mfma);
    KIND(lpool(2048), Hk::lstm_gs(0), one_layer(LSTM, 64), true, LK::Quad);                      // pool.cpp:77 (never), :61 (k_mfma_ls1 beyond 2048 streams only)
    KIND(lpool(2049), Hk::lstm_gs(0), one_layer(LSTM, 64), true, LK::Mfma);
    KIND(lpool(64), Hk::lstm_gs(1), one_layer(LSTM, 64), true, LK::Mfma);                        // pool.cpp:78 (wherever it serves)
    KIND(lpool(64), Hk::lstm_gs(1), one_layer(LSTM, 32), true, LK::Table);                       // pool.cpp:77 (40 / 64 / 80 units only)
    KIND(lpool(64), also_gru_gm(Hk::lstm_gs(1), 'f'), one_layer(LSTM, 64), true, LK::Quad);      // pool.cpp:77 (AIDAX_GRU_GM=f32 keeps round 3's table)
    KIND(lpool(2048), none, one_layer(LSTM, 80), true, LK::Mfma);                                // pool.cpp:62
    KIND(lpool(2048), Hk::ls1(0), one_layer(LSTM, 80), true, LK::Quad);                          // pool.cpp:89-90, :125
    KIND(lpool(2048), Hk::ls1(1), one_layer(LSTM, 80), true, LK::Mfma);                          // pool.cpp:89 (only =0 is read here)
    KIND(lpool(2048), Hk::lp_split('0'), one_layer(LSTM, 80), true, LK::Quad);                   // pool.cpp:54-55
    KIND(lpool(2048), Hk::lp_split('9'), one_layer(LSTM, 80), true, LK::Mfma);
    KIND(lpool(3584), also_lp_split(Hk::lstm_gs(0), '0'), one_layer(LSTM, 64), true, LK::Quad);  // pool.cpp:95-96: round 3's table, seven eighths of a round
    KIND(lpool(3585), also_lp_split(Hk::lstm_gs(0), '0'), one_layer(LSTM, 64), true, LK::Mfma);
    KIND(lpool(64), Hk::gru_gm('f'), one_layer(GRU, 64), true, LK::Quad);                        // pool.cpp:106, :112, :114, :122
    KIND(lpool(64), Hk::gru_gm('0'), one_layer(GRU, 64), true, LK::Mfma);                        // pool.cpp:106 (only =f32 is read here)
    KIND(lpool(2560), Hk::gru_gm('f'), one_layer(GRU, 64), true, LK::Mfma);                      // pool.cpp:114 (five eighths of a round)
    KIND(lpool(4096), Hk::mfma_lp(0), one_layer(LSTM, 64), true, LK::Mfma);                      // (the other hooks move nothing in the kind)
}

void conv_rows()
{
    const FormHooks none = Hk::none();
    // ---- stage 2, conv stacks (model.cpp:48-70). resident: what the occupancy query of the family answers
    const ConvWant ms_fused{ S::ConvMs, true, false, true, false, true }, ms_packed{ S::ConvMs, false, false, true, false, true };
    CONV(lpool(16), none, true, true, true, 512, ms_fused);                                                                // model.cpp:55-56, :65-68
    CONV(lpool(512), none, true, true, true, 512, ms_fused);                                                               // model.cpp:67 (<=)
    CONV(lpool(4096), none, true, true, true, 512, ms_packed);                                                             // ... a second round of workgroups
    CONV(lpool(16), none, true, false, true, 1024, S::ConvMfma, true, false, false, false, true);                          // model.cpp:55 (ms_ok), :68
    CONV(lpool(4096), none, true, false, true, 1024, S::ConvMfma, false, false, false, false, true);
    CONV(lpool(16), Hk::conv_ms_off(), true, true, true, 1024, S::ConvMfma, true, false, false, false, true);              // model.cpp:54-55
    CONV(lpool(16), Hk::conv_st_off(), true, true, true, 512, S::ConvMs, true, true, true, false, true);                   // model.cpp:59-60
    CONV(lpool(16, 64, 256, Force::Valu), Hk::conv_st_off(), true, true, true, 0, S::Conv, false, true, false, false, false);      // ... whatever the family
    CONV(lpool(16), Hk::conv_fused(0), true, true, true, 512, S::ConvMs, false, false, true, false, false);                // model.cpp:64, :66
    CONV(lpool(4096), Hk::conv_fused(1), true, true, true, 512, S::ConvMs, true, false, true, false, false);
    CONV(lpool(4096), Hk::conv_fused(1), true, false, true, 0, S::ConvMfma, true, false, false, false, false);
    CONV(lpool(4096, 512), none, true, true, true, 0, S::ConvMs, true, false, true, false, false);                         // model.cpp:65 (long blocks: the one-launch form only)
    CONV(lpool(4096, 512), Hk::conv_fused(0), true, true, true, 0, S::ConvMs, true, false, true, false, false);            // ... ahead of the hook
    CONV(lpool(4096, 256), none, true, true, true, 512, ms_packed);                                                        // model.cpp:65 (> 256)
    CONV(lpool(16, 64, 256, Force::Valu), none, true, true, true, 0, S::Conv, false, false, false, false, false);          // model.cpp:50, :68
    CONV(lpool(16, 64, 256, Force::Valu), Hk::conv_fused(1), true, true, true, 0, S::Conv, false, false, false, false, false);     // model.cpp:65 (conv_mfma &&)
    CONV(lpool(16), none, false, true, true, 0, S::Conv, false, false, false, false, false);                               // model.cpp:50 (convm_lds_bytes)
    CONV(lpool(16, 8192), none, false, true, false, 0, S::Conv, false, false, false, true, false);                         // model.cpp:69-70: refused
    CONV(lpool(16, 8192, 256, Force::Valu), none, true, true, false, 0, S::Conv, false, false, false, true, false);
    CONV(lpool(16, 512), none, true, true, false, 0, S::ConvMs, true, false, true, false, false);                          // model.cpp:69 (!conv_mfma &&): k_conv's planes do not matter
}

void mfma_rows()
{
    const FormHooks none = Hk::none();
    // ---- stage 2, the matrix-core forms (model.cpp:109-168)
    const ModelShape l64x2 = stacked(LSTM, 64, 2), l32x2 = stacked(LSTM, 32, 2);
    const MfmaFacts f64x2 = chained_facts(2, 64, 0), f32x2 = chained_facts(2, 32, 0);
    MFMA(lpool(16), none, l64x2, f64x2, S::Ls, true, 6, 0, true, true, 16);                      // model.cpp:129, :142-144, :151-156, :167
    MFMA(lpool(2048), none, l64x2, f64x2, S::Ls, true, 6, 0, true, true, 2048);                  // model.cpp:134, :139 (128 groups are one range)
    MFMA(lpool(2049), none, l64x2, f64x2, S::Ls, true, 6, 2048, true, true, 2048);               // model.cpp:134-139, :152, :167 (ranges of 128 groups)
    MFMA(lpool(4096), none, l64x2, f64x2, S::Ls, true, 6, 2048, true, true, 2048);
    MFMA(lpool(1024, 64, 64), none, l64x2, f64x2, S::Ls, true, 6, 512, true, true, 512);         // model.cpp:134 on 64 CUs: p.cus (:115 asked the same device again)
    MFMA(lpool(16, 64, 8), none, l64x2, f64x2, S::Mfma, false, 0, 0, false, false, 16);          // model.cpp:134, :139 (a range of no groups), :143 (16 workgroups on 8 CUs)
    MFMA(lpool(2048), none, l32x2, f32x2, S::Ls, true, 6, 0, true, true, 2048);                  // model.cpp:143 (256 workgroups on 256 CUs)
    MFMA(lpool(2049), none, l32x2, f32x2, S::Mfma, false, 0, 0, false, false, 2049);             // model.cpp:138 (below 64 units: no ranges), :142-143 (272 workgroups)
    MFMA(lpool(1280), none, stacked(LSTM, 32, 3), chained_facts(3, 32, 0), S::Ls, true, 6, 0, true, true, 1280);        // model.cpp:142 (80 groups x 3)
    MFMA(lpool(1360), none, stacked(LSTM, 32, 3), chained_facts(3, 32, 0), S::Mfma, false, 0, 0, false, false, 1360);   // model.cpp:140-142 (85 groups x 3 are 264 workgroups)
    MFMA(lpool(4096), none, stacked(LSTM, 64, 3), chained_facts(3, 64, 0), S::Ls, true, 6, 1280, true, true, 1280);     // model.cpp:134 (256 / 3 / 8 * 8 = 80 groups)
    MFMA(lpool(4096), none, stacked(LSTM, 80, 2), chained_facts(2, 80, 0), S::Ls, true, 6, 2048, true, true, 2048);     // model.cpp:138 (LSTM-80: up to two grids' worth)
    MFMA(lpool(4112), none, stacked(LSTM, 80, 2), chained_facts(2, 80, 0), S::Mfma, false, 0, 0, false, false, 4112);   // ... 257 groups on 256 CUs
    MFMA(lpool(8192), none, stacked(GRU, 80, 2), chained_facts(2, 80, 1), S::Ls, true, 6, 2048, true, true, 2048);      // model.cpp:138 (L[0].cell != 0)
    MFMA(lpool(8192), none, stacked(LSTM, 96, 2), chained_facts(2, 96, 0), S::Ls, true, 6, 2048, true, true, 2048);
    // what a kernel does not serve, or has no LDS for (model.cpp:129-130, :144, :154-156)
    MFMA(lpool(16), none, l64x2, without(f64x2, &MfmaFacts::ls_serves), S::Lp, true, 0, 0, true, false, 16);
    MFMA(lpool(16), none, l64x2, without(f64x2, &MfmaFacts::ls_lds_ok), S::Lp, true, 0, 0, true, false, 16);
    MFMA(lpool(4096), none, l64x2, without(f64x2, &MfmaFacts::ls_lds_ok), S::Mfma, false, 0, 0, false, false, 4096);    // model.cpp:139, :143 (no ranges without k_mfma_ls)
    MFMA(lpool(16), none, l64x2, without(f64x2, &MfmaFacts::lp_serves), S::Mfma, false, 0, 0, false, false, 16);        // model.cpp:144, :151 (ls needs lp)
    MFMA(lpool(4096), none, l64x2, without(f64x2, &MfmaFacts::lp_lds_ok), S::Mfma, false, 0, 0, false, false, 4096);    // model.cpp:144, :152
    MFMA(lpool(16), none, l64x2, without(f64x2, &MfmaFacts::ls_fused_serves), S::Ls, false, 6, 0, true, true, 16);      // model.cpp:155
    MFMA(lpool(16), none, l64x2, without(f64x2, &MfmaFacts::ls_fused_lds_ok), S::Ls, false, 6, 0, true, true, 16);
    MFMA(lpool(16), none, l64x2, without(without(f64x2, &MfmaFacts::ls_serves), &MfmaFacts::lp_fused_serves), S::Lp, false, 0, 0, true, false, 16);      // model.cpp:156
    MFMA(lpool(16), none, l64x2, without(without(f64x2, &MfmaFacts::ls_serves), &MfmaFacts::lp_fused_lds_ok), S::Lp, false, 0, 0, true, false, 16);
    MFMA(lpool(16), none, l64x2, without(f64x2, &MfmaFacts::lp_fused_serves), S::Ls, true, 6, 0, true, true, 16);       // (k_mfma_ls asks its own)
    // the hooks of the chained kernels
    MFMA(lpool(16), Hk::mfma_lp(0), l64x2, f64x2, S::Mfma, false, 0, 0, false, false, 16);                              // model.cpp:113, :143
    MFMA(lpool(4096), Hk::mfma_lp(0), l64x2, f64x2, S::Mfma, false, 0, 0, false, false, 4096);
    MFMA(lpool(4096), Hk::mfma_lp(1), l64x2, f64x2, S::Ls, true, 6, 0, true, true, 4096);                               // model.cpp:139 (=1: never in ranges), :143
    MFMA(lpool(2049), Hk::mfma_lp(1), l32x2, f32x2, S::Ls, true, 6, 0, true, true, 2049);                               // model.cpp:143 (on, where it would not pay)
    MFMA(lpool(16), Hk::mfma_lp(1), l64x2, without(f64x2, &MfmaFacts::lp_lds_ok), S::Mfma, false, 0, 0, false, false, 16);      // model.cpp:144 (the LDS is no matter of choice)
    MFMA(lpool(16), Hk::lp_split('0'), l64x2, f64x2, S::Lp, true, 0, 0, true, false, 16);                               // model.cpp:125, :129
    MFMA(lpool(4096), Hk::lp_split('0'), l64x2, f64x2, S::Mfma, false, 0, 0, false, false, 4096);
    MFMA(lpool(16), Hk::lp_split('9'), l64x2, f64x2, S::Ls, true, 9, 0, true, true, 16);                                // model.cpp:167
    MFMA(lpool(4096), Hk::lp_split('9'), l64x2, f64x2, S::Ls, true, 9, 2048, true, true, 2048);
    MFMA(lpool(16), Hk::lp_fused_off(), l64x2, f64x2, S::Ls, false, 6, 0, true, true, 16);                              // model.cpp:153-154
    MFMA(lpool(16), Hk::lp_fused_off(), l64x2, without(f64x2, &MfmaFacts::ls_serves), S::Lp, false, 0, 0, true, false, 16);
    MFMA(lpool(272), Hk::round_groups(8), l64x2, f64x2, S::Ls, true, 6, 128, true, true, 128);                          // model.cpp:131-133, :139 (17 groups in ranges of 8)
    MFMA(lpool(272), Hk::round_groups(8), l32x2, f32x2, S::Ls, true, 6, 128, true, true, 128);                          // model.cpp:138 (rg_env ||: any width)
    MFMA(lpool(128), Hk::round_groups(8), l64x2, f64x2, S::Ls, true, 6, 0, true, true, 128);                            // model.cpp:139 (8 groups are one range)
    MFMA(lpool(32), Hk::round_groups(1), l64x2, f64x2, S::Ls, true, 6, 16, true, true, 16);                             // model.cpp:139 (rg_env ? 1u : 8u)
    MFMA(lpool(4096), Hk::round_groups(0), l32x2, f32x2, S::Ls, true, 6, 2048, true, true, 2048);                       // model.cpp:132 (set, not > 0: the device's range), :138
    MFMA(lpool(272), also_lp_split(Hk::round_groups(8), '0'), l64x2, f64x2, S::Lp, true, 0, 0, true, false, 272);       // model.cpp:139 (ls_ok &&)
    // one-layer models: k_mfma_ls1 and the one-launch k_mfma_lp (model.cpp:119, :121, :127-128, :143)
    const ModelShape l80 = one_layer(LSTM, 80), l40 = one_layer(LSTM, 40), l64 = one_layer(LSTM, 64), g64 = one_layer(GRU, 64), g80 = one_layer(GRU, 80);
    const MfmaFacts f80 = chained_facts(1, 80, 0), f48 = chained_facts(1, 48, 0), f64 = with_lstm_gs(chained_facts(1, 64, 0));
    const MfmaFacts fg64 = with_gru_kernels(chained_facts(1, 64, 1)), fg80 = with_gru_kernels(chained_facts(1, 80, 1));
    MFMA(lpool(4096), none, l80, f80, S::Ls, true, 6, 0, true, true, 4096);                                             // pool.cpp:62, model.cpp:128, :143 (ls_ok && !lp_chained)
    MFMA(lpool(8192), none, l80, f80, S::Ls, true, 6, 0, true, true, 8192);                                             // model.cpp:138 (LSTM-80 beyond a round of groups: no ranges), :143
    MFMA(lpool(4096), Hk::ls1(0), l80, f80, S::Lp, true, 0, 0, true, false, 4096);                                      // model.cpp:128, :143 (256 workgroups)
    MFMA(lpool(8192), Hk::ls1(0), l80, f80, S::Mfma, false, 0, 0, false, false, 8192);                                  // model.cpp:119 (80 > 48 units), :143
    MFMA(lpool(64), none, l80, f80, S::Lp, true, 0, 0, true, false, 64);                                                // pool.cpp:62 (4 groups), model.cpp:143
    MFMA(lpool(64), Hk::ls1(1), l80, f80, S::Ls, true, 6, 0, true, true, 64);                                           // model.cpp:128 (forced on)
    MFMA(lpool(64), also_lp_split(Hk::ls1(1), '0'), l80, f80, S::Lp, true, 0, 0, true, false, 64);                      // model.cpp:129
    MFMA(lpool(4096), Hk::lp_split('0'), l80, f80, S::Lp, true, 0, 0, true, false, 4096);                               // pool.cpp:54-55
    MFMA(lpool(8192), Hk::lp_split('0'), l40, f48, S::Lp, true, 0, 0, true, false, 8192);                               // model.cpp:119 (<= 48 units: several rounds of the one-launch form)
    MFMA(lpool(8192), Hk::lp_split('0'), l40, without(f48, &MfmaFacts::lp_fused_serves), S::Mfma, false, 0, 0, false, false, 8192);
    MFMA(lpool(8192), none, l40, f48, S::Ls, true, 6, 0, true, true, 8192);                                             // pool.cpp:60 (beyond a round), model.cpp:138 (48 units: no ranges)
    MFMA(lpool(8192), Hk::ls1(0), g80, without(without(fg80, &MfmaFacts::gru_gs_serves), &MfmaFacts::gru_gm_serves), S::Mfma, false, 0, 0, false, false, 8192);
    MFMA(lpool(8192), none, g80, without(without(fg80, &MfmaFacts::gru_gs_serves), &MfmaFacts::gru_gm_serves), S::Ls, true, 6, 4096, true, true, 4096);      // model.cpp:134 (256 groups), :138 (a GRU)
    // ... and their one-launch kernels (model.cpp:146-165)
    MFMA(lpool(4096), none, l64, f64, S::LstmGs, false, 6, 0, true, true, 4096);                                        // model.cpp:160-161; the ring of pk.lp all the same (:158)
    MFMA(lpool(4096), Hk::gs_products(9), l64, f64, S::LstmGs, false, 9, 0, true, true, 4096);                          // model.cpp:147-148
    MFMA(lpool(4096), Hk::lstm_gs(0), l64, f64, S::Ls, true, 6, 0, true, true, 4096);                                   // pool.cpp:77, model.cpp:167
    MFMA(lpool(4096), Hk::gru_gm('f'), l64, f64, S::Ls, true, 6, 0, true, true, 4096);                                  // pool.cpp:76-77
    MFMA(lpool(4096), none, l64, without(f64, &MfmaFacts::lstm_gs_lds_ok), S::Ls, true, 6, 0, true, true, 4096);        // model.cpp:160
    MFMA(lpool(4096), none, l64, without(f64, &MfmaFacts::lstm_gs_serves), S::Ls, true, 6, 0, true, true, 4096);
    MFMA(lpool(16), Hk::lstm_gs(1), l64, f64, S::LstmGs, false, 6, 0, true, false, 16);                                 // pool.cpp:78; model.cpp:143 (8 workgroups), no k_mfma_ls1 (pool.cpp:61)
    MFMA(lpool(16), none, l64, f64, S::Lp, true, 0, 0, true, false, 16);                                                // pool.cpp:81 (AIDAX_KERNEL=mfma on a small pool)
    MFMA(lpool(4096), none, l80, with_lstm_gs(f80), S::Ls, true, 6, 0, true, true, 4096);                               // pool.cpp:81 (LSTM-80: served, not in the rule)
    MFMA(lpool(4096), Hk::lstm_gs(1), l80, with_lstm_gs(f80), S::LstmGs, false, 6, 0, true, true, 4096);
    MFMA(lpool(64), none, g64, fg64, S::GruGs, false, 6, 0, true, false, 64);                                           // model.cpp:162-163
    MFMA(lpool(64), Hk::gs_products(9), g64, fg64, S::GruGs, false, 9, 0, true, false, 64);
    MFMA(lpool(64), Hk::gru_gm('f'), g64, fg64, S::GruGm, false, 0, 0, true, false, 64);                                // model.cpp:162, :164-165
    MFMA(lpool(64), Hk::gru_gm('0'), g64, fg64, S::Lp, true, 0, 0, true, false, 64);                                    // model.cpp:162, :164, :167
    MFMA(lpool(64), also_gru_gm(Hk::ls1(1), '0'), g64, fg64, S::Ls, true, 6, 0, true, true, 64);
    MFMA(lpool(64), none, g64, without(fg64, &MfmaFacts::gru_gs_lds_ok), S::GruGm, false, 0, 0, true, false, 64);       // model.cpp:162
    MFMA(lpool(64), none, g80, without(fg80, &MfmaFacts::gru_gm_serves), S::GruGs, false, 6, 0, true, false, 64);       // (80 units: the split kernel only)
    MFMA(lpool(64), Hk::gru_gm('f'), g80, without(fg80, &MfmaFacts::gru_gm_serves), S::Lp, true, 0, 0, true, false, 64);
    MFMA(lpool(64), none, g64, without(without(fg64, &MfmaFacts::gru_gs_lds_ok), &MfmaFacts::gru_gm_lds_ok), S::Lp, true, 0, 0, true, false, 64);      // model.cpp:164
    MFMA(lpool(8192), none, g64, fg64, S::GruGs, false, 6, 0, false, false, 8192);                                      // model.cpp:143 (512 workgroups: no ring), :163
}

void load_expect(bool ok, const char* what, const LoadPool& p, const ModelShape& m, int detail)
{
    ++checks;
    if (ok) return;
    if (++failures <= 20) std::printf("load property \"%s\": streams %u max_frames %u cus %d force %d | cell %d hidden %d layers %d | %d\n", what, p.n_streams, p.max_frames, p.cus, (int)p.force, m.cell, m.hidden, m.n_rnn, detail);
}

void load_properties()
{
    const Force forces[] = { Force::None, Force::Wave, Force::Pipe, Force::Split, Force::Valu, Force::Mfma, Force::Quad, Force::Q4 };
    std::initializer_list<FormHooks> hooks = { Hk::none(), Hk::ls1(0), Hk::ls1(1), Hk::lstm_gs(0), Hk::lstm_gs(1), Hk::gru_gm('0'), Hk::gru_gm('f'), Hk::mfma_lp(0), Hk::mfma_lp(1),
                                               Hk::lp_split('0'), Hk::lp_split('9'), Hk::lp_fused_off(), Hk::round_groups(8), Hk::round_groups(0), Hk::gs_products(9),
                                               Hk::conv_ms_off(), Hk::conv_st_off(), Hk::conv_fused(0), Hk::conv_fused(1) };
    auto shape = [](int cell, int hidden, int layers) { return layers == 1 && hidden <= 80 ? one_layer(cell, hidden) : layers == 1 ? wide_layer(cell, hidden) : stacked(cell, hidden, layers); };
    for (const FormHooks& h : hooks)
    for (const uint32_t streams : { 1u, 16u, 272u, 2048u, 4096u, 8192u })
    for (const uint32_t max_frames : { 4u, 64u, 256u, 512u })
    for (const int cus : { 8, 64, 256 }) {
        // stage 1, and the conv stacks: every forced form, the packed chains with and without room
        for (const Force force : forces)
        for (int packed = 0; packed <= 1; ++packed) {
            LoadPool p = lpool(streams, max_frames, cus, force);
            p.packed_fits = packed != 0;
            for (const int cell : { LSTM, GRU })
            for (const int hidden : { 16, 32, 40, 64, 80, 96 })
            for (const int layers : { 1, 2, 3 })
            for (int bits = 0; bits < 4; ++bits) {      // mfma_form_fits, quad_lds_ok
                const ModelShape m = shape(cell, hidden, layers);
                const LK k = load_kind(p, h, bits & 1 ? m : unfit(m), (bits & 2) != 0);
                load_expect(k != LK::Conv, "a recurrent model is no conv slot", p, m, (int)k);
                load_expect(force != Force::Valu || (k != LK::Mfma && k != LK::Quad), "a forced Valu never yields a matrix-core kind", p, m, (int)k);
                load_expect(k != LK::Quad || (layers == 1 && m.table_kernel && (bits & 2) && packed), "k_quad: a table model, its LDS, the packed chains", p, m, (int)k);
                load_expect(k != LK::Mfma || ((bits & 1) && packed), "the matrix-core kind: mfma_form_fits, the packed chains", p, m, (int)k);
                load_expect((k == LK::Stack) == (m.stack && k != LK::Mfma), "what is left of the stacked models: k_stack", p, m, (int)k);
            }
            // (a non-MFMA kind never has lp: only mfma_form hands one out — a conv decision has no such field)
            for (int bits = 0; bits < 8; ++bits)        // convm_lds_ok, ms_ok, conv_lds_ok
            for (const int resident : { 0, 16, 4096 }) {
                const ModelShape m = conv_stack();
                load_expect(load_kind(p, h, m, true) == LK::Conv, "a conv model is a conv slot", p, m, bits);
                const ConvFamily f = conv_family(p, h, bits & 1, bits & 2, bits & 4);
                const SlotForm s = conv_form(f, p, h, resident);
                load_expect(force != Force::Valu || s.serve() == S::Conv, "a forced Valu never yields a matrix-core conv family", p, m, bits);
                load_expect(s.serve() == S::Conv || s.serve() == S::ConvMfma || s.serve() == S::ConvMs, "a conv form", p, m, bits);
                load_expect((s.serve() == S::ConvMs) == f.ms && (s.serve() != S::Conv) == f.mfma && (!f.ms || ((bits & 2) && !h.conv_ms_off)), "the family", p, m, bits);
                load_expect(f.refused == (s.serve() == S::Conv && !(bits & 4)), "refused: k_conv without room for its planes", p, m, bits);
                load_expect(!s.fused() || s.serve() != S::Conv, "k_conv is never fused", p, m, bits);
                load_expect(s.serve() == S::Conv || max_frames <= 256 || s.fused(), "long blocks: the one-launch form only", p, m, bits);
                load_expect(f.by_size || s.serve() == S::Conv || conv_form(f, p, h, 0).fused() == conv_form(f, p, h, 1 << 30).fused(), "by_size says when the resident count is read", p, m, bits);
            }
        }
        // stage 2 of the matrix-core kind, on every descriptor the kernels might report (it reads neither the forced form nor packed_fits)
        const LoadPool p = lpool(streams, max_frames, cus);
        for (const int cell : { LSTM, GRU })
        for (const int hidden : { 16, 32, 40, 64, 80, 96 })
        for (const int layers : { 1, 2, 3 })
        for (int serves = 0; serves < 32; ++serves)
        for (int lds = 0; lds < 4; ++lds) {
            const ModelShape m = shape(cell, hidden, layers);
            MfmaFacts f = chained_facts(layers, hidden == 40 ? 48 : hidden, cell);
            f.lp_serves = serves & 1; f.ls_serves = serves & 2; f.lp_fused_serves = serves & 4; f.ls_fused_serves = (serves & 2) && (serves & 4);
            if (layers == 1 && cell == LSTM && (serves & 8)) f = with_lstm_gs(f);
            if (layers == 1 && cell == GRU && (serves & 8)) f = with_gru_kernels(f);
            if (serves & 16) f.gru_gm_serves = f.gru_gm_lds_ok = false;
            f.lp_lds_ok = f.lp_serves && (lds & 1); f.lp_fused_lds_ok = f.lp_fused_serves && (lds & 1); f.ls_lds_ok = f.ls_serves && (lds & 2); f.ls_fused_lds_ok = f.ls_fused_serves && (lds & 2);
            const MfmaChoice c = mfma_form(p, h, m, f);
            const S s = c.form.serve();
            const bool one_launch = s == S::GruGm || s == S::GruGs || s == S::LstmGs;
            load_expect(!c.ls || c.lp, "ls implies lp", p, m, serves);
            // (a one-launch slot keeps the ring k_mfma_ls1 would have had, ranges and all, though no pass of its form uses it: allocation as it was)
            load_expect(one_launch || c.ring_streams == (c.form.round_streams() ? c.form.round_streams() : streams), "ring_streams is n_streams unless the form has round_streams", p, m, serves);
            load_expect(c.ring_streams == streams || (c.ls && c.ring_streams % 16u == 0 && c.ring_streams < streams), "a shorter ring: k_mfma_ls's, whole groups", p, m, serves);
            load_expect(!c.form.round_streams() || (s == S::Ls && c.form.round_streams() == c.ring_streams && c.ring_streams < streams), "stream ranges: k_mfma_ls only, more than one", p, m, serves);
            load_expect(s == S::Mfma || s == S::Lp || s == S::Ls || one_launch, "a matrix-core form", p, m, serves);
            load_expect((s != S::Lp || (c.lp && !c.ls)) && (s != S::Ls || c.ls) && (s != S::Mfma || !c.lp), "Lp / Ls / Mfma say what the slot holds", p, m, serves);
            load_expect(!c.lp || (f.lp_serves && f.lp_lds_ok), "lp: served, with room in the LDS", p, m, serves);
            load_expect(!c.ls || (f.ls_serves && f.ls_lds_ok && h.lp_split != '0'), "ls: served, with room in the LDS, not switched off", p, m, serves);
            load_expect(!(c.form.fused() && h.lp_fused_off) && (!c.form.fused() || s == S::Lp || s == S::Ls), "fused: the chained kernels, unless switched off", p, m, serves);
            load_expect(!one_launch || layers == 1, "the one-launch kernels: one-layer models", p, m, serves);
            load_expect(c.form.products() == (s == S::Ls ? (h.lp_split == '9' ? 9 : 6) : s == S::GruGs || s == S::LstmGs ? h.gs_products : 0), "term products: the split kernels'", p, m, serves);
        }
    }
}

}  // namespace

int main()
{
    // parse_force: AIDAX_KERNEL's seven words, everything else no force
    const struct { const char* word; Force f; } words[] = { { "wave", Force::Wave }, { "pipe", Force::Pipe }, { "split", Force::Split }, { "valu", Force::Valu }, { "mfma", Force::Mfma },
                                                            { "quad", Force::Quad }, { "q4", Force::Q4 }, { "", Force::None }, { "pipe4", Force::None }, { "WAVE", Force::None }, { nullptr, Force::None } };
    for (const auto& w : words) { ++checks; if (parse_force(w.word) != w.f) { ++failures; std::printf("parse_force(%s)\n", w.word ? w.word : "null"); } }
    const long n_words = checks;
    rows();
    const long n_rows = checks - n_words;
    properties();
    const long n_pass = checks;
    kind_rows();
    conv_rows();
    mfma_rows();
    const long n_load_rows = checks - n_pass;
    load_properties();
    std::printf("form_harness: %ld rows, %ld checks, %d failures (load form: %ld rows, %ld checks)\n", n_rows, checks, failures, n_load_rows, checks - n_pass);
    return failures ? 1 : 0;
}
