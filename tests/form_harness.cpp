// form_harness.cpp — the pass-form decision (csrc/aidax_pass_form.h: resolve_pass) as a plain host program, built with ASan + UBSan by
// `make asan_form` and run by tests/test_pass_form_host.py. Two parts:
//   (a) a literal table of rows, facts -> (kernel, chains around, carries event / word, pieces, in place, name). Every row restates what the
//       three hand-written copies of the decision did before they became one function; the comment on a row names the lines of that commit
//       (784ca42: pool.h = csrc/aidax_pool.h, pool.cpp = csrc/aidax_pool.cpp, model.cpp = csrc/aidax_pool_model.cpp) it was read from.
//   (b) properties over the whole product of small inputs, on the 18 cells of the kernel table with their presence bits restated here.
// It reads no oracle of itself: every expectation is written out below.
#include <cstdio>
#include <cstring>
#include <initializer_list>

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
    std::printf("form_harness: %ld rows, %ld checks, %d failures\n", n_rows, checks, failures);
    return failures ? 1 : 0;
}
