// aidax_pass_form.h — which kernels serve a pass of a pool: the ONE statement of it. choose_form (aidax_pool_model.cpp) writes a model's
// SlotForm once per load; resolve_pass turns it, the pool's facts and the facts of one pass into a PassForm, which aidax_pool::launch
// executes, aidax_pool_kernel_name names and aidax_pool_process asks whether the pass may run in place on host memory. A new form is
// one PassKern enumerator, one arm here and one in launch. No HIP header, no lock, no allocation, no environment: a plain host program
// can include this file (tests/form_harness.cpp does).
#pragma once

#include <cstddef>
#include <cstdint>
#include <cstring>

#include "aidax_layout.h"

namespace aidax {

// AIDAX_KERNEL=wave|pipe|split|valu|mfma|quad|q4 (test build): overrides the heuristics, for A/B runs and tests
enum class Force : uint8_t { None, Wave, Pipe, Split, Valu, Mfma, Quad, Q4 };
inline Force parse_force(const char* s)
{
    static const struct { const char* word; Force f; } words[] = { { "wave", Force::Wave }, { "pipe", Force::Pipe }, { "split", Force::Split }, { "valu", Force::Valu },
                                                                   { "mfma", Force::Mfma }, { "quad", Force::Quad }, { "q4", Force::Q4 } };
    for (const auto& w : words)
        if (s && std::strcmp(s, w.word) == 0) return w.f;
    return Force::None;
}

// The kernel families a pass can launch (k_conv_st is no form of a pass: launch_conv_ms_kernel takes it for the block lengths it is compiled for)
enum class PassKern : uint8_t { NoModel, Wave, Pipe, Pipe4, PipeBank, Q4, Nn, Quad, Mfma, MfmaLp, MfmaLs, GruGm, GruGs, LstmGs, Stack, Conv, ConvMfma, ConvMs };

// What a (cell, hidden) pair of the kernel table offers next to its one-wave kernel, and the kernels' names (KernelEntry::has)
struct CellKernels {
    bool pipe, nn, pipe4, pipe4c, bank;      // k_*_pipe, k_nn, k_*_pipe4 for plain / conditioned models, k_*_pipe_bank
    const char *name, *name_pipe, *name_split, *name_pipe4, *name_bank;
};

// What choose_form decides for a model in a pool: how its passes are served. Built by the named constructors only, so that a field never
// says something its `serve` cannot mean (term products without a split kernel, stream ranges without k_mfma_ls, a fused k_conv).
class SlotForm {
public:
    enum class Serve : uint8_t {
        NoModel,
        Table,                       // the table kernels: the form of a pass follows from the three facts below
        Quad, Stack,
        Conv, ConvMfma, ConvMs,      // k_conv; on the matrix cores (blocks of <= 256 frames) in fp32 / as bf16 term products (its own history layout)
        Mfma,                        // k_mfma between packed chains
        Lp, Ls,                      // the chained kernels, while the slot holds a ring and nobody has refused or retired them (PassFacts::ring_ready), else k_mfma
        GruGm, GruGs, LstmGs,        // one-layer models, the whole run() in one launch (passes of n > 0 frames; every other launch: k_mfma)
    };
    SlotForm() = default;
    // pipe_capacity: streams the 3-wave pipeline keeps resident at once (0: never use it); split_pays: the lean recurrent kernel keeps the
    // occupancy of the one-wave kernel; q4: the slot holds k_lstm_q4's weight record (AIDAX_KERNEL=q4)
    static SlotForm table(int pipe_capacity, bool split_pays, bool q4) { SlotForm f(Serve::Table); f.pipe_capacity_ = pipe_capacity; f.split_pays_ = split_pays; f.q4_ = q4; return f; }
    static SlotForm quad() { return SlotForm(Serve::Quad); }
    static SlotForm stack() { return SlotForm(Serve::Stack); }
    static SlotForm conv() { return SlotForm(Serve::Conv); }
    // fused: the DSP chain runs inside the same launch (else packed k_chain launches go around it)
    static SlotForm conv_mfma(bool fused) { return SlotForm(Serve::ConvMfma, fused); }
    static SlotForm conv_ms(bool fused) { return SlotForm(Serve::ConvMs, fused); }
    static SlotForm mfma() { return SlotForm(Serve::Mfma); }
    static SlotForm lp(bool fused) { return SlotForm(Serve::Lp, fused); }
    // products: 6 or 9 term products of the split operands; round_streams: a pass over more streams goes out as one launch per range of so many (0: one launch)
    static SlotForm ls(int products, bool fused, uint32_t round_streams) { SlotForm f(Serve::Ls, fused, products); f.round_streams_ = round_streams; return f; }
    static SlotForm gru_gm() { return SlotForm(Serve::GruGm); }
    static SlotForm gru_gs(int products) { return SlotForm(Serve::GruGs, false, products); }
    static SlotForm lstm_gs(int products) { return SlotForm(Serve::LstmGs, false, products); }

    Serve serve() const { return serve_; }
    bool fused() const { return fused_; }
    int products() const { return products_; }
    uint32_t round_streams() const { return round_streams_; }
    int pipe_capacity() const { return pipe_capacity_; }
    bool split_pays() const { return split_pays_; }
    bool q4() const { return q4_; }

private:
    explicit SlotForm(Serve s, bool fused = false, int products = 0) : serve_(s), fused_(fused), products_(static_cast<uint8_t>(products)) {}
    Serve serve_ = Serve::NoModel;
    bool fused_ = false, split_pays_ = false, q4_ = false;
    uint8_t products_ = 0;
    int pipe_capacity_ = 0;
    uint32_t round_streams_ = 0;
};

// The pool's side of the decision. The hooks are read by the pool on every call (tests switch forms within one process) and passed in.
struct PoolFacts {
    uint32_t n_streams, max_frames;
    int cus;
    Force force;
    bool pipe4_off;              // AIDAX_PIPE4=0
    int pipe4_min;               // AIDAX_PIPE4_MIN, < 0: not set
    bool bank;                   // the model bank is in force on the playing slot, and this is a pass of it
    bool lp_off;                 // a hand-over of this pool gave up: no chained kernel for stacked models any more
    bool packed_fits;            // the packed chains' eight rows of max_frames fit their LDS (chain_lds_bytes <= kChainLdsLimit)
};

// ... and one pass's
struct PassFacts {
    SlotForm slot;
    const CellKernels* has;      // Table slots: the cell's kernels (nullptr otherwise)
    int mode;                    // MODE_CHAIN, MODE_WARMUP, MODE_NN_ONLY
    uint32_t n_frames, n_streams;
    int input_size;
    bool pipe4_lds_ok;           // Table: k_*_pipe4's LDS for this block fits a CU (pipe4_lds_bytes <= 160 KiB)
    bool ring_ready;             // Lp / Ls: the slot holds its hand-over ring and the runtime has not refused its grid
    bool hand_over;              // ... and its layers hand over through it (two layers or more: lp_off retires the kernel)
    bool conv_st;                // ConvMs: the stack has a k_conv_st geometry (ConvDesc::st_ok)
};

struct PassForm {
    PassKern kern;
    bool chains;                 // packed k_chain launches go around the kernel — which is then left out of a pass of no frames
    bool carries_event;          // the launch can take the pass-done event with it ...
    bool carries_word;           // ... and its one workgroup can write the completion word
    enum Pieces : uint8_t { WHOLE, TIME_SLICES, STREAM_RANGES } pieces;      // slices of the extension kernels' 256 frames; ranges of SlotForm::round_streams
    bool host_in_place;          // the blocking host path may let the pass read and write pinned host memory (NOT "is it one launch": no matrix-core form does)
    const char* name;
};

// Four streams per workgroup (k_*_pipe4: 61.9 us per cfg2 block against k_lstm_pipe's 63.8, the small cells 9 - 19 % ahead, conditioned models
// 9 - 25 % at every cell up to 32: profiles/r06_cfg2_pipe4.txt, r06_pipe4_cells.txt) in place of the three-wave pipeline, on the same state:
// whole 16-frame tiles, at least one full workgroup of four streams (a conditioned model: any pool), every workgroup on a CU of its own.
// (a plain model below one full workgroup: level at 256 frames, 0.6 - 1.0 us behind at 64 — the helper wave's longer prologue; a conditioned
// model is 11 - 20 % ahead also as a pool of ONE stream, the LV2 instance's. AIDAX_PIPE4_MIN, test build: the measurement's switch)
inline bool pipe4_serves(const PoolFacts& p, const PassFacts& f)
{
    const uint32_t n = f.n_frames, min_streams = p.pipe4_min >= 0 ? static_cast<uint32_t>(p.pipe4_min) : f.input_size > 1 ? 1u : 4u;
    if (p.pipe4_off || p.force != Force::None || !(f.input_size > 1 ? f.has->pipe4c : f.has->pipe4) || f.input_size < 1 || f.input_size > 3 || n == 0 || n % 16u || p.n_streams < min_streams) return false;
    return p.cus > 0 && (p.n_streams + 3u) / 4u <= static_cast<uint32_t>(p.cus) && f.pipe4_lds_ok;
}

// A MODE_CHAIN pass of a Table slot or of a pool without a model: one wave per stream; the three-wave pipeline (all streams resident at once:
// latency-bound regime); split launches with packed chains (many streams: issue-bound regime — needs no model); four streams per workgroup
// with the cell on the matrix cores (k_lstm_q4: opt-in only, measured slower than the pipeline, see aidax_q4.hip)
inline PassKern table_pass_kern(const PoolFacts& p, const PassFacts& f)
{
    const bool model = f.slot.serve() == SlotForm::Serve::Table;
    const PassKern wave = model ? PassKern::Wave : PassKern::NoModel;
    if (f.mode != MODE_CHAIN) return wave;
    if (model && f.slot.q4() && p.force == Force::Q4) return PassKern::Q4;
    if (p.force == Force::Wave) return wave;
    const bool pipe = model && f.has->pipe;
    if (p.force == Force::Pipe) return pipe ? PassKern::Pipe : wave;
    if (p.force == Force::Split) return p.packed_fits && (!model || f.has->nn) ? PassKern::Nn : wave;
    if (pipe && static_cast<int>(p.n_streams) <= f.slot.pipe_capacity()) return pipe4_serves(p, f) ? PassKern::Pipe4 : PassKern::Pipe;
    if (p.n_streams < 64 || !p.packed_fits) return wave;
    return !model || f.slot.split_pays() ? PassKern::Nn : wave;
}

// May a slot that holds its hand-over ring (and whose grid the runtime has not refused) still use its chained kernel? A give-up of the pool
// (lp_off) retires it for the models whose layers hand over through the ring; a lone layer waits for nothing and keeps it.
inline bool chained_usable(bool ring_ready, bool hand_over, bool lp_off) { return ring_ready && !(hand_over && lp_off); }

inline PassForm resolve_pass(const PoolFacts& p, const PassFacts& f)
{
    using S = SlotForm::Serve;
    const bool chain = f.mode == MODE_CHAIN, frames = f.n_frames != 0;
    PassForm r{ PassKern::NoModel, false, false, false, PassForm::WHOLE, true, "k_nomodel" };
    switch (f.slot.serve()) {
    case S::NoModel:
    case S::Table: {
        const bool model = f.slot.serve() == S::Table;
        // (the bank in force: the whole pass is one launch of k_*_pipe_bank, whatever form the pool model alone would take)
        r.kern = p.bank && model ? PassKern::PipeBank : table_pass_kern(p, f);
        r.chains = r.kern == PassKern::Nn;
        // A one-launch pass takes its end markers with it: the pipelined host path's "pass done" event rides on the dispatch (it saves the
        // marker packet behind the kernel), and the blocking path's completion word is written by the one workgroup of a one-stream pool itself
        r.carries_event = r.kern == PassKern::Pipe || r.kern == PassKern::Pipe4 || r.kern == PassKern::PipeBank;
        r.carries_word = r.carries_event && f.n_streams == 1 && frames;
        r.host_in_place = !r.chains;
        if (model)      // (no model: "k_nomodel" also where the passes go out in the split form)
            switch (r.kern) {
            case PassKern::PipeBank: r.name = f.has->name_bank; break;
            case PassKern::Q4: r.name = "k_lstm_q4<32>"; break;
            case PassKern::Pipe4: r.name = f.has->name_pipe4; break;
            case PassKern::Pipe: r.name = f.has->name_pipe; break;
            case PassKern::Nn: r.name = f.has->name_split; break;
            default: r.name = f.has->name;
            }
        break;
    }
    case S::Quad:
        r.kern = PassKern::Quad; r.chains = chain; r.host_in_place = false; r.name = chain ? "k_chain+k_quad" : "k_quad";
        break;
    case S::Stack:
        r.kern = PassKern::Stack; r.name = "k_stack";
        break;
    case S::Conv:
        r.kern = PassKern::Conv; r.name = "k_conv";
        break;
    case S::ConvMfma:
    case S::ConvMs: {
        // the bare-model modes run unfused; a fused block longer than the kernel's 256 frames goes through in time slices, each the whole
        // run() of its slice
        const bool ms = f.slot.serve() == S::ConvMs, fused = chain && f.slot.fused();
        r.kern = ms ? PassKern::ConvMs : PassKern::ConvMfma;
        r.chains = chain && !fused;
        r.host_in_place = f.slot.fused();
        if (fused && f.n_frames > (p.max_frames < 256 ? p.max_frames : 256)) r.pieces = PassForm::TIME_SLICES;
        // ("k_conv_st": what a block of 64 / 128 / 256 frames runs; every other length: k_conv_ms)
        r.name = ms ? (r.chains ? "k_chain+k_conv_ms" : !fused ? "k_conv_ms" : f.conv_st && p.max_frames >= 64 ? "k_conv_st" : "k_conv_ms")
                    : r.chains ? "k_chain+k_conv_mfma" : "k_conv_mfma";
        break;
    }
    default: {
        // The matrix-core forms of recurrent models. Only the passes themselves take a one-launch or chained kernel: warm-ups (worker stream,
        // next to the passes) and the bare-model modes run on k_mfma, which leaves bit-identical state — two chained grids must never be in
        // flight together. A pass of no frames is the two packed chains.
        const S s = f.slot.serve();
        r.host_in_place = false;
        const bool tick = s == S::GruGm || s == S::GruGs || s == S::LstmGs;
        const bool chained = (s == S::Lp || s == S::Ls) && chained_usable(f.ring_ready, f.hand_over, p.lp_off);
        if (!chain) { r.kern = PassKern::Mfma; r.name = "k_mfma"; }
        else if (tick && frames) {
            r.kern = s == S::GruGm ? PassKern::GruGm : s == S::GruGs ? PassKern::GruGs : PassKern::LstmGs;
            r.name = s == S::GruGm ? "k_gru_gm" : s == S::GruGs ? "k_gru_gs" : "k_lstm_gs";
        } else if (chained) {
            const bool fused = f.slot.fused() && frames, ls = s == S::Ls;
            r.kern = ls ? PassKern::MfmaLs : PassKern::MfmaLp;
            r.chains = !fused;
            if (ls && f.slot.round_streams() && f.n_streams > f.slot.round_streams()) r.pieces = PassForm::STREAM_RANGES;
            static const char* const names[3][2] = { { "k_chain+k_mfma_lp", "k_mfma_lp" }, { "k_chain+k_mfma_ls", "k_mfma_ls" }, { "k_chain+k_mfma_ls1", "k_mfma_ls1" } };
            r.name = names[!ls ? 0 : f.hand_over ? 1 : 2][fused];      // (k_mfma_ls1: the spelling of k_mfma_ls on a lone layer)
        } else { r.kern = PassKern::Mfma; r.chains = true; r.name = "k_chain+k_mfma"; }
        break;
    }
    }
    if (p.bank) r.host_in_place = true;
    return r;
}

}  // namespace aidax
