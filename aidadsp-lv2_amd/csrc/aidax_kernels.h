// aidax_kernels.h — host-callable launchers defined in aidax_kernels.hip.
#pragma once

#include <hip/hip_runtime_api.h>

#include "aidax_layout.h"
#include "aidax_pass_form.h"

namespace aidax {

// One (cell, hidden) pair of the reference's table: its one-wave kernel, the optional forms (nullptr: the cell has none) and, in `has`,
// which of them exist and what they are called — the part the pass-form decision reads (aidax_pass_form.h)
struct KernelEntry {
    int cell, hidden;
    void (*fn)(LaunchArgs);           // one wavefront per stream (throughput form)
    void (*fn_pipe)(LaunchArgs);      // three wavefronts per stream (latency form)
    void (*fn_nn)(LaunchArgs);        // recurrent cell only, between the two packed chain launches (split form)
    void (*fn_pipe4)(LaunchArgs);     // four streams per workgroup, one helper wave (k_*_pipe4)
    void (*fn_pipe4c)(LaunchArgs);    // the same for a conditioned model (PARAM1 / PARAM2 as inputs): the helper wave also runs the PARAM smoothers
    void (*fn_pipe_bank)(LaunchArgs); // fn_pipe with every stream on the model of its own record (LaunchArgs::bank): the model bank's pass
    int pack_regs, state_floats;
    CellKernels has;
};

const KernelEntry* find_kernel(int cell, int hidden);
hipError_t launch_stream_kernel(const KernelEntry* e, const LaunchArgs& a, size_t lds_bytes, hipStream_t stream);
hipError_t launch_nn_kernel(const KernelEntry* e, const LaunchArgs& a, hipStream_t stream);      // the split form's recurrent cell, between two launch_chain_pass (e == nullptr: no model, nothing)
bool split_form_pays(const KernelEntry* e, uint32_t n_frames);
size_t pipe_lds_bytes(int hidden, uint32_t n_frames);
hipError_t launch_pipe_kernel(const KernelEntry* e, const LaunchArgs& a, hipStream_t stream, hipEvent_t done = nullptr);
hipError_t launch_pipe_bank_kernel(const KernelEntry* e, const LaunchArgs& a, hipStream_t stream, hipEvent_t done = nullptr);
int pipe_resident_streams(const KernelEntry* e, uint32_t n_frames, int device);
// k_*_pipe4: a pass of whole 16-frame tiles, whole workgroups of four streams, (the caller checks)
size_t pipe4_lds_bytes(int hidden, uint32_t n_frames, int input_size);
hipError_t launch_pipe4_kernel(const KernelEntry* e, const LaunchArgs& a, hipStream_t stream, hipEvent_t done = nullptr);
size_t stack_lds_bytes(const StackDesc& d, uint32_t n_frames);
size_t conv_lds_bytes(const ConvDesc& d, uint32_t n_frames);
size_t mfma_lds_bytes(const MfmaDesc& d, uint32_t n_frames);
size_t chain_lds_bytes(uint32_t n_frames);
constexpr size_t kChainLdsLimit = 72 * 1024;     // packed chains: eight rows of <= 2048 frames + hand-over slots
// one packed chain launch (8 streams per wave): pre = LPF/pre-gain/EQ(pre) in -> out, else DC/EQ(post)/master in place
hipError_t launch_chain_pass(bool pre, const LaunchArgs& a, hipStream_t stream);
hipError_t launch_mfma_kernel(const LaunchArgs& a, const MfmaDesc& d, hipStream_t stream);
// k_mfma_lp (aidax_mfmalp.hip): stacked models, one workgroup per (16 streams, layer), layers chained through a global ring
bool mfma_lp_serves(const MfmaDesc& d);
size_t mfma_lp_lds_bytes(const MfmaDesc& d, uint32_t n_frames, bool fused = false);
bool mfma_lp_fused_serves(const MfmaDesc& d, uint32_t max_frames);       // the DSP chain inside the same launch: one-layer models (helper waves), stacked models with blocks <= 256 frames
size_t mfma_lp_ring_bytes(const MfmaDesc& d, uint32_t n_streams);
size_t mfma_lp_counter_bytes(const MfmaDesc& d, uint32_t n_streams);
// `fault`: device view of a word in pinned host memory that a workgroup bumps when a hand-over wait timed out
// k_gru_gm (aidax_tick.hip): one-layer GRU on gate-major tiles, the whole run() in one launch (MODE_CHAIN, n_frames > 0)
bool gru_gm_serves(const MfmaDesc& d);
size_t gru_gm_lds_bytes(const MfmaDesc& d, uint32_t n_frames);
hipError_t launch_gru_gm_kernel(const LaunchArgs& a, const MfmaDesc& d, hipStream_t stream);
// k_gru_gs (aidax_tick.hip): k_gru_gm with the recurrent product as bf16 MFMAs of operands split exactly into three bf16
// terms; n_products: 6 (to fp32 rounding) or 9 (every term product)
bool gru_gs_serves(const MfmaDesc& d);
size_t gru_gs_lds_bytes(const MfmaDesc& d, uint32_t n_frames);
hipError_t launch_gru_gs_kernel(const LaunchArgs& a, const MfmaDesc& d, int n_products, hipStream_t stream);
// k_lstm_gs (aidax_tick.hip): the same structure for one-layer LSTMs of 40 (run as 48) / 64 units (pack_mfma's LSTM record at gs_off)
bool lstm_gs_serves(const MfmaDesc& d);
size_t lstm_gs_lds_bytes(const MfmaDesc& d, uint32_t n_frames);
hipError_t launch_lstm_gs_kernel(const LaunchArgs& a, const MfmaDesc& d, int n_products, hipStream_t stream);
hipError_t launch_mfma_lp_kernel(const LaunchArgs& a, const MfmaDesc& d, float* ring, uint32_t* counters, uint32_t* fault, hipStream_t stream, bool fused = false);
// k_mfma_ls (aidax_mfmals.hip): k_mfma_lp's stacked models with the contractions as bf16 MFMAs of operands split exactly into
// three bf16 terms (n_products: 6 or 9); same ring protocol, its own ring geometry (a frame is the h fragments)
bool mfma_ls_serves(const MfmaDesc& d);
size_t mfma_ls_lds_bytes(const MfmaDesc& d, uint32_t n_frames, bool fused = false);
bool mfma_ls_fused_serves(const MfmaDesc& d, uint32_t max_frames);
size_t mfma_ls_ring_bytes(const MfmaDesc& d, uint32_t n_streams);
hipError_t launch_mfma_ls_kernel(const LaunchArgs& a, const MfmaDesc& d, float* ring, uint32_t* counters, uint32_t* fault, int n_products,
                                 hipStream_t stream, bool fused = false);
// k_lstm_q4 (aidax_q4.hip): LSTM-32 snapshot models, four streams per workgroup, the whole run() in one launch
bool q4_serves(int cell, int hidden, int input_size);
size_t q4_lds_bytes(int hidden, uint32_t n_frames);
hipError_t launch_q4_kernel(int hidden, const LaunchArgs& a, hipStream_t stream);     // a.wpack = the pack_q4 record
size_t quad_lds_bytes(int hidden, uint32_t n_frames);
hipError_t launch_quad_kernel(int cell, int hidden, const LaunchArgs& a, const QuadDesc& qd, hipStream_t stream);
hipError_t launch_stack_kernel(const LaunchArgs& a, const StackDesc& d, hipStream_t stream);
size_t convm_lds_bytes(const ConvDesc& d, uint32_t n_frames);
int convm_resident_streams(const ConvDesc& d, uint32_t n_frames, int device);                 // workgroups of the fused form resident at once
hipError_t launch_conv_mfma_kernel(const LaunchArgs& a, const ConvDesc& d, bool fused, hipStream_t stream);   // n_frames <= 256; fused: whole run()
hipError_t launch_conv_kernel(const LaunchArgs& a, const ConvDesc& d, hipStream_t stream);
// k_conv_ms (aidax_convs.hip): the conv stacks conv_ms_shape_ok admits, as bf16 term products; its own history layout (ConvDesc::ms_*)
size_t convs_lds_bytes();
int convs_resident_streams(int device, int st_geo);      // st_geo: the stack's k_conv_st geometry (ConvDesc::st_ok - 1), -1 = none
bool conv_st_block_ok(uint32_t n_frames);                // a block length k_conv_st is compiled for (64 / 128 / 256 frames)
hipError_t launch_conv_ms_kernel(const LaunchArgs& a, const ConvDesc& d, bool fused, hipStream_t stream);   // n_frames <= 256; fused: whole run()
hipError_t launch_set_pending(StreamState* st, uint32_t n_streams, int32_t stream, uint32_t bits, hipStream_t q);
hipError_t launch_init_streams(StreamState* st, uint32_t n, hipStream_t q);
hipError_t launch_stage_params(const StreamState* live, StreamState* staged, uint32_t n, hipStream_t q);
hipError_t launch_install_params(StreamState* live, const StreamState* staged, uint32_t n, hipStream_t q);
hipError_t launch_set_param_targets(StreamState* st, float t0, float t1, hipStream_t q);
hipError_t launch_adopt_dsp(StreamState* dst, const StreamState* src, hipStream_t q);
hipError_t launch_reset_for_model(StreamState* st, float* nn, uint32_t n_streams, uint32_t nn_stride, float p_den, hipStream_t q);

// The cabinet IR stage (aidax_ir_mfma.hip). A pool's history ring: per stream a row of ring_row = R + kIrMirror floats (R a power of two,
// mask = R - 1) whose first kIrMirror slots are repeated behind slot R - 1; `pos` is the ring slot of the block's first frame.
constexpr uint32_t kIrMaxTaps = 8192;          // a pool's default IR capacity (aidax_pool_set_ir_capacity raises it), and the longest fade
constexpr uint32_t kIrMirror = 32;
constexpr uint32_t kIrItemStreams = 64;        // streams of one work item: the 4 x 16 MFMA columns of a k_ir_conv wave
// One work item of k_ir_conv's plan: an IR and up to 64 streams that use it, streams[first .. first + count - 1] in stream order
struct IrItem {
    const uint32_t* frag;        // the IR's A fragments: [n_diag][3 terms][64 lanes][4 words] (pack_ir_fragments)
    uint32_t n_diag, count, first, pad;
};
struct IrArgs {
    const IrItem* items;         // the plan: one item per blockIdx.y
    const uint32_t* streams;     // the items' stream lists, one after the other
    const float* ring;
    float* out;                  // [n_streams][n_frames]
    float* part;                 // n_splits > 1: [n_splits][n_streams][n_frames] partial sums
    uint32_t n_items, n_listed, ring_row, mask, pos, n_streams, n_frames, n_splits;      // n_listed: entries of `streams` the items use;
                                                                                         // n_streams: the pass's (prefix), an entry at or beyond it is skipped
};
uint32_t ir_diagonals(uint32_t n_taps);        // diagonals of 16 frames an IR of n_taps reaches: (n_taps + 30) / 16 + 1
uint32_t ir_windows(uint32_t n_diag);          // 32-frame input windows a wave walks
// workgroups the windows are split over (a wave per SIMD of a device with `cus` CUs, at least four windows each, at most `cap`), for a
// grid of `n_items` work items of up to 64 streams; n_diag: the longest IR's
uint32_t ir_k_splits(uint32_t n_items, uint32_t n_frames, uint32_t n_diag, int cus, uint32_t cap);
hipError_t launch_ir_append(float* ring, uint32_t ring_row, uint32_t mask, uint32_t pos, const float* dry, uint32_t n_streams, uint32_t n_frames,
                            hipStream_t q);
// k_ir_conv (+ k_ir_reduce when n_splits > 1): the rows of the plan's streams = each one's IR over its ring; other rows are not touched
hipError_t launch_ir_conv(const IrArgs& a, hipStream_t q);
// The crossfade of an IR change (k_ir_fade), behind launch_ir_conv of the pass and of its fade-out section: for every entry of `mix`
// (a stream index; kIrFadeDry set: the stream's old side is its dry block, read from the ring at pos + t, else its row of `side`,
// [n_streams][n_frames]) the first `lf` frames of the stream's row of `out` become u[t] old + w[t] new, w[t] = (t + 1) / lf,
// u[t] = (lf - 1 - t) / lf (frame lf - 1 is the new side exactly). 1 <= lf <= n_frames; an entry at or beyond n_streams is skipped.
constexpr uint32_t kIrFadeDry = 0x80000000u;
struct IrFadeArgs {
    const uint32_t* mix;
    const float* side;
    const float* ring;
    float* out;
    uint32_t n_mix, ring_row, mask, pos, n_streams, n_frames, lf;
};
hipError_t launch_ir_fade(const IrFadeArgs& a, hipStream_t q);
// The blend of two IRs (k_ir_mix), behind launch_ir_conv of the pass and of its blend section: for every entry of `list` ALL frames of
// the stream's row of `out` (its A side: the main section's convolution, or the dry block) become u[k] A + w[k] B, B being the stream's
// row of `side` or, with kIrBlendDry set in `stream`, its dry block out of the ring at pos + t. Frame t of the pass is ramp frame
// k = entry.k + k_off + t of a ramp m0 -> m1 over `ramp` frames: for k + 1 < ramp, wd = m0 + (m1 - m0) (k + 1) / ramp in fp64 (one
// subtraction, one multiplication, one division, one addition, each rounded), w = (float)wd, u = (float)(1 - wd); from then on w = m1,
// u = (float)(1 - (double)m1). w == 0 leaves A's bits, w == 1 gives B's, otherwise fmaf(w, B, u * A) with the product rounded to fp32.
// entry.k <= 2^24 and k_off <= 2^25 (the host saturates it: beyond any ramp's end). An entry at or beyond n_streams is skipped.
constexpr uint32_t kIrBlendDry = 0x80000000u;
constexpr uint32_t kIrMaxRamp = 1u << 24;
constexpr uint32_t kIrMaxRampOffset = 1u << 25;
// Frame k of a ramp v0 -> v1 over `ramp` frames, in fp64 with every operation rounded on its own (the sources are built without
// contraction): the ONE statement of it, shared by k_ir_mix and IrPlan::weight (the weight of B) and by k_mix, MixBook and
// aidax_mix_gain (a send's gain). k + 1 must not wrap.
__host__ __device__ inline double ramp_value(float v0, float v1, uint32_t ramp, uint32_t k)
{
    if (k + 1u >= ramp) return static_cast<double>(v1);
    const double step = static_cast<double>(v1) - static_cast<double>(v0);
    const double run = step * static_cast<double>(k + 1u);
    const double part = run / static_cast<double>(ramp);
    return static_cast<double>(v0) + part;
}
struct IrBlendEntry {
    uint32_t stream;
    float m0, m1;
    uint32_t ramp, k;
};
struct IrBlendArgs {
    const IrBlendEntry* list;
    const float* side;
    const float* ring;
    float* out;
    uint32_t n_blend, ring_row, mask, pos, n_streams, n_frames, k_off;
};
hipError_t launch_ir_mix(const IrBlendArgs& a, hipStream_t q);

// The streaming resampler (aidax_resample.hip, k_resample): one launch appends the call's n_in new frames per stream to the history ring
// (per stream a row of mask + 1 floats, frame k in slot k & mask) and writes the call's n_out outputs per stream. Output t of the call has
// the numerator a0 + t M, a0 = q0 L + phi0 (include/aidax.h, "Rate conversion"), and reads the inputs q - H .. q + H around
// q = q0 + (phi0 + t M) / L; input frames are named relative to the first new one (frame -1 is the ring's latest), and frames before
// -n_hist are zeros. Workgroups over (output tile of kRsTile, stream); a call without outputs runs one workgroup per stream for the append.
constexpr uint32_t kRsTile = 256;
constexpr uint32_t kRsWindow = 4096;           // floats of LDS a tile's input window may take; a wider window is read from memory in place
struct ResampleArgs {
    const float* wt;             // the weight rows, transposed: [T][L]
    float* ring;
    const float* in;             // [n_streams][n_in]
    float* out;                  // [n_streams][n_out]
    uint32_t L, M, H, mask, pos; // pos: the ring slot of the first new frame
    uint32_t n_streams, n_in, n_out, n_hist, phi0;
    int32_t q0;                  // relative to the first new frame
    uint32_t copy;               // equal rates: out = x[q], a bit copy
};
uint32_t resample_window(uint32_t L, uint32_t M, uint32_t H);      // floats of a full tile's input window
hipError_t launch_resample(const ResampleArgs& a, hipStream_t q);

// The stream meters (aidax_meter.hip, k_meter): one launch folds the rows of a pass's block, [n_active][n_frames], into the streams'
// records, a wave per stream. MeterRec is aidax_stream_meter of include/aidax.h, field for field. side kMeterIn: the block the pass was
// handed (in_nonfinite, in_energy, in_peak); kMeterOut: the block it returns (every other field, `frames` and `passes` among them).
struct MeterRec {
    uint64_t frames, passes, in_nonfinite, out_nonfinite, out_over;
    double in_energy, out_energy;
    float in_peak, out_peak;
};
static_assert(sizeof(MeterRec) == 64, "a stream's meter record is 64 bytes");
enum { kMeterIn = 0, kMeterOut = 1 };
hipError_t launch_meter(const float* buf, MeterRec* rec, uint32_t n_active, uint32_t n_frames, int side, hipStream_t q);

// The noise gate ahead of the model (aidax_gate.hip, k_gate): one launch turns the block a pass was handed, [n_active][n_frames], into
// the gated block `out` of the same shape (never the same memory), a wave per stream, by the per-frame rule of include/aidax.h ("Noise
// gate"). GateRec is aidax_gate_rec and GateState aidax_gate_state, field for field. A stream whose record is off, or whose control
// record lacks CTL_ENABLED, has its row copied bit for bit and its state left alone.
constexpr uint32_t kGateUnit = 1u << 24;       // P: the attenuation position of a fully closed gate
struct GateRec {
    float t_open, t_close, floor, span;
    uint32_t hold, up, down, on;
};
struct GateState {
    uint32_t hold_left, atten;                 // c, q
};
static_assert(sizeof(GateRec) == 32 && sizeof(GateState) == 8, "a stream's gate record is 32 bytes, its state 8");
hipError_t launch_gate(const float* in, float* out, const GateRec* rec, GateState* state, const StreamCtl* ctl, uint32_t n_active, uint32_t n_frames,
                       hipStream_t q);

// The stream tuners ahead of the model (aidax_tune.hip, k_tune): one launch, a workgroup per stream of the pass, appends the rows of the
// block the pass was handed, [n_active][n_frames], to the tuned streams' history rings (per stream a row of mask + 1 floats, frame p of
// the tuner's count in slot p & mask; mask + 1 >= window + the longest pass) and moves their frame counts; `analyse` also runs the
// analysis of include/aidax.h ("Stream tuners") for every stream whose count crosses a hop boundary (the device decides per stream from
// its own count: the host's mirror, TunerBook, only tells whether any stream of the pass can). TunerReading is aidax_tuner_reading,
// field for field. A stream whose `on` word is 0 is not touched.
constexpr uint32_t kTuneMaxTiles = 9;          // lag tiles of 256: tmax + 1 <= 2048
struct TunerReading {
    uint64_t frame;
    uint32_t analyses, lag;
    float hz, period, clarity, level;
};
static_assert(sizeof(TunerReading) == 32, "a stream's tuner reading is 32 bytes");
struct TuneArgs {
    const float* in;             // [n_active][n_frames]: only read
    float* ring;                 // [n_streams][mask + 1]
    uint64_t* pos;               // [n_streams]
    const uint32_t* on;          // [n_streams]
    TunerReading* reading;       // [n_streams]
    float* curve;                // [n_streams][curve_row]: the NSDF rows, lags 0 .. tmax + 1
    double samplerate;
    uint32_t n_active, n_frames, mask, curve_row;
    uint32_t window, hop, tmin, tmax;
    float threshold, clarity_min, level_min;
};
size_t tune_lds_bytes(uint32_t window, uint32_t tmax);
hipError_t launch_tune(const TuneArgs& a, bool analyse, hipStream_t q);

// The mix buses behind a pool's last stage (aidax_mix.hip, k_mix): one launch gathers the rows of the block a pass returns, [n_streams]
// [n_frames], into the pool's bus block, [n_buses][n_frames], by the rule of include/aidax.h ("Mix buses"). The plan is CSR: the entries
// of bus b are entries[bus_start[b] .. bus_start[b + 1] - 1], in ascending (stream, send) order; frame t of the pass is ramp frame
// k = entry.k + k_off + t of the entry's ramp g0 -> g1 over `ramp` frames (ramp_value; entry.k <= 2^24, k_off <= 2^25: the host
// saturates it). An entry at or beyond n_streams (a prefix pass) is left out. max_entries: the longest bus's entries, which picks the
// one-wave form (every bus of at most kMixGroup entries), the four-wave form (at most 4 kMixGroup) or the sixteen-wave form.
constexpr uint32_t kMixGroup = 32;             // entries of one group sum
constexpr uint32_t kMixMaxRampOffset = 1u << 25;
struct MixEntry {
    uint32_t stream;
    float g0, g1;
    uint32_t ramp, k;
};
struct MixArgs {
    const uint32_t* bus_start;   // [n_buses + 1]
    const MixEntry* entries;
    const float* y;              // the block the pass returns: only read
    float* out;                  // [n_buses][n_frames]
    uint32_t n_buses, n_streams, n_frames, k_off;
};
hipError_t launch_mix(const MixArgs& a, uint32_t max_entries, hipStream_t q);

// The bus limiters behind k_mix (aidax_bus_limit.hip, k_bus_limit): one launch turns the raw bus block k_mix wrote, [n_buses][n_frames],
// into the pool's bus block of the same shape by the per-frame rule of include/aidax.h ("Bus limiters"), a workgroup per bus. LimitRec is
// aidax_bus_limit_rec and BusMeterRec aidax_bus_meter, field for field. Each bus has a row of mask + 1 floats in `ring`, the sanitised
// samples of its past: absolute frame k lives in slot k & mask, `pos` is the absolute frame (modulo 2^32) of the pass's first one, and the
// launch appends the pass's frames. The row holds at least 2 L + H - 1 frames of history next to the longest pass, for every record the
// host admits (lookahead 1 .. kLimitMaxLookahead, hold 0 .. kLimitMaxHold). A bus whose record is off gets the raw bits.
constexpr uint32_t kLimitUnit = 1u << 22;      // U: the gain position of "no reduction"
constexpr uint32_t kLimitMaxLookahead = 512, kLimitMaxHold = 4096;
struct LimitRec {
    float ceiling;
    uint32_t lookahead, hold, on;
};
struct BusMeterRec {
    uint64_t frames, passes, in_nonfinite, limited;
    float in_peak, out_peak, min_gain, reserved;
};
static_assert(sizeof(LimitRec) == 16 && sizeof(BusMeterRec) == 48, "a bus's limiter record is 16 bytes, its meter record 48");
struct BusLimitArgs {
    const float* raw;            // [n_buses][n_frames]: what k_mix wrote, only read
    float* out;                  // [n_buses][n_frames]
    float* ring;                 // [n_buses][mask + 1]
    const LimitRec* rec;         // [n_buses]
    BusMeterRec* meter;          // [n_buses]
    uint32_t n_buses, n_frames, mask, pos;
};
hipError_t launch_bus_limit(const BusLimitArgs& a, hipStream_t q);

// The bus reverbs between k_mix and k_bus_limit (aidax_bus_reverb.hip, k_bus_reverb): one launch reverberates, in place, the block k_mix
// wrote, [n_buses][n_frames], by the per-frame rule of include/aidax.h ("Bus reverbs"), a workgroup per bus. ReverbRec is
// aidax_bus_reverb_rec, field for field. Each bus has eight rows of mask + 1 floats in `ring`, one per delay line: d_i of absolute frame k
// lives in slot k & mask of row i, `pos` is the absolute frame (modulo 2^32) of the pass's first one, and a slot whose frame lies before
// the record's epoch (compared modulo 2^32) reads as 0. A row holds max_delay + 1 frames of history next to the longest pass. A bus whose
// record is off is not touched.
constexpr uint32_t kReverbLines = 8, kReverbMinDelay = 64, kReverbMaxDelay = 32768;
struct ReverbRec {
    uint32_t m[kReverbLines];
    float gq[kReverbLines];
    float a, wet, dry;
    uint32_t on, epoch, reserved[3];
};
static_assert(sizeof(ReverbRec) == 96, "a bus's reverb record is 96 bytes");
struct BusReverbArgs {
    float* block;                // [n_buses][n_frames]: what k_mix wrote, reverberated in place
    float* ring;                 // [n_buses][8][mask + 1]
    const ReverbRec* rec;        // [n_buses]
    uint32_t n_buses, n_frames, mask, pos, max_delay;
};
hipError_t launch_bus_reverb(const BusReverbArgs& a, hipStream_t q);

// The stream delays behind the IR stage (aidax_delay.hip, k_delay): one launch delays, in place, the block a pass returns, [n_active]
// [n_frames], by the per-frame rule of include/aidax.h ("Stream delays"), a workgroup per stream. DelayRec is aidax_delay_rec and
// DelayState aidax_delay_state, field for field. Each stream has one row of mask + 1 floats in `ring`, its line's memory: d of the line's
// frame k lives in slot k & mask, and a frame before the line's frame 0 reads as 0. A row holds cap + 3 frames of history next to the
// longest pass. A stream whose record is off, or whose control record lacks CTL_ENABLED, is not touched: its row keeps its bits and its
// state does not move.
constexpr uint32_t kDelayMin = 64, kDelayMax = 1u << 18, kDelayMaxDepth = 4096, kDelayMaxFade = 1u << 20;
struct DelayRec {
    uint32_t m, depth_q16, lfo_step, fade;
    float fb, damp, wet, dry;
    uint32_t on, reserved[3];
};
struct DelayState {
    uint64_t pos;
    uint32_t m_cur, m_old, fade_len, fade_left, phase, replaced;
};
static_assert(sizeof(DelayRec) == 48 && sizeof(DelayState) == 32, "a stream's delay record is 48 bytes, its state 32");
struct DelayArgs {
    float* block;                // [n_active][n_frames]: what the pass returns, delayed in place
    float* ring;                 // [n_streams][mask + 1]
    const DelayRec* rec;         // [n_streams]
    DelayState* state;           // [n_streams]
    const StreamCtl* ctl;        // [n_streams]
    uint32_t n_active, n_frames, mask, cap;
};
hipError_t launch_delay(const DelayArgs& a, hipStream_t q);

hipError_t launch_keep_warm_kernel(int workgroups, hipStream_t stream);      // an empty grid (AIDAX_KEEP_WARM_US, aidax_pool.cpp)

}  // namespace aidax
