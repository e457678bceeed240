/*
 * aidax.h — C ABI of the MI355X-native rt-neural-generic hot path.
 *
 * This is the drop-in boundary: the reference's LV2 shell keeps its own
 * plumbing (ports, atoms, worker, state) and calls these entry points where it
 * used to call its four private DSP statics (rt-neural-generic.h:321-324) and
 * its model loader. Every entry point cites the reference code it replaces
 * (paths relative to the reference repo root). Plain pointers and sizes only;
 * integer status codes; no exceptions cross this boundary; `process` never
 * allocates. There is NO CPU fallback: without a usable HIP device every
 * device-touching call fails with AIDAX_ERR_DEVICE.
 *
 * One `aidax_pool` = N independent mono streams (N plugin instances' DSP
 * state) sharing one model, resident on one GPU. The reference processes one
 * stream per plugin instance; a host that wants GPU batching aggregates its
 * instances into one pool. The LV2 shell built from
 * aidadsp-lv2_amd/lv2/ uses a pool of N=1 per instance.
 */
#ifndef AIDAX_H
#define AIDAX_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#if defined(__GNUC__)
#define AIDAX_API __attribute__((visibility("default")))
#else
#define AIDAX_API
#endif

/* ------------------------------------------------------------------ status */
enum {
    AIDAX_OK = 0,
    AIDAX_ERR_ARG = -1,        /* null / out-of-range argument                                  */
    AIDAX_ERR_IO = -2,         /* file unreadable                                               */
    AIDAX_ERR_JSON = -3,       /* json malformed or a required key missing ("Unable to load
                                  json file", rt-neural-generic.cpp:1017-1020)                  */
    AIDAX_ERR_ARCH = -4,       /* "Unable to identify a known model architecture!" (:1025-1026),
                                  input_size > 3 (:978-980) or in_skip > 1 (:984-985)           */
    AIDAX_ERR_DEVICE = -5,     /* HIP error / no device / kernels not loadable                  */
    AIDAX_ERR_STATE = -6       /* call not valid in the current state                           */
};

AIDAX_API const char* aidax_last_error(void);      /* thread-local message of the last failure */
AIDAX_API const char* aidax_version(void);

/* ------------------------------------------------------------------- model */
typedef struct aidax_model aidax_model;            /* host-side DynamicModel minus its state
                                                      (rt-neural-generic.h:115-129)             */

enum { AIDAX_CELL_LSTM = 0, AIDAX_CELL_GRU = 1, AIDAX_CELL_CONV = 2 };

typedef struct {
    int32_t cell;              /* AIDAX_CELL_*  (layers[0].type, model_variant.hpp:62-71)       */
    int32_t hidden;            /* layers[0].shape[-1]                                           */
    int32_t input_size;        /* in_shape[-1] in 1..3 (rt-neural-generic.cpp:977-980); this is
                                  also the value of the ModelInSize output port (:518)          */
    int32_t n_rnn_layers;      /* 1 for every architecture the reference can load; >1 or cell ==
                                  CONV are extensions                           */
    int32_t input_skip;        /* in_skip (:982-989)                                            */
    float   input_gain;        /* DB_CO(in_gain) or 1 (:991-996)                                */
    float   output_gain;       /* DB_CO(out_gain) or 1 (:998-1003)                              */
    float   samplerate;        /* metadata.samplerate / samplerate if NUMBER, else 48000 (:1005-1013) */
    int32_t n_golden;          /* length of input_batch/output_batch if both present, else 0    */
    int32_t in_reference_set;  /* 1 if one of the 54 variants of model_variant.hpp:6-59         */
    uint64_t n_weights;
} aidax_model_info_t;

/* loadModelFromPath, parse + architecture match half (rt-neural-generic.cpp:963-1044).
 * Host only; does not touch the GPU. Besides the reference's 54 variants this build loads its extension
 * architectures (n_rnn_layers > 1, wider single layers, conv1d stacks; in_reference_set == 0); with
 * AIDAX_STRICT_REFERENCE_SET=1 in the environment those are rejected with the reference's own message
 * (:1025-1026). The LV2 shell applies that rule by default (AIDAX_STRICT_REFERENCE_SET=0 lifts it). */
AIDAX_API int  aidax_model_load(const char* json_path, aidax_model** out);
AIDAX_API int  aidax_model_load_memory(const char* json_text, size_t len, const char* label, aidax_model** out);
AIDAX_API int  aidax_model_info(const aidax_model* m, aidax_model_info_t* info);
AIDAX_API const char* aidax_model_path(const aidax_model* m);            /* DynamicModel::path */
/* copies min(cap, n_golden) floats of input_batch / output_batch (either may be NULL) */
AIDAX_API int  aidax_model_golden(const aidax_model* m, float* in, float* out, uint32_t cap);
AIDAX_API void aidax_model_free(aidax_model* m);                          /* freeModel :1093-1101 */

/* ---------------------------------------------------------------- controls */
/* The 20 input control ports of the generic build, by value, in TTL order
 * (ports_t rt-neural-generic.h:84-112; ranges/defaults rt-neural-generic.ttl:94-313). */
typedef struct {
    float in_lpf_pc;           /*  4 ANTIALIASING %   */
    float pregain_db;          /*  5 PREGAIN dB       */
    float net_bypass;          /*  6 NETBYPASS        */
    float param1;              /*  7 PARAM1           */
    float param2;              /*  8 PARAM2           */
    float eq_bypass;           /*  9 EQBYPASS         */
    float eq_position;         /* 10 EQPOS 0=post 1=pre */
    float bass_boost_db;       /* 11 BASS             */
    float bass_freq;           /* 12 BFREQ            */
    float mid_boost_db;        /* 13 MID              */
    float mid_freq;            /* 14 MFREQ            */
    float mid_q;               /* 15 MIDQ             */
    float mid_type;            /* 16 MTYPE 0=peak 1=bandpass */
    float treble_boost_db;     /* 17 TREBLE           */
    float treble_freq;         /* 18 TFREQ            */
    float depth_boost_db;      /* 19 DEPTH            */
    float presence_boost_db;   /* 20 PRESENCE         */
    float dc_blocker;          /* 21 DCBLOCKER        */
    float master_db;           /* 22 MASTER           */
    float enabled;             /* 24 enabled          */
} aidax_controls;

AIDAX_API void aidax_controls_default(aidax_controls* c);                /* lv2:default values */

/* Biquad::setBiquad -> calcBiquad (common/Biquad.cpp:60-165): coefficients
 * a0,a1,a2,b1,b2 for (type 0..6, Fc/fs, Q, gain dB). Host only. */
AIDAX_API int aidax_biquad_design(int type, double fc, double q, double gain_db, double coeffs[5]);
/* DB_CO (rt-neural-generic.h:160) and the ANTIALIASING % -> Fc map (.h:167,178-179; cpp:515) */
AIDAX_API float aidax_db_to_coeff(float db);
AIDAX_API float aidax_lpf_fc(float percent);

/* ------------------------------------------------------- device placement
 * The reference's unit of independence is the plugin instance (instantiate(), rt-neural-generic.cpp:244-333; instances
 * share nothing, rt-neural-generic.h:198-239, 311-319), so on a node with several GPUs instances are the thing to spread.
 * aidax_device_count: HIP devices this process sees (0 and AIDAX_ERR_DEVICE without a usable runtime).
 * aidax_pick_device: the placement rule, a pure function (no HIP call): `spec` names the candidates — NULL / "" / "0" the
 * first device (what AIDAX_DEVICE unset means), "auto" every device, else a list of indices and ranges ("0-3,6"); of the
 * candidates below device_count the one with the smallest load[] wins, ties go to the lowest index. load may be NULL (all
 * idle). AIDAX_ERR_ARG when spec is malformed or names no device below device_count. The LV2 shell keeps one load count
 * per device and process (instances in one-stream mode, hubs' seats in hub mode) and asks this function at instantiate()
 * resp. when it opens a hub. */
AIDAX_API int aidax_device_count(int* count);
AIDAX_API int aidax_pick_device(const char* spec, int device_count, const uint32_t* load, int* device_out);
/* aidax_pick_hub: which of the n hubs that serve one model file an instance joins (hub mode of the LV2 shell), a pure function too.
 * hub_device[i] / hub_free_seats[i] describe hub i; current_device is the device of the hub the instance plays in NOW (a model-file
 * swap: work() -> work_response(), rt-neural-generic.cpp:807-893), or -1 for an instance that joins its first hub. An instance
 * that already plays STAYS ON ITS DEVICE — its seven biquad memories and both gain smoothers are carried into the new seat by a
 * device-side copy (aidax_hub_adopt; the reference keeps them across a swap, :868-875), which two pools on different devices
 * cannot do. *index_out: the first hub on that device with a free seat, or -1 = open a new hub, on *device_out. For a first join:
 * the first hub with a free seat whatever its device; else a new hub on the device aidax_pick_device(spec, ...) names.
 * AIDAX_ERR_ARG as for aidax_pick_device, or when current_device is not below device_count. */
AIDAX_API int aidax_pick_hub(const int* hub_device, const uint32_t* hub_free_seats, int n_hubs, int current_device,
                             const char* spec, int device_count, const uint32_t* load, int* index_out, int* device_out);

/* ------------------------------------------------------- launch-form rule (diagnostic)
 * Which kernel family a pool of n_streams instances of a ONE-layer model of the reference's table (cell: AIDAX_CELL_LSTM /
 * AIDAX_CELL_GRU, hidden units) takes on a device with compute_units CUs, beyond the per-stream forms: 0 none (the wavefront /
 * pipeline / split forms, chosen by residency at pool creation), 1 four streams per workgroup on the 4x4 matrix instruction
 * (k_quad), 2 sixteen streams per workgroup on the 16x16 ones (k_gru_gs, k_lstm_gs, k_mfma_ls1, k_mfma_lp, k_mfma). A pure
 * function (no HIP call, environment switches apply): the decision table of csrc/aidax_pool.cpp, measured at 256-frame blocks on
 * 256 CUs; exported so that hosts and tests can see what a pool size will run on. */
AIDAX_API int aidax_many_streams_form(int cell, int hidden, uint32_t n_streams, int compute_units);
/* ... for a pool made for blocks of max_frames frames (the reference's run() is called with the HOST's period, rt-neural-generic.cpp:484:
 * 64 or 128 frames on MOD devices and low-latency set-ups). The table was re-measured at 64 / 128 / 256 frames (profiles/r05_blocklen_forms*.txt):
 * one crossover moves with the block length (LSTM-32 at 5632 .. 6144 streams); aidax_many_streams_form is this function at 256 frames. */
AIDAX_API int aidax_many_streams_form_at(int cell, int hidden, uint32_t n_streams, int compute_units, uint32_t max_frames);

/* ... and which kernel family a conv1d-stack model (an extension of the path: BASELINE config 4) takes, by its shape alone — the packer's
 * rules (csrc/aidax_pack.cpp: conv_ms_shape_ok, conv_st_shape_ok), pure, no HIP call: 0 not a conv model, 1 k_conv (VALU, any stack the
 * loader admits), 2 k_conv_mfma (fp32 matrix instructions: up to sixteen equal channels, a plane that fits LDS), 3 k_conv_ms (bf16 term
 * products: exactly sixteen channels, two to four taps, histories its plane + two register fragments hold), 4 k_conv_ms with FULL 256-frame
 * blocks of the fused form on k_conv_st, the streaming kernel (eight layers of three taps, dilation 2^l). Environment switches of the test
 * build are not applied: this is the shape rule. */
AIDAX_API int aidax_model_conv_form(const aidax_model* m);

/* -------------------------------------------------------------------- pool */
typedef struct aidax_pool aidax_pool;

enum { AIDAX_ALL_STREAMS = -1 };
enum {
    AIDAX_START_WARMUP = 0,    /* release build: 2048-zero pre-buffer through applyModel after
                                  reset() (rt-neural-generic.cpp:1075-1079)                     */
    AIDAX_START_RESET = 1      /* reset() state only (what the DEBUG self-test path leaves)     */
};

/* instantiate(), DSP half (rt-neural-generic.cpp:283-321) for n_streams
 * instances on GPU `device_id`: gain smoothers (T60 0.1 s at host rate, pre
 * target 1, master target 0), the seven biquads, loading = true, no model.
 * max_frames bounds n_frames of every later process call (<= 8192 for the reference's model table; the
 * extension architectures stage whole blocks in LDS and take max_frames <= 2048 (stacked / wide
 * recurrent) resp. <= ~1000 (conv stacks): aidax_pool_set_model reports AIDAX_ERR_ARG beyond that). */
AIDAX_API int  aidax_pool_create(uint32_t n_streams, uint32_t max_frames, double host_samplerate,
                                 int device_id, aidax_pool** out);
AIDAX_API void aidax_pool_destroy(aidax_pool* p);                         /* cleanup() :664-677 */
AIDAX_API uint32_t aidax_pool_streams(const aidax_pool* p);

/* Model swap, split the way the reference splits it between its two threads (:807-893).
 *
 * aidax_pool_prepare_model — work() / loadModelFromPath's device half (:822-836, :1034-1079), WORKER thread:
 *   packs the weights for the kernel form this pool will use, allocates and uploads them, gives every stream
 *   a fresh DynamicModel (reset(), PARAM smoothers rebuilt around the targets the playing model holds at that
 *   moment, :822-825 and :1053-1061) and runs the warm-up per start_mode — all into buffers of its own, on a
 *   stream of its own, while the audio thread keeps playing the old model. Blocks until the model is complete.
 *   model == NULL prepares an unload (no model, loading = true). The caller still owns `m`.
 * aidax_pool_commit_model — work_response() (:859-893), AUDIO thread: swaps the prepared model in and clears
 *   `loading`. Host assignments plus one small kernel on the pool's stream: no allocation, no free, no wait of
 *   any kind. After the call `staged` holds what the swap retired (the previous model's buffers);
 * aidax_staged_free — the reference's kWorkerFree leg (:838-840, :868-875), WORKER thread: frees a staged
 *   object (the retired buffers after a commit; the unused model if it was never committed).
 * aidax_pool_set_model is prepare + commit + free in one blocking call, for hosts without a worker. */
typedef struct aidax_staged aidax_staged;
AIDAX_API int  aidax_pool_prepare_model(aidax_pool* p, const aidax_model* m, int start_mode, aidax_staged** out);
AIDAX_API int  aidax_pool_commit_model(aidax_pool* p, aidax_staged* staged);
AIDAX_API void aidax_staged_free(aidax_staged* staged);
AIDAX_API int  aidax_pool_set_model(aidax_pool* p, const aidax_model* m, int start_mode);

/* Per-stream amp models: a bank of AIDAX_MODEL_SLOTS slots per pool beside the pool model above, and per stream the model it plays:
 * AIDAX_MODEL_POOL (the default: whatever aidax_pool_set_model / commit_model put there) or a bank slot 0 .. 63. The bank holds WEIGHT
 * VARIANTS OF THE POOL MODEL'S ARCHITECTURE: a slot's model has the pool model's cell, hidden size, input_size and sample rate, and brings
 * its own weights, in_gain, out_gain and in_skip. The pool model keeps deciding everything else (state layout, the PARAM smoothers' time
 * constant, the launch geometry). Opt-in: a pool that never prepares a slot allocates nothing for the bank, and while no stream is assigned
 * to a slot (slots loaded or not) every pass issues exactly the launches it issues without a bank, bit for bit. While at least one stream
 * is assigned, every pass of the pool — any block length, zero-length and ragged blocks, any pool size, prefix passes, passes under a rate
 * adapter — goes out as ONE launch of k_lstm_pipe_bank<H> / k_gru_pipe_bank<H> (the three-wave pipeline with every workgroup reading the
 * model of its own stream; streams on AIDAX_MODEL_POOL read the pool model's), and aidax_pool_kernel_name says so. A banked stream's
 * output and state are bit-identical to the same stream of a pool whose pool model is that file, run on k_*_pipe.
 * aidax_model_bank_compatible    pure (no device, any thread): AIDAX_OK when both models are one-layer LSTM / GRU models of the table with
 *                                the same cell, hidden size, input_size and sample rate; else AIDAX_ERR_ARCH with the differing field in
 *                                aidax_last_error(). in_skip, in_gain and out_gain may differ: they travel with the slot.
 * aidax_pool_prepare_model_slot  WORKER thread: packs m's weights in the pool model's layout, allocates and uploads them on the worker
 *                                stream, blocks until complete; m == NULL prepares emptying the slot. The first successful call also
 *                                allocates the per-stream selection records, so no audio-side call ever allocates. Commit with
 *                                aidax_pool_commit_model: the staged object knows its slot and afterwards holds what the commit retired,
 *                                behind the usual fence (aidax_staged_free at any time after the commit). AIDAX_ERR_ARG for slot >=
 *                                AIDAX_MODEL_SLOTS; AIDAX_ERR_STATE when the pool has no model; AIDAX_ERR_ARCH, with the reason, when m
 *                                is not compatible with the pool's model, when the pool's model is not served as a table model at this
 *                                pool size (a pool on k_quad or a matrix-core kernel carries no bank), when the cell has no three-wave
 *                                pipeline (LSTM-64 / 80), or when max_frames does not fit the pipeline's LDS.
 * aidax_pool_set_model_slot      prepare_model_slot + commit + free in one blocking call.
 * aidax_pool_assign_model        AUDIO side, between passes: ONE stream (AIDAX_ALL_STREAMS is not accepted) plays `slot` from the next
 *                                pass on. No allocation, no free, no wait: host records plus the launches aidax_pool_reset_stream issues,
 *                                on the pool's stream. The stream gets what the reference's swap gives an instance (:822-825, :868-875,
 *                                :1046-1079): a fresh DynamicModel (recurrent state zero, PARAM smoothers rebuilt around the targets they
 *                                hold now, paramFirstRun set) and, with AIDAX_START_WARMUP, 2048 zeros through applyModel with the NEW
 *                                slot's weights and gains; the seven biquad memories and both gain smoothers stay, and `loading` is not
 *                                touched (a host that wants the reference's mute around the swap uses aidax_pool_set_loading). Assigning
 *                                the slot a stream already has is a reload: still a fresh DynamicModel. AIDAX_ERR_ARG for a stream or
 *                                slot out of range or a bad start_mode, AIDAX_ERR_STATE for an empty slot or a pool without a model.
 * aidax_pool_stream_model        the assignment of one stream (AIDAX_ERR_ARG for a stream out of range).
 * The rules:
 *  - A commit into a slot (content or NULL) while any stream is assigned to it returns AIDAX_ERR_STATE and changes nothing. To replace a
 *    model: load a free slot, move the streams, empty the old one.
 *  - aidax_pool_commit_model of a POOL model (or of an unload) returns AIDAX_ERR_STATE ("empty the model bank first") and changes nothing
 *    while any stream is assigned to a slot, or while a loaded slot is not compatible with the model being committed (for an unload: while
 *    any slot is loaded). With an empty bank it behaves bit for bit as without one.
 *  - The commit of a slot re-checks compatibility against the pool's current model (host integers only): AIDAX_ERR_STATE if the pool
 *    model changed since the prepare.
 *  - aidax_pool_reset_stream keeps the assignment and warms up with the assigned slot's weights, gains and skip.
 *  - Each pass runs with the assignments and slot contents in force when it was issued (also the blocks in flight through
 *    aidax_pool_submit*, passes on a caller's stream, prefix passes and passes under the rate adapter): the per-stream records reach the
 *    device stream-ordered from a ring of four pinned snapshots, like the control records.
 *  - k_*_pipe4, the split form, k_quad and the matrix-core kernels are not used while the bank is in force. */
#define AIDAX_MODEL_SLOTS 64
enum { AIDAX_MODEL_POOL = -1 };
AIDAX_API int  aidax_model_bank_compatible(const aidax_model* pool_model, const aidax_model* m);
AIDAX_API int  aidax_pool_prepare_model_slot(aidax_pool* p, uint32_t slot, const aidax_model* m, aidax_staged** out);
AIDAX_API int  aidax_pool_set_model_slot(aidax_pool* p, uint32_t slot, const aidax_model* m);
AIDAX_API int  aidax_pool_assign_model(aidax_pool* p, int32_t stream, int32_t slot, int start_mode);
AIDAX_API int  aidax_pool_stream_model(const aidax_pool* p, uint32_t stream, int32_t* slot);

/* Cabinet impulse response (IR): an optional last stage of every stream's run(), after the master gain ramp (rt-neural-generic.cpp:654-655).
 * A pool holds one pool IR h[0..L-1] (fp32, 1 <= L <= 8192: the length of the cabinet IRs the reference ships next to its models; up to 65536
 * in a pool whose IR capacity was raised, see "IR capacity" below) and a bank
 * of per-stream IRs (below); while it does, the output block of every stream that follows it (by default, all of them) is the causal
 * convolution of the block the pool would have returned without it (`dry`) with h:
 *     y[s][t] = sum_{k < L} h[k] * dry[s][t - k]
 * whatever the stream's `enabled` control says (the cabinet sits after the plugin). No latency, any block length the pool takes; n_frames == 0
 * touches nothing. The IR is applied by the matrix cores (k_ir_conv) to fp32 accuracy, and an IR of a single tap that is a power of two
 * (a delay, a gain of 2^-k) reproduces the dry signal exactly. Output is deterministic (the same inputs give the same bits).
 * History: the first aidax_pool_prepare_ir allocates, per stream, a ring of the latest dry samples in device memory; from then on every
 * pass feeds it, also while no IR is attached, so an IR committed later starts on the true past. Samples from before that first prepare,
 * or from before a stream's aidax_pool_reset_stream, count as 0. A pool that was never given an IR allocates and launches nothing for it.
 * The IR swap is split between the threads like a model swap:
 * aidax_ir_load_wav      host only: RIFF/WAVE, PCM 16 / 24 / 32-bit, IEEE float 32-bit, WAVE_FORMAT_EXTENSIBLE of either; channel 0 of
 *                        a multi-channel file; integers scaled to [-1, 1) by 2^(bits-1); unknown chunks skipped. Copies min(cap, frames)
 *                        samples to `taps` (cap == 0: only *n_frames and *samplerate; taps may then be NULL) and reports the file's frame
 *                        count and rate. AIDAX_ERR_IO when the file cannot be read, AIDAX_ERR_ARG (with the reason in aidax_last_error)
 *                        for a malformed or unsupported file: truncated chunks, a data size past the end of the file, no frames, other tags.
 * aidax_pool_prepare_ir  WORKER thread: the history on first use, the IR packed into the kernel's operand form and uploaded on the worker
 *                        stream; blocks until done. taps == NULL prepares the removal of the IR. AIDAX_ERR_ARG for L == 0 or L > the pool's
 *                        IR capacity (8192 unless raised), a tap that is not finite, or a samplerate other than the pool's host rate: this
 *                        call converts nothing, aidax_ir_resample (below) brings an IR to the pool's rate first.
 * aidax_pool_commit_ir   AUDIO thread, between passes: swaps the prepared IR in (no allocation, no free, no wait); `staged` then holds
 *                        the retired IR for aidax_staged_free on the worker.
 * aidax_pool_set_ir      prepare + commit + free in one blocking call.
 * aidax_pool_process with an IR: the pass's completion word is written behind the IR stage, never by the model's kernel. */
AIDAX_API int  aidax_ir_load_wav(const char* path, float* taps, uint32_t cap, uint32_t* n_frames, double* samplerate);
AIDAX_API int  aidax_pool_prepare_ir(aidax_pool* p, const float* taps, uint32_t n_taps, double samplerate, aidax_staged** out);
AIDAX_API int  aidax_pool_commit_ir(aidax_pool* p, aidax_staged* staged);
AIDAX_API int  aidax_pool_set_ir(aidax_pool* p, const float* taps, uint32_t n_taps, double samplerate);

/* Per-stream IRs: a bank of AIDAX_IR_SLOTS slots per pool beside the pool IR above, and per stream the IR its output goes through:
 * AIDAX_IR_POOL (the default: the pool IR, whatever aidax_pool_set_ir / commit_ir put there), AIDAX_IR_NONE, or a bank slot 0 .. 63.
 * A stream on AIDAX_IR_NONE, on an empty slot or on the pool IR while the pool has none returns its dry block. The history above is per
 * stream and does not depend on the assignment: a stream moved to another IR at a block boundary hears the new IR applied to its whole
 * past, and a commit into a slot switches all of that slot's streams at the same block boundary. aidax_pool_reset_stream clears the
 * stream's history and keeps its assignment; a pool that never prepared an IR of either kind allocates and launches nothing for the stage,
 * assignments or not. Each pass runs with the assignments and slots in force when it was issued (also the blocks in flight through
 * aidax_pool_submit, and passes on a caller's stream). One k_ir_conv launch per pass, whatever the number of distinct IRs; with every stream
 * on one IR (the pool IR or any one slot) the output is bit-identical to that IR as the pool IR.
 * aidax_pool_prepare_ir_slot  WORKER thread: as aidax_pool_prepare_ir, into bank slot `slot` (taps == NULL: prepares emptying it); the
 *                             first prepare of either kind allocates the history. AIDAX_ERR_ARG also for slot >= AIDAX_IR_SLOTS. Commit
 *                             with aidax_pool_commit_ir: the staged object knows its slot, and holds the retired fragments afterwards.
 * aidax_pool_set_ir_slot      prepare_ir_slot + commit + free in one blocking call.
 * aidax_pool_assign_ir        AUDIO thread: stream (AIDAX_ALL_STREAMS: every stream) goes through `slot` from the next pass on. No
 *                             allocation, no free, no wait. AIDAX_ERR_ARG for a stream or slot out of range.
 * aidax_pool_stream_ir        the assignment of one stream (AIDAX_ERR_ARG for a stream out of range). */
#define AIDAX_IR_SLOTS 64
enum { AIDAX_IR_POOL = -1, AIDAX_IR_NONE = -2 };
AIDAX_API int  aidax_pool_prepare_ir_slot(aidax_pool* p, uint32_t slot, const float* taps, uint32_t n_taps, double samplerate, aidax_staged** out);
AIDAX_API int  aidax_pool_set_ir_slot(aidax_pool* p, uint32_t slot, const float* taps, uint32_t n_taps, double samplerate);
AIDAX_API int  aidax_pool_assign_ir(aidax_pool* p, int32_t stream, int32_t slot);
AIDAX_API int  aidax_pool_stream_ir(const aidax_pool* p, uint32_t stream, int32_t* slot);

/* IR fade: a change of IR without a click. A pool has an IR fade length F in frames (0, the default: off, and everything above holds
 * bit for bit). With F > 0, call the IR a stream's output actually goes through its effective IR: the pool IR, a bank slot's content, or
 * nothing (AIDAX_IR_NONE, an empty slot, the pool IR while the pool has none). When a stream's effective IR in the pass being issued
 * differs from the one in the last pass issued (after aidax_pool_assign_ir, a commit into its slot, a commit or removal of the pool IR,
 * or any combination: the changes between two passes collapse into one, and A -> B -> A is no change), that one pass returns
 *     y[t] = (1 - w[t]) (h_old * x)[t] + w[t] (h_new * x)[t],   w[t] = min(1, (t + 1) / Lf),   Lf = min(F, n_frames)
 * for that stream, x being its dry history including this block and "nothing" the unit impulse (that side is the dry block). The fade
 * ends inside the pass: its frames t >= Lf, and every later pass, are bit-identical to a pool that had the new IR all along, and so is
 * every stream whose effective IR did not change. A pass of n_frames == 0 leaves a pending fade pending. Each pass runs with the fade,
 * plan and assignments in force when it was issued (blocks in flight through aidax_pool_submit and passes on a caller's stream too).
 * A fade pass costs a second k_ir_conv launch (the old IRs, over the fading streams only) and k_ir_fade; a pass without a pending fade
 * issues exactly the launches of a pool without a fade length. Deterministic like the stage itself.
 * Lifetime: with F > 0 a commit does not hand the fragments it retires to `staged` if they have been played; it parks them in the pool,
 * one parked IR per slot and one for the pool IR, for the fade pass to read, and `staged` receives what was parked there before (an IR
 * retired one commit earlier, whose last use precedes the commit's fence). Content that is retired before any pass was issued with it
 * goes to `staged` at once and the parked IR stays. So aidax_staged_free may run at any time after the commit, as ever, also before
 * the fade pass is issued; parked fragments are freed by a later retirement's aidax_staged_free or by aidax_pool_destroy. With this
 * scheme a slot committed twice (or more) between two passes still fades, from the content last played to the content last committed.
 * What does not fade: a pool's very first pass (there is no earlier pass to differ from), and a stream whose old IR was retired while
 * F was 0: it switches at the block boundary as with F == 0. The crossfade's side buffer (n_streams x max_frames floats) is allocated
 * with the history, by the first prepare of either kind, so the fade length may be set and changed at any time between passes.
 * Prefix passes of the hub fade the streams of the prefix; the others switch.
 * aidax_pool_set_ir_fade   AUDIO thread, between passes: host records only. AIDAX_ERR_ARG for a null pool or frames > 8192.
 * aidax_pool_ir_fade       the fade length (0 for a null pool). */
AIDAX_API int      aidax_pool_set_ir_fade(aidax_pool* p, uint32_t frames);
AIDAX_API uint32_t aidax_pool_ir_fade(const aidax_pool* p);

/* IR blend: a stream through two IRs at once, and crossfades longer than a pass. Besides its assignment A (aidax_pool_assign_ir) a stream
 * has a second assignment B (AIDAX_IR_NONE by default) and a mix w in [0, 1], the weight of B (0 by default):
 *     y[t] = u (h_A * x)[t] + w (h_B * x)[t]
 * with "nothing" on either side (AIDAX_IR_NONE, an empty slot, the pool IR of a pool without one) the unit impulse: that side is the dry
 * block, so B = AIDAX_IR_NONE with a mix is a wet / dry control. The mix moves in ramps that outlive a pass. m_now is the fp32 weight of
 * the last frame issued for the stream (0 for a stream that never had a mix); aidax_pool_set_ir_mix(.., mix, R) starts a ramp from
 * m0 = m_now to m1 = mix whose frame k = 0 is the stream's next issued frame (several calls between two passes: the last one wins, m0 is
 * unchanged; a ramp between equal weights has ended when it is set). Ramp frame k has, in fp64 with every operation rounded on its own,
 *     k + 1 <  R:  wd = (double)m0 + ((double)m1 - (double)m0) * (double)(k + 1) / (double)R,  w = (float)wd,  u = (float)(1.0 - wd)
 *     k + 1 >= R:  w = m1,  u = (float)(1.0 - (double)m1)                                    (R = 0: a jump at the block boundary)
 * and k counts the stream's issued frames, not passes: a ramp's weights do not depend on how the host cuts the stream into blocks. A frame
 * with w == 0 returns A's bits, one with w == 1 B's, any other fmaf(w, yB, u * yA) with the product rounded to fp32 (k_ir_mix).
 * At rest: a stream all of whose coming frames have a weight of exactly 0 or 1 is an ordinary one-IR stream. It costs and returns exactly
 * what a stream assigned to that IR (A on 0, B on 1) returns, and that IR is its effective IR in the sense of the IR fade. Every pass issued
 * after the one in which a ramp ends on 0 or 1 is bit-identical, for that stream, to a pool in which the stream was assigned that IR with
 * aidax_pool_assign_ir. Coming to rest and leaving rest is never an IR change for the IR fade. A stream that rests strictly inside (0, 1)
 * stays blended at a constant weight.
 * While blended (a ramp is running, or the stream rests inside (0, 1)) a change of A or B (an assignment, a commit into the slot that side
 * plays) takes effect on that side at the block boundary, unfaded: to replace a cabinet without a click, move the mix off that side first
 * (INTEGRATION.md). The IR fade applies to a stream only when it is at rest in the last pass issued and in this one.
 * Ramp positions are host integers, advanced by n_frames for the streams of every pass issued (not by a pass of 0 frames or one that failed
 * on its way; a prefix pass of the hub advances the streams of the prefix). Each pass runs with the weights in force when it was issued
 * (blocks in flight through aidax_pool_submit and passes on a caller's stream too). aidax_pool_reset_stream keeps A, B and the mix, and a
 * running ramp goes on. A pass with blended streams costs one more k_ir_conv launch (the B sides, over the blended streams only) and
 * k_ir_mix; a running ramp uploads no plan, and a pass without a blended stream issues exactly the launches it issued before. In a pool
 * that never prepared an IR the stage does not run and both sides are the dry block: the output is the dry block, the ramps run on.
 * aidax_pool_assign_ir_b     AUDIO thread, between passes: the stream's (AIDAX_ALL_STREAMS: every stream's) B is `slot`: AIDAX_IR_POOL,
 *                            AIDAX_IR_NONE or 0 .. 63. Host records only: no allocation, no free, no wait.
 * aidax_pool_set_ir_mix      AUDIO thread, between passes: a ramp to `mix` over `ramp_frames` frames (AIDAX_ALL_STREAMS: every stream from
 *                            its own m_now). Host records only. AIDAX_ERR_ARG for a null pool, a stream or slot out of range, a mix that is
 *                            not finite or outside [0, 1], ramp_frames > 2^24 (both calls; a refused call changes nothing).
 * aidax_pool_stream_ir_mix   the state behind the last pass issued (any pointer may be NULL): B, m_now, the ramp's target, and the frames
 *                            still to be issued until m_now is the target (0: the ramp has ended; a jump has 1 until a frame is issued). */
AIDAX_API int aidax_pool_assign_ir_b(aidax_pool* p, int32_t stream, int32_t slot);
AIDAX_API int aidax_pool_set_ir_mix(aidax_pool* p, int32_t stream, float mix, uint32_t ramp_frames);
AIDAX_API int aidax_pool_stream_ir_mix(const aidax_pool* p, uint32_t stream, int32_t* slot_b, float* mix_now, float* mix_target, uint32_t* frames_left);

/* IR rate conversion (host only: no device, no pool, any thread). The IRs the reference ships, like most commercial cabinet IRs, are
 * 48 kHz files; a pool at another host rate plays them after
 * aidax_ir_resample   `in` (n_in taps at rate_in) converted to rate_out by a Kaiser-windowed sinc. Both rates are positive integers (as
 *                     doubles, <= 2^24); with L / M = rate_out / rate_in in lowest terms, c = min(1, L / M), Z = 32 zero crossings a side
 *                     and beta = 12,
 *                         out[i] = (M / L) sum_k in[k] c sinc(c u) K(c u / Z),   u = ((i - lead) M - k L) / L,
 *                         K(v) = I0(beta sqrt(1 - v^2)) / I0(beta) for |v| < 1, else 0,
 *                     evaluated in fp64 from the exact integer (i - lead) M - k L (the sine from its residue, so an integer u weighs
 *                     exactly 0, and 1 at u = 0) and rounded once to fp32. The factor M / L keeps the frequency response of the filter
 *                     that the IR is (sum out ~ sum in): the cabinet sounds as loud at either rate. Equal rates give a bit copy of `in`
 *                     behind `lead` zeros; a ratio L / M = r of 2 or 4 gives out[lead + r k] == in[k] / r bit for bit. The same inputs
 *                     give the same bits.
 *                     lead: output frame i stands for time (i - lead) / rate_out. A band-limited copy of a causal IR rings before
 *                     t = 0, over ceil(Z max(1, L / M)) frames; `lead` (0 .. 1024) of those frames are kept, frames before the
 *                     kernel's support are zeros, and the caller reports `lead` frames to its host as latency. lead = 0 cuts the
 *                     pre-ringing off for a cabinet without latency, at the price of an error in the passband response of about
 *                     0.1 % from 48 to 44.1 kHz and about 2 % going up (1.1e-3 / 1.9e-2 / 2.3e-2 of max |H| to 44.1 / 96 / 192 kHz
 *                     on a decaying-noise IR of 8192 taps).
 *                     Length: *n_full = lead + floor((n_in - 1 + Z / c) L / M) + 1 frames hold the whole support (16447 for 8192 taps
 *                     from 48 to 96 kHz); min(cap, *n_full) are written to `out`; cap == 0 with out == NULL asks for *n_full alone, as
 *                     in aidax_ir_load_wav. A result cut short by `cap` ends abruptly: no fade is applied to its tail.
 *                     AIDAX_ERR_ARG for a null `in` or `n_full` (or `out` with cap > 0), n_in == 0, a tap that is not finite, a rate
 *                     that is not a positive integer, lead > 1024, or a result of 2^31 frames or more. At most
 *                     *n_full x 2 Z max(1, M / L) kernel values; about 2 ms on one host core for 8192 taps from 48 to 44.1, 96 or 192 kHz
 *                     (the weights of a ratio with max(L, M) <= 4096 are tabulated once per call), 40 ms for an odd ratio such as 48000 : 44101. */
AIDAX_API int      aidax_ir_resample(const float* in, uint32_t n_in, double rate_in, double rate_out, uint32_t lead, float* out, uint32_t cap,
                                     uint32_t* n_full);

/* IR capacity: the longest IR a pool takes, 8192 taps by default and up to AIDAX_IR_MAX_CAPACITY for a pool that asks. An 8192-frame
 * 48 kHz cabinet is about 16 450 taps at a 96 kHz host and 32 830 at 192 kHz; 65536 taps are 1.36 s at 48 kHz. The capacity sizes the
 * history: the first prepare of either kind allocates n_streams x (R + 32) x 4 bytes of ring, R the power of two >= capacity +
 * max_frames (1024 streams x 256 frames: 67 MB at the default, 537 MB at 65536). The stage's work per block is linear in the taps of
 * the IRs in use, not in the capacity; a pool that never raises it allocates and launches exactly what it did before this call existed.
 * The fade length keeps its limit of 8192 frames.
 * aidax_pool_set_ir_capacity  SET-UP side, before the pool's first aidax_pool_prepare_ir / _ir_slot (and not concurrently with it):
 *                             a host record. AIDAX_ERR_ARG for a null pool or max_taps outside 8192 .. 65536, AIDAX_ERR_STATE once
 *                             the history has been allocated.
 * aidax_pool_ir_capacity      the capacity in taps (0 for a null pool). */
#define AIDAX_IR_MAX_CAPACITY 65536
AIDAX_API int      aidax_pool_set_ir_capacity(aidax_pool* p, uint32_t max_taps);
AIDAX_API uint32_t aidax_pool_ir_capacity(const aidax_pool* p);

/* Rate conversion: a model at its trained rate inside a host at another. An AIDA-X model is a nonlinear filter trained at one rate
 * (aidax_model_info_t.samplerate, 48 kHz for the bundled files; the reference leaves the mismatch open, rt-neural-generic.cpp:348). The
 * host creates the pool at the MODEL's rate, so the EQ, the gain smoothers and any IR keep their frequencies and times, and wraps it in a
 * rate adapter at its own rate: every block is converted on the device, host -> pool rate, the pool's pass, pool -> host rate, with
 * per-stream history. A pool that is never wrapped allocates and launches exactly what it did before these calls existed.
 *
 * aidax_resampler: the streaming polyphase resampler underneath, for n_streams streams. It is the window of aidax_ir_resample applied to
 * a signal (no M / L factor): Z = 32, beta = 12, L / M = rate_out / rate_in in lowest terms, D = max(L, M), c = min(1, L / M),
 * H = ceil(Z D / L), T = 2 H + 1. For the output index j >= 0, counted since creation and shared by all streams,
 *     a = (j - d_out) M - d_in L   (exact integers),   q = floor(a / L),   phi = a - q L
 *     out[s][j] = sum_{i = -H .. H} w_phi[i + H] x[s][q - i]
 *     w_phi[i + H] = c sinc(c (phi + i L) / L) K(c (phi + i L) / (L Z)),   rounded once from fp64 to fp32
 * with K and the exact-integer sine of aidax_ir_resample (an integer argument weighs exactly 0, and exactly 1 at 0). x[k] = 0 for k < 0
 * and for frames from before the stream's last reset; d_in and d_out are integer delays in input and output frames, fixed at creation
 * (0 .. 65536). The L rows of T weights are built on the host in fp64 at creation and uploaded once. Both rates are positive integers
 * <= 2^24 with max(L, M) <= 640: every pair of 44.1 / 48 / 88.2 / 96 / 176.4 / 192 kHz (the longest rows, T = 281, at 192 -> 44.1 kHz);
 * anything else is AIDAX_ERR_ARG with the reason. Equal rates are legal: the row is a delta, the stage a pure delay and a bit copy.
 * Sums are fp32, one fixed order per output sample: the same inputs give the same bits, and the bits of an output do not depend on how
 * the input was cut into calls.
 * aidax_resampler_create          SET-UP side: the weight table, per stream a history ring (the power of two >= T + 2 max_in_frames +
 *                                 2 ceil(M / L) + 2 frames) and the staging of aidax_resampler_process on device `device_id`. n_streams 1 .. 65535.
 * aidax_resampler_row             host only and pure: row `phase` (0 .. L - 1) of the filter, min(cap, T) weights to `w`, T to *n_taps
 *                                 (cap == 0 with w == NULL asks for T alone).
 * aidax_resampler_process_device  appends n_in frames per stream, laid out [n_streams][n_in], then writes the next n_out outputs, laid
 *                                 out [n_streams][n_out] (another buffer than d_in). Either count may be 0. One kernel launch,
 *                                 asynchronous on `hip_stream` (NULL: the resampler's own stream), no host sync; consecutive calls on
 *                                 different streams are ordered by an event edge. AIDAX_ERR_STATE, with nothing appended, when an output
 *                                 is asked for whose row reaches past the inputs received (q + H >= frames received), or when outputs
 *                                 of earlier calls were left untaken for so long that the new frames would overwrite history they need
 *                                 (more than about max_in_frames behind). AIDAX_ERR_ARG for n_in > max_in_frames or n_out > 2^20.
 * aidax_resampler_process         the same with host buffers, blocking (pinned staging allocated at creation; waits for the
 *                                 resampler's stream only); at most ceil((max_in_frames + T) L / M) + 2 outputs a call.
 * aidax_resampler_ready           how many outputs may be asked for now.
 * aidax_resampler_reset_stream    that stream's past counts as zeros from here on (ordered behind the calls issued so far); the output
 *                                 index goes on.
 *
 * aidax_rate: the adapter around a pool. With r = pool_rate / host_rate = La / Ma, stage A converts host -> pool with d_in = H_A,
 * d_out = 0, stage B pool -> host with d_in = 0, d_out = d_B = ceil((H_B + 1) Ma / La). A call of n host frames that brings the total
 * received to N gives stage A the n frames and takes m = floor(N r) - floor((N - n) r) pool frames from it, runs the pool's pass over
 * those m frames (m == 0: the legal pre-run), gives them to stage B and takes exactly n host frames. With these delays every row ends
 * inside the frames received, for any block size down to 1, and m differs by at most one from call to call. The latency is the integer
 * H_A + d_B host frames: 66 at 44.1 -> 48 kHz, 130 at 96 -> 48, 260 at 192 -> 48, 71 at 48 -> 44.1; report it to the host. Equal rates:
 * the adapter forwards to the pool, latency 0, bit-identical to aidax_pool_process.
 * aidax_pool_samplerate      the rate the pool was created at.
 * aidax_rate_create          SET-UP side: borrows `pool`, which must outlive the adapter. While the adapter exists blocks go through it,
 *                            not through the pool's own process calls; every other call (model, controls, IRs, reset) stays on the pool.
 *                            AIDAX_ERR_ARG for rates the resampler refuses (the pool's included) and when ceil(max_frames r) exceeds the
 *                            pool's max_frames.
 * aidax_rate_destroy         SET-UP side: waits for the adapter's passes and puts the pool back on its own stream, without a pass.
 * aidax_rate_latency_frames  H_A + d_B (0 at equal rates).
 * aidax_rate_latency         the same, pure and host only, for a host that reports its latency before it builds anything.
 * aidax_rate_process         AUDIO side, blocking, host buffers laid out [n_streams][n] (in place allowed): the adapter's own pinned
 *                            staging, waits for its stream only; a pool pass that went wrong is reported as aidax_pool_process
 *                            reports it (silence and AIDAX_ERR_DEVICE). n == 0 runs the pool's pre-run and moves nothing else.
 * aidax_rate_process_device  AUDIO side, asynchronous on `hip_stream` (NULL: the adapter's own stream), device buffers, d_out another
 *                            buffer than d_in; a stream handed in stays valid as for aidax_pool_process_device.
 * aidax_rate_reset_stream    AUDIO side: both stages' history of that stream; the caller resets the pool's stream itself.
 * None of the processing calls allocates or frees. */
typedef struct aidax_resampler aidax_resampler;
typedef struct aidax_rate aidax_rate;
AIDAX_API int      aidax_resampler_create(uint32_t n_streams, double rate_in, double rate_out, uint32_t d_in, uint32_t d_out,
                                          uint32_t max_in_frames, int device_id, aidax_resampler** out);
AIDAX_API void     aidax_resampler_destroy(aidax_resampler* rs);
AIDAX_API int      aidax_resampler_row(double rate_in, double rate_out, uint32_t phase, float* w, uint32_t cap, uint32_t* n_taps);
AIDAX_API int      aidax_resampler_process_device(aidax_resampler* rs, const float* d_in, uint32_t n_in, float* d_out, uint32_t n_out,
                                                  void* hip_stream);
AIDAX_API int      aidax_resampler_process(aidax_resampler* rs, const float* in, uint32_t n_in, float* out, uint32_t n_out);
AIDAX_API uint32_t aidax_resampler_ready(const aidax_resampler* rs);
AIDAX_API int      aidax_resampler_reset_stream(aidax_resampler* rs, uint32_t stream);
AIDAX_API double   aidax_pool_samplerate(const aidax_pool* p);
AIDAX_API int      aidax_rate_create(aidax_pool* pool, double host_rate, uint32_t max_frames, aidax_rate** out);
AIDAX_API void     aidax_rate_destroy(aidax_rate* r);
AIDAX_API uint32_t aidax_rate_latency_frames(const aidax_rate* r);
AIDAX_API int      aidax_rate_latency(double host_rate, double pool_rate, uint32_t* frames);
AIDAX_API int      aidax_rate_process(aidax_rate* r, const float* in, float* out, uint32_t n_frames);
AIDAX_API int      aidax_rate_process_device(aidax_rate* r, const float* d_in, float* d_out, uint32_t n_frames, void* hip_stream);
AIDAX_API int      aidax_rate_reset_stream(aidax_rate* r, uint32_t stream);

/* Stream meters: what is on each stream of a pool, computed where the blocks are. Opt-in: a pool that never switches them on allocates
 * and launches exactly what it did before these calls existed, bit for bit, and a metered pool's audio is bit-identical to an unmetered
 * pool's (the meters only read). While metering is on, every pass of n_frames > 0 folds each of its streams' rows into that stream's
 * 64-byte record on the device, with two launches of k_meter on the pass's stream: one over the block the pass was handed, ahead of the
 * model's launch, and one over the block it returns, behind the last stage.
 * Input and output:
 *  - "Input" is the stream's row of the block the pass was handed, before PREGAIN and everything else, the noise gate included
 *    ("Noise gate" below): a gated stream's in_peak and in_energy describe the ungated block.
 *  - "Output" is its row of the block the pass returns: behind the master ramp and, where the pool has an IR history, behind the IR stage
 *    and its fade.
 *  - A stream with `enabled` = 0 is metered like any other; its output is its input.
 *  - Under a rate adapter the blocks, and so the frames counted, are the pool's: the pool-rate blocks between the adapter's two stages.
 * Which passes are metered:
 *  - A pass is metered when metering is on at the moment it is issued: the blocking path, aidax_pool_submit* / collect (the blocks in
 *    flight too), aidax_pool_process_device on the pool's or a caller's stream, passes under aidax_rate_*.
 *  - A pass of n_frames == 0 touches nothing, and a pass issued while metering is off is not counted.
 *  - The records survive switching off and on, aidax_pool_reset_stream, model and IR swaps and assignments; only `clear` zeroes them.
 *  - `frames` and `passes` are counted by the output side: a pass that fails on its way may leave its input side counted.
 * Arithmetic:
 *  - Peaks, counts and `frames` are exact.
 *  - Each square is formed in fp64 from the fp32 sample (exact: 48 significant bits) and the squares are summed in fp64 in an unspecified
 *    order. All terms are non-negative, so an energy is within frames x 2^-52 relative of the exact sum.
 *  - A sample that is NaN or +-Inf is counted as non-finite and enters neither the peak nor the energy of its side.
 * aidax_pool_set_metering  the FIRST call with on != 0 is a SET-UP side call, like aidax_pool_set_ir_capacity: it allocates n_streams
 *                          zeroed records on the device and the pinned staging of the read, and may wait. Every later call is an AUDIO
 *                          side host record, between passes: no allocation, no free, no wait. A call with on == 0 before any with
 *                          on != 0 changes nothing. AIDAX_ERR_ARG for a null pool.
 * aidax_pool_metering      1 while metering is on, else 0 (0 for a null pool).
 * aidax_pool_read_meters   AUDIO side, and it waits, like aidax_pool_export_stream_dsp: the copy of `count` records from stream `first`
 *                          enters the pool's own stream behind every pass issued so far, on whatever stream; with clear != 0 exactly those
 *                          records are zeroed behind the copy, stream-ordered, so no sample between copy and clear is lost; then the
 *                          call waits for that stream only. AIDAX_ERR_ARG for a null argument, count == 0 or first + count > n_streams
 *                          (nothing is changed), AIDAX_ERR_STATE when metering was never enabled.
 * A stream whose biquad memories went non-finite (one NaN or Inf in its input is enough) stays that way until aidax_pool_reset_stream,
 * as an instance of the reference does. Where the model lets the NaN through to the output (in_skip = 1, for one) its out_nonfinite
 * grows from pass to pass while its in_nonfinite does not; the recurrent kernels clamp their tanh arguments in a way that turns a NaN
 * into a saturated finite value, so without such a path the stuck stream's output is finite and only in_nonfinite tells. A host
 * resets a stream on either count ("Stream meters"). Hub seats are not metered (a hub parks seats as disabled raw copies of stale rows: aidax_hub never switches its pool's meters on). */
typedef struct {
    uint64_t frames;           /* frames metered since the last clear                                 */
    uint64_t passes;           /* passes of n_frames > 0 metered since the last clear                 */
    uint64_t in_nonfinite;     /* input samples that are NaN or +-Inf                                 */
    uint64_t out_nonfinite;    /* output samples that are NaN or +-Inf                                */
    uint64_t out_over;         /* finite output samples with |x| > 1.0f                               */
    double   in_energy;        /* sum of x*x over the finite input samples, in fp64                   */
    double   out_energy;       /* ... over the finite output samples                                  */
    float    in_peak;          /* max |x| over the finite input samples, 0 if none                    */
    float    out_peak;         /* ... output samples                                                  */
} aidax_stream_meter;          /* 64 bytes, no padding */
AIDAX_API int  aidax_pool_set_metering(aidax_pool* p, int on);
AIDAX_API int  aidax_pool_metering(const aidax_pool* p);
AIDAX_API int  aidax_pool_read_meters(aidax_pool* p, uint32_t first, uint32_t count, aidax_stream_meter* out, int clear);

/* Noise gate: a per-stream gate AHEAD of the amp model, computed where the blocks are (k_gate, aidax_gate.hip). Opt-in: a pool that never
 * enables one allocates and launches exactly what it did before these calls existed, bit for bit, and so does every pass issued while no
 * stream's gate is on. While at least one stream's gate is on, every pass of n_frames > 0 issues one launch of k_gate on the pass's stream,
 * ahead of the model's launch: it reads the block the pass was handed and writes the gated block into a side block of the pool's
 * (n_streams x max_frames floats), which the model's launch takes as its input. The caller's input block is never written, and a pass
 * may work in place as before.
 * The rule, per stream and frame by frame, with P = 2^24 and the stream's record (aidax_gate_rec) and state (aidax_gate_state: c =
 * hold_left, q = atten; all zero is "unity gain, hold expired"):
 *     a = |x|                                          (a NaN compares false everywhere: a quiet frame)
 *     if      a >= t_open:             c = hold
 *     else if a >= t_close and c > 0:  c = hold        (hysteresis: the close level only keeps an open gate open)
 *     else if c > 0:                   c = c - 1
 *     if c > 0: q = max(q - up, 0)   else   q = min(q + down, P)
 *     if q == 0: y = x                                 (the input's bits, NaN payloads included)
 *     else:      w = (float)(P - q) * 2^-24            (exact)
 *                g = floor + span * w                  (two fp32 operations, each rounded, no fma)
 *                y = x * g
 * Before use c is clipped to the record's `hold` (a parameter change while the stream plays). Everything stateful is an integer, so the
 * kernel's parallel evaluation matches this sequential statement bit for bit; there is no look-ahead and no latency, and the state
 * carries across passes: the output does not depend on how the host cuts the stream into blocks.
 * Which rows are gated:
 *  - A pass plays under the gate records in force when it was issued (they reach the device from a ring of snapshots, like the control
 *    records): the blocking path, aidax_pool_submit* / collect (the blocks in flight too), aidax_pool_process_device on the pool's or a
 *    caller's stream, passes under aidax_rate_* (the gate then sees the pool-rate block between the adapter's two stages).
 *  - A stream whose gate is off, and a stream with `enabled` = 0, get their row as it was handed in, bit for bit, and their state does not
 *    move: a disabled stream's output is its input, and that is the UNGATED input.
 *  - The stream meters' "input" stays the block the pass was handed, before the gate.
 *  - Turning a stream's gate from off to on zeroes its state, and so does aidax_pool_reset_stream, stream-ordered behind the passes issued
 *    so far: a gate switched on in mid-signal starts at unity gain and closes along the release ramp, it never steps. A parameter change
 *    while on keeps the state.
 * aidax_gate_design        pure, host only, any thread: the record of `params` at `samplerate`, in fp64: t_open / t_close =
 *                          (float)pow(10, dB / 20); floor likewise, and exactly 0 for floor_db <= -120; span = (float)(1.0 - (double)floor);
 *                          frames = min(2^24, max(1, llround(ms * samplerate / 1000))) for hold, attack and release; up = ceil(P /
 *                          attack frames), down = ceil(P / release frames); on = 1. AIDAX_ERR_ARG (the reason in aidax_last_error()) for a
 *                          null pointer, a non-finite field, open_db or close_db outside [-120, 0], close_db > open_db, floor_db > 0, a
 *                          time outside [0, 10000] ms, a samplerate that is not positive.
 * aidax_pool_set_gate      `stream` (AIDAX_ALL_STREAMS: every stream) is gated with `params`, designed at aidax_pool_samplerate (under a
 *                          rate adapter: the model's rate), from the next pass on; params == NULL switches the gate off. The FIRST call
 *                          with params != NULL is a SET-UP side call, like the first aidax_pool_set_metering(.., 1): it allocates the
 *                          records, the states, the side block and the snapshots, and may wait. Every later call is an AUDIO side host
 *                          record, between passes (plus, for streams that go from off to on, an asynchronous clear of their states on the
 *                          pool's own stream): no allocation, no free, no wait. A refused call changes nothing. AIDAX_ERR_ARG for a null
 *                          pool, a stream out of range and whatever aidax_gate_design refuses.
 * aidax_pool_stream_gate   the stream's host record: its parameters as last set (zeros if never) and whether its gate is on.
 * aidax_pool_read_gate     AUDIO side, and it waits, like aidax_pool_read_meters: the states of `count` streams from `first`, behind every
 *                          pass issued so far. AIDAX_ERR_ARG for a null argument, count == 0 or first + count > n_streams,
 *                          AIDAX_ERR_STATE when no gate was ever enabled.
 * Not covered: hub seats (aidax_hub never enables a gate on its pool) and so the LV2 shell (the reference's TTL has no ports for it), a
 * side-chain or look-ahead gate, a gate behind the model. */
typedef struct { float open_db, close_db, floor_db, attack_ms, hold_ms, release_ms; } aidax_gate_params;
typedef struct { float t_open, t_close, floor, span; uint32_t hold, up, down, on; } aidax_gate_rec;   /* 32 bytes */
typedef struct { uint32_t hold_left, atten; } aidax_gate_state;                                        /* c, q */
AIDAX_API int  aidax_gate_design(const aidax_gate_params* params, double samplerate, aidax_gate_rec* out);
AIDAX_API int  aidax_pool_set_gate(aidax_pool* p, int32_t stream, const aidax_gate_params* params);
AIDAX_API int  aidax_pool_stream_gate(const aidax_pool* p, uint32_t stream, aidax_gate_params* out, int* on);
AIDAX_API int  aidax_pool_read_gate(aidax_pool* p, uint32_t first, uint32_t count, aidax_gate_state* out);

/* Stream tuners: a monophonic pitch tracker per stream, computed where the blocks are (k_tune, aidax_tune.hip): the McLeod pitch method,
 * a normalised autocorrelation over a window of W frames, with the autocorrelation on the matrix cores. Opt-in: a pool that never calls
 * aidax_pool_set_tuning, or has the stage off, allocates and launches exactly what it did before these calls existed, bit for bit, and
 * the tuners only read the block a pass was handed: a tuned pool's audio is bit-identical to an untuned pool's.
 * While the stage is on and at least one stream's tuner is on, every pass of n_frames > 0 issues one launch of k_tune on the pass's
 * stream, ahead of the model's launch (next to the meters' input side: the pass may work in place). It reads rows < n_active of the block
 * the pass was HANDED — the DI signal: ungated, whatever the stream's `enabled` control says — appends each tuned stream's row to that
 * stream's history ring, and analyses the streams that cross a hop boundary.
 * The rule, normative (tests/tunehelp.py restates it in numpy). A stream's tuner has a frame count `pos`: the frames of the blocks the
 * stream was handed since its tuner went on or was restarted. With the design's window W, hop H, lags tmin .. tmax, threshold k:
 *  1. A pass that takes pos from p0 to p1 analyses the stream if and only if b = floor(p1 / H) * H > p0 and b >= W. The window x[0 .. W)
 *     is the W frames that end at frame b (exclusive), oldest first: not "the last W frames of the block". A stream's readings do not
 *     depend on how the host cuts its blocks; a pass that crosses several boundaries analyses the last one only.
 *  2. r[t] = sum_{j = 0}^{W - 1 - t} x[j] x[j + t] for t = 0 .. tmax + 1 (zeros outside the window). Computed as bf16 term products
 *     accumulated in fp32 (both operands split exactly into three bf16 terms, six of the nine products kept, the partial sums of the
 *     four waves added in a fixed order): within 2^-23 sum |x[j] x[j + t]| plus the accumulation's rounding of the exact sum, and EXACT
 *     where every product and partial sum is an fp32 number (small integers times a power of two).
 *  3. With c the prefix sums of x^2 in fp64 (c[0] = 0, summation order unspecified): m[t] = c[W - t] + (c[W] - c[t]).
 *  4. The NSDF: n[t] = (float)((2.0 * (double)r[t]) / m[t]), or 0.0f where m[t] <= 0.
 *  5. Key maxima, over the lags 1 .. tmax + 1 (lag tmax + 2 counts as not positive). Skip the lobe around lag 0: lags 1, 2, .. while
 *     n > 0. From there on every maximal run of lags with n > 0 is a lobe; its candidates are the lags t with tmin <= t <= tmax,
 *     n[t] >= n[t - 1] and n[t] > n[t + 1]; its key maximum is the candidate of largest n, the earliest on a tie; a lobe without a
 *     candidate has none. (A NaN compares false: not positive, no candidate.)
 *  6. With nmax the largest key maximum, the chosen lag q is the first key maximum with n[q] >= k * nmax (fp32, one rounded product).
 *  7. In fp64 from the fp32 values a = n[q - 1], b = n[q], c = n[q + 1], every operation rounded on its own: den = (a - 2 b) + c;
 *     d = den < 0 ? (0.5 (a - c)) / den : 0; period = q + d; clarity = b - (0.25 (a - c)) d; hz = samplerate / period. Each of the
 *     three is rounded once to fp32.
 *  8. level = (float)sqrt(c[W] / W). The reading is UNVOICED when there is no key maximum (clarity is then 0), when clarity <
 *     clarity_min or when level < the level floor: hz = 0, period = 0, lag = 0; clarity and level are still reported.
 * The reading of the last analysis stays until the next one; `analyses` counts them since the restart, `frame` is the last one's b.
 * A row of silence or of NaN gives an unvoiced reading (level 0, or NaN) and touches nothing but the stream's own tuner.
 * aidax_tuner_design       pure, host only, any thread: the record of `params` at `samplerate`: tmin = floor(samplerate / f_max),
 *                          tmax = ceil(samplerate / f_min), level_min = (float)pow(10, level_min_db / 20) (0 for <= -200 dB).
 *                          AIDAX_ERR_ARG (the reason in aidax_last_error()) for a null pointer, a window other than 1024, 2048 or 4096,
 *                          a hop that is no multiple of 16 or outside 64 .. 65536, a non-finite field, f_min or f_max not positive,
 *                          f_min > f_max, tmin < 2, tmax > window / 2 - 1, a threshold outside (0, 1], a clarity_min outside [0, 1],
 *                          level_min_db > 0, a samplerate that is not positive.
 * aidax_tuner_params_default   window 2048, hop 1024, 70 .. 1400 Hz, threshold 0.93, clarity_min 0.5, level_min_db -60.
 * aidax_tuner_note         pure: the nearest equal-tempered MIDI note of `hz` for A4 = a4_hz (note 69) and the deviation in cents,
 *                          n = 69 + 12 log2(hz / a4_hz) in fp64, midi_note = the integer nearest n, cents = (float)(100 (n - midi_note)).
 *                          AIDAX_ERR_ARG for a null pointer or a frequency that is not positive and finite.
 * aidax_pool_set_tuning    the FIRST call with params != NULL is a SET-UP side call, like the first aidax_pool_set_metering(.., 1): it
 *                          fixes the design at aidax_pool_samplerate for the pool's life and allocates, per stream, a history ring (R
 *                          floats, R the power of two >= window + max_frames), the frame count, the reading, the NSDF row (tmax + 2
 *                          floats) and the snapshots and pinned staging; it switches the stage on, every stream's tuner off, and may
 *                          wait. A later call with params != NULL must name the same design (AIDAX_ERR_STATE otherwise) and switches
 *                          the stage on; params == NULL switches it off (the tuners' counts do not move while it is off). Both are
 *                          AUDIO side host records. AIDAX_ERR_ARG for a null pool and whatever aidax_tuner_design refuses.
 * aidax_pool_tuning        the design (zeros if never set); returns 1 while the stage is on, else 0.
 * aidax_pool_set_tuner     AUDIO side host record: the tuner of `stream` (AIDAX_ALL_STREAMS: every stream) on or off, from the next
 *                          pass on. Off -> on restarts it: pos = 0, an empty history, reading and NSDF row zeroed, on the pool's own
 *                          stream behind the passes issued so far; aidax_pool_reset_stream does the same. A stream whose tuner is
 *                          off keeps the reading it has (zeros if it was never on). AIDAX_ERR_STATE before aidax_pool_set_tuning.
 * aidax_pool_stream_tuner  whether the stream's tuner is on, and its frame count as the host mirrors it.
 * aidax_pool_read_tuners   AUDIO side, and it waits, like aidax_pool_read_meters: the readings of `count` streams from `first`, behind
 *                          every pass issued so far. AIDAX_ERR_ARG for a null argument, count == 0 or first + count > n_streams,
 *                          AIDAX_ERR_STATE before aidax_pool_set_tuning.
 * aidax_pool_read_tuner_curve  the same for the NSDF row of the stream's last analysis, lags 0 .. count - 1, count <= tmax + 2: what
 *                          a tuner display draws.
 * Not covered: hub seats (aidax_hub never enables the stage on its pool) and so the LV2 shell, polyphonic pitch, a tuner behind the
 * model, a window or range per stream. */
typedef struct { uint32_t window, hop; float f_min, f_max, threshold, clarity_min, level_min_db; } aidax_tuner_params;
typedef struct {
    uint32_t window, hop, tmin, tmax;      /* W, H, the lag range                                             */
    float    threshold, clarity_min;       /* k, the clarity floor                                            */
    float    level_min, reserved;          /* the level floor, linear                                         */
    double   samplerate;
} aidax_tuner_rec;                         /* 40 bytes */
typedef struct {
    uint64_t frame;            /* b of the last analysis: the window is frames b - W .. b - 1 of the stream's count */
    uint32_t analyses;         /* analyses since the restart                                          */
    uint32_t lag;              /* the chosen lag q, 0: unvoiced                                       */
    float    hz, period;       /* samplerate / period; q + the parabola's offset, in frames; 0: unvoiced */
    float    clarity, level;   /* the interpolated NSDF peak; the window's RMS                        */
} aidax_tuner_reading;         /* 32 bytes, no padding */
AIDAX_API void aidax_tuner_params_default(aidax_tuner_params* params);
AIDAX_API int  aidax_tuner_design(double samplerate, const aidax_tuner_params* params, aidax_tuner_rec* out);
AIDAX_API int  aidax_tuner_note(double hz, double a4_hz, int32_t* midi_note, float* cents);
AIDAX_API int  aidax_pool_set_tuning(aidax_pool* p, const aidax_tuner_params* params);
AIDAX_API int  aidax_pool_tuning(const aidax_pool* p, aidax_tuner_rec* out);
AIDAX_API int  aidax_pool_set_tuner(aidax_pool* p, int32_t stream, int on);
AIDAX_API int  aidax_pool_stream_tuner(const aidax_pool* p, uint32_t stream, int* on, uint64_t* pos);
AIDAX_API int  aidax_pool_read_tuners(aidax_pool* p, uint32_t first, uint32_t count, aidax_tuner_reading* out);
AIDAX_API int  aidax_pool_read_tuner_curve(aidax_pool* p, uint32_t stream, float* out, uint32_t count);

/* Mix buses: the streams of a pool summed into output buses where the blocks are (k_mix, aidax_mix.hip): two amps of one player, a
 * stereo pair from two cabinets, monitor mixes, the rooms of a service. Opt-in: a pool that never calls aidax_pool_set_buses, or has
 * its buses off, allocates and launches exactly what it did before these calls existed, bit for bit, and the buses only read the
 * stream block: a pool's audio does not depend on them.
 * Buses, sends and the bus block:
 *  - A pool has B buses (aidax_pool_set_buses) and every stream AIDAX_SENDS = 4 sends. A send is (bus, gain); bus is 0 .. B - 1 or
 *    AIDAX_BUS_NONE, the default.
 *  - While the buses are on, every pass of n_frames > 0 ends with one launch of k_mix on the pass's stream, behind the last stage (the
 *    IR stage, the meters): after it the pool's BUS BLOCK, [B][n_frames] floats, rows dense at that pass's n_frames like the stream
 *    block's, holds the mix of the stream block that pass returned — exactly what the caller gets for each stream, whatever produced
 *    it: a disabled stream's row is its raw input, and that is what is summed. A pass of 0 frames touches nothing.
 *  - There is ONE bus block per pool: it is that of the last pass issued, on every path (the blocking calls, aidax_pool_submit* /
 *    collect, aidax_pool_process_device on the pool's or a caller's stream, passes under aidax_rate_*, whose blocks are the pool-rate
 *    ones). A host that keeps blocks in flight reads the buses of the last one it submitted; bus blocks per block in flight do not exist.
 * The sum, normative (tests/mixhelp.py restates it in numpy; the kernel agrees with it bit for bit):
 *  - The entries of bus b are the sends on b in ascending (stream, send index) order. A pass over the first n_active streams only (the
 *    hub's prefix pass) leaves the entries of the other streams out, and their ramps do not move.
 *  - Frame t of entry e contributes the term (float)(g_e[t] * y[stream_e][t]), one fp32 multiplication. A term whose gain is exactly 0
 *    is left out whatever y holds: a muted send of a stream that plays NaN or Inf does not poison its bus.
 *  - The entries are cut into groups of 32 consecutive ones by position in the bus's list. A group sum starts at +0.0f and adds its
 *    terms in order; the bus sample starts at +0.0f and adds the group sums in group order. Every addition is one fp32 operation,
 *    rounded to nearest; there is no fma anywhere. A bus of at most 32 entries is therefore the plain sequential sum, and a bus without
 *    entries is +0.0f.
 *  - A bus with one send at gain 1 carries the stream's bits, except that -0.0 becomes +0.0 (0 + -0 = +0) and a NaN's payload is the
 *    hardware's.
 * Gain ramps, by the IR blend's convention ("IR blend" above):
 *  - g_now is the fp32 gain of the send's last issued frame on its bus: 0 for a send that never played, and for one that has just been
 *    moved to another bus.
 *  - aidax_pool_set_send(.., bus, gain, R): if `bus` is the bus the send played on in the last pass issued, a ramp from g0 = g_now to
 *    g1 = gain whose frame k = 0 is the stream's next issued frame. If it is another bus, the send moves at the block boundary and ramps
 *    from g0 = 0: a new send fades in. AIDAX_BUS_NONE removes the send at the block boundary, and its g_now is 0 from then on: to
 *    remove a send without a click, ramp it to 0 first. Every call is judged against the state behind the last pass issued: of
 *    several calls between two passes the last one wins, from the same g0.
 *  - Ramp frame k has, in fp64 with every operation rounded on its own,
 *        k + 1 <  R:  g = (float)((double)g0 + ((double)g1 - (double)g0) * (double)(k + 1) / (double)R)
 *        k + 1 >= R:  g = g1                                                                    (R = 0: a jump at the block boundary)
 *    and k counts the stream's issued frames, not passes: a ramp does not depend on how the host cuts the stream into blocks.
 *  - Ramp positions are host integers, advanced by n_frames for the streams of every pass issued while the buses are on (not by a pass
 *    of 0 frames, not while they are off). aidax_pool_reset_stream keeps the sends and a running ramp goes on.
 *  - Each pass is mixed with the sends in force when it was issued. The plan (which entries each bus has, and their ramps) reaches the
 *    device from a ring of snapshots ahead of the pass that follows an aidax_pool_set_send; a pass without a changed send uploads
 *    nothing, running ramps or not.
 * aidax_pool_set_buses      SET-UP side. The first call with n_buses > 0 (1 .. AIDAX_MAX_BUSES) allocates everything the feature
 *                           ever needs — the bus block [n_buses][max_frames], zeroed, the plan for n_streams x AIDAX_SENDS entries, its
 *                           snapshots, the pinned staging of the reads — switches the buses on, and may wait. The count is fixed from
 *                           then on: a later call with the same count switches them on again, one with another non-zero count is
 *                           AIDAX_ERR_STATE. 0 switches them off and keeps sends, ramps and allocation (before any other call: nothing
 *                           to do); while off, no pass is mixed, the bus block stays as it was and ramps do not advance. Later calls are
 *                           host records of the audio side. AIDAX_ERR_ARG for a null pool or a count beyond AIDAX_MAX_BUSES.
 * aidax_pool_buses          the bus count (0 until it is set, and for a null pool), on or off.
 * aidax_pool_set_send       AUDIO thread, between passes: send `send` of `stream` (AIDAX_ALL_STREAMS: of every stream, each from its own
 *                           g_now) as above. Host records only: no allocation, no free, no wait. AIDAX_ERR_ARG for a null pool, a
 *                           stream, send or bus out of range, a gain that is not finite or beyond AIDAX_MIX_MAX_GAIN = 16 in magnitude,
 *                           ramp_frames > 2^24 (a refused call changes nothing); AIDAX_ERR_STATE before aidax_pool_set_buses.
 * aidax_pool_stream_send    the state behind the last pass issued, as the next aidax_pool_set_send would find it (any pointer may be
 *                           NULL): the send's bus, g_now, the ramp's target, and the frames still to be issued until g_now is the
 *                           target (0: the ramp has ended; a jump has 1 until a frame is issued). Before aidax_pool_set_buses:
 *                           AIDAX_BUS_NONE, 0, 0, 0.
 * aidax_mix_gain            pure, host only, any thread, like aidax_gate_design: the gain of ramp frame k by the formula above.
 *                           AIDAX_ERR_ARG for a null pointer and for what aidax_pool_set_send refuses of g0, g1 and ramp_frames.
 * aidax_pool_read_buses     AUDIO side, and it waits, like aidax_pool_read_meters: rows first .. first + count - 1 of the last mixed pass's
 *                           bus block, count x n_frames floats dense at that pass's n_frames (returned in *n_frames, which may be NULL;
 *                           0 and nothing copied before the first mixed pass), behind every pass issued so far on whatever stream.
 *                           AIDAX_ERR_ARG for a null pool or buffer, count == 0, first + count > the bus count or cap_floats too small
 *                           (nothing is changed), AIDAX_ERR_STATE before aidax_pool_set_buses.
 * aidax_pool_buses_device   the device address of the bus block, for hosts of aidax_pool_process_device: valid from
 *                           aidax_pool_set_buses until the pool's end, written on the stream each pass ran on (a reader on another
 *                           stream orders itself behind that pass, as it does for the stream block).
 * aidax_pool_process_buses  the blocking host call that downloads only the buses: uploads `in` through the pool's staging as
 *                           aidax_pool_process does for blocks beyond its in-place path, runs the pass into the pool's own device
 *                           block, downloads [B][n_frames] into bus_out through pinned staging and waits for the pool's stream (no
 *                           in-place host memory, no completion word). n_frames == 0 is the pre-run and writes nothing.
 *                           AIDAX_ERR_STATE while the buses are off or were never set.
 * Not covered: hub seats (aidax_hub never sets buses on its pool) and so the LV2 shell, a bus block per block in
 * flight, a pan law (the host sets two gains), more than four sends per stream. */
#define AIDAX_SENDS 4
#define AIDAX_BUS_NONE (-1)
#define AIDAX_MAX_BUSES 4096
#define AIDAX_MIX_MAX_GAIN 16.0f
AIDAX_API int      aidax_pool_set_buses(aidax_pool* p, uint32_t n_buses);
AIDAX_API uint32_t aidax_pool_buses(const aidax_pool* p);
AIDAX_API int      aidax_pool_set_send(aidax_pool* p, int32_t stream, uint32_t send, int32_t bus, float gain, uint32_t ramp_frames);
AIDAX_API int      aidax_pool_stream_send(const aidax_pool* p, uint32_t stream, uint32_t send, int32_t* bus, float* gain_now, float* gain_target, uint32_t* frames_left);
AIDAX_API int      aidax_mix_gain(float g0, float g1, uint32_t ramp_frames, uint32_t k, float* gain);
AIDAX_API int      aidax_pool_read_buses(aidax_pool* p, uint32_t first, uint32_t count, float* out, size_t cap_floats, uint32_t* n_frames);
AIDAX_API int      aidax_pool_buses_device(aidax_pool* p, float** d_ptr);
AIDAX_API int      aidax_pool_process_buses(aidax_pool* p, const float* in, float* bus_out, uint32_t n_frames);

/* Bus limiters: the master section of the mix buses — a look-ahead brick-wall limiter and a meter on every bus, computed where the bus
 * block is (k_bus_limit, aidax_bus_limit.hip). Opt-in: a pool that never calls aidax_pool_set_bus_limiting, or has the stage off,
 * allocates and launches exactly what it did before these calls existed, bit for bit. While the stage and the buses are on, k_mix of
 * every pass of n_frames > 0 writes a raw side block and one launch of k_bus_limit, behind it on the pass's stream, writes the pool's
 * bus block: aidax_pool_read_buses, aidax_pool_buses_device and aidax_pool_process_buses then return the LIMITED block.
 * The rule, normative (tests/limithelp.py restates it in numpy; the kernel agrees with it bit for bit). Each bus has a record
 * (aidax_bus_limit_rec): C the ceiling (linear, fp32, > 0), L the look-ahead in frames (1 .. AIDAX_BUS_LOOKAHEAD_MAX), H the hold in
 * frames (0 .. AIDAX_BUS_HOLD_MAX). U = 2^22, W = L + 1 + H. x[j] is the SANITISED raw bus sample of absolute frame j: what k_mix
 * produced, with NaN and +-Inf replaced by +0.0f. Frames are counted from the stage's first enabling, and x[j] = 0 for j < 0.
 *     q[j] = U                                               if |x[j]| <= C
 *          = floor(((double)C / (double)|x[j]|) * 2^22)      otherwise (one rounded fp64 division, an exact scaling, floor)
 *     h[m] = min(q[m - W + 1 .. m])                          (a sliding minimum over W frames)
 *     s[n] = h[n - L + 1] + .. + h[n]                        (an integer, at most L U <= 2^31: any order of summation)
 *     g[n] = (float)((double)s[n] / (double)(L U))           (one fp64 division, one rounding to fp32)
 *     out[n] = x[n - L] * g[n]                               (one rounded fp32 multiplication)
 * The bus is delayed by exactly L frames: the latency a host reports for it (aidax_pool_bus_limiter). The gain falls linearly over the L
 * frames ahead of a peak, is held for H frames and rises linearly over L frames. Consequences:
 *  - The ceiling holds without a clamp: every output is finite and |out[n]| <= C, since g[n] <= q[n - L] / U, that bound is exactly
 *    representable and rounding is monotone.
 *  - The output does not depend on how the host cuts the frames into blocks.
 *  - A bus that never exceeds C comes out with its own bits, L frames late, and every g is exactly 1.
 * A pass is evaluated with the record in force when it was issued, over the whole sample history, frames mixed under an older record
 * included: a change of record, or of a limiter's on / off, takes effect at the block boundary and is NOT click-free, and a change of L
 * also changes the delay. A bus whose limiter is OFF (the default) returns the raw k_mix bits undelayed, NaN included; its history is
 * still kept. The history moves only with limited passes: not with a pass of 0 frames, not while the buses or the stage are off.
 * The bus meter (aidax_bus_meter), folded by the same launch: every field is a maximum, a minimum or an integer count.
 *  - frames, passes: of the limited passes since the last clear. in_nonfinite: raw samples that are NaN or +-Inf.
 *  - in_peak: max |x| over the sanitised samples. out_peak: max |out|.
 *  - limited: frames with s[n] < L U (the integer test: at L = 512, s = L U - 1 rounds to g == 1.0f). min_gain: min g, 1.0 after a clear.
 *  - A bus whose limiter is off folds its in_peak into out_peak as well and leaves limited and min_gain alone.
 * aidax_bus_limit_design      pure, host only, any thread: the record of `params` at `samplerate`, in fp64: ceiling = (float)pow(10,
 *                             dB / 20) for -60 <= ceiling_db <= 12; lookahead and hold = ms * samplerate / 1000 rounded to nearest; on
 *                             = 1. AIDAX_ERR_ARG for a null pointer, a non-finite field, a ceiling out of range, a negative time, a
 *                             look-ahead below 1 or beyond 512 frames, a hold beyond 4096 frames, a samplerate that is not positive.
 * aidax_pool_set_bus_limiting SET-UP side. The first call with on != 0 allocates everything the feature ever needs — the raw side block,
 *                             a ring of sanitised samples per bus (zeroed), the records (every limiter off), the meter records
 *                             (cleared), their snapshots and the pinned staging of the read — all or nothing, fixes the capacities
 *                             (max_lookahead_frames 1 .. 512, max_hold_frames 0 .. 4096: no record beyond them is accepted), switches
 *                             the stage on, and may wait. Later calls only flip a host record of the audio side: on != 0 with another
 *                             capacity is AIDAX_ERR_STATE, on == 0 ignores the capacities. AIDAX_ERR_STATE before aidax_pool_set_buses,
 *                             AIDAX_ERR_ARG for a null pool or a capacity out of range.
 * aidax_pool_bus_limiting     1 while the stage is on, else 0 (0 for a null pool).
 * aidax_pool_set_bus_limiter  AUDIO thread, between passes: `bus` (AIDAX_ALL_BUSES: every bus) is limited with `params`, designed at
 *                             aidax_pool_samplerate, from the next pass on; params == NULL switches its limiter off. Host records only
 *                             (they reach the device from a ring of snapshots ahead of the next limited pass): no allocation, no free, no
 *                             wait. AIDAX_ERR_ARG for a null pool, a bus out of range, whatever aidax_bus_limit_design refuses and a
 *                             record beyond the capacities (a refused call changes nothing); AIDAX_ERR_STATE before the stage's first
 *                             enabling.
 * aidax_pool_bus_limiter      the bus's host record (any pointer may be NULL): its parameters as last set (zeros while off), whether
 *                             its limiter is on, and its latency in frames (L while on, else 0).
 * aidax_pool_read_bus_meters  AUDIO side, and it waits and clears like aidax_pool_read_meters (a cleared record has min_gain = 1.0).
 *                             AIDAX_ERR_ARG for a null argument, count == 0 or first + count > the bus count, AIDAX_ERR_STATE before the
 *                             stage's first enabling.
 * Not covered: hub seats and so the LV2 shell, resetting a bus's history, click-free parameter changes, a release longer than the
 * look-ahead, linked (stereo) buses. */
#define AIDAX_ALL_BUSES (-1)
#define AIDAX_BUS_LOOKAHEAD_MAX 512
#define AIDAX_BUS_HOLD_MAX 4096
typedef struct { float ceiling_db, lookahead_ms, hold_ms; } aidax_bus_limit_params;
typedef struct { float ceiling; uint32_t lookahead, hold, on; } aidax_bus_limit_rec;   /* 16 bytes */
typedef struct {
    uint64_t frames;           /* frames limited since the last clear                                 */
    uint64_t passes;           /* limited passes since the last clear                                 */
    uint64_t in_nonfinite;     /* raw bus samples that are NaN or +-Inf                               */
    uint64_t limited;          /* frames with s[n] < L U                                              */
    float    in_peak;          /* max |x| over the sanitised samples                                  */
    float    out_peak;         /* max |out|                                                           */
    float    min_gain;         /* min g, 1.0 after a clear                                            */
    float    reserved;
} aidax_bus_meter;             /* 48 bytes, no padding */
AIDAX_API int      aidax_bus_limit_design(const aidax_bus_limit_params* params, double samplerate, aidax_bus_limit_rec* out);
AIDAX_API int      aidax_pool_set_bus_limiting(aidax_pool* p, int on, uint32_t max_lookahead_frames, uint32_t max_hold_frames);
AIDAX_API int      aidax_pool_bus_limiting(const aidax_pool* p);
AIDAX_API int      aidax_pool_set_bus_limiter(aidax_pool* p, int32_t bus, const aidax_bus_limit_params* params);
AIDAX_API int      aidax_pool_bus_limiter(const aidax_pool* p, uint32_t bus, aidax_bus_limit_params* out, int* on, uint32_t* latency_frames);
AIDAX_API int      aidax_pool_read_bus_meters(aidax_pool* p, uint32_t first, uint32_t count, aidax_bus_meter* out, int clear);

/* Bus reverbs: a room on every mix bus — a feedback delay network of eight delay lines with an orthogonal feedback matrix, computed
 * where the bus block is (k_bus_reverb, aidax_bus_reverb.hip), behind k_mix and ahead of k_bus_limit. Opt-in: a pool that never calls
 * aidax_pool_set_bus_reverbs, or has the stage off, allocates and launches exactly what it did before these calls existed, bit for bit.
 * While the stage and the buses are on, one launch of k_bus_reverb behind k_mix of every pass of n_frames > 0 works in place on the
 * block k_mix wrote (the limiters' raw side block while they are on, else the pool's bus block): the limiters and their meters, and
 * aidax_pool_read_buses, aidax_pool_buses_device and aidax_pool_process_buses, then see the REVERBERATED block. A bus whose reverb is
 * OFF (the default) keeps the bits k_mix wrote, NaN included.
 * The rule, normative (tests/reverbhelp.py restates it in numpy; the kernel agrees with it bit for bit). Each bus has a record
 * (aidax_bus_reverb_rec): eight delays m[i] in frames (AIDAX_BUS_REVERB_MIN_DELAY = 64 <= m[i] <= the pool's delay capacity), eight
 * feedback gains gq[i] (fp32, 0 <= gq[i] < 1/sqrt(8)), a damping a (fp32, 0 <= a <= 0.5), wet and dry (fp32, finite, magnitude <= 4),
 * on, and an epoch, a frame position modulo 2^32. x[n] is the SANITISED raw bus sample of absolute frame n: what k_mix produced, with
 * NaN and +-Inf replaced by +0.0f and then clamped to +-2^64. d_i[j] is line i's memory at absolute frame j; it is 0 for every frame
 * before the record's epoch. Every operation below is ONE fp32 operation rounded to nearest; there is no fma anywhere. Per frame n, for
 * i = 0 .. 7:
 *     s_i = d_i[n - m_i]        t_i = d_i[n - m_i - 1]                      (the taps)
 *     f_i = s_i + a * (t_i - s_i)                                           (the damping: a 2-tap FIR of magnitude <= 1 at every frequency;
 *                                                                            deliberately not a one-pole, which would chain the frames)
 *     h   = the unnormalised Hadamard butterfly of f in three stages with strides 1, 2 and 4: in each stage the element whose stride
 *           bit is clear becomes lo + hi and its partner lo - hi (the factor 1/sqrt(8) is inside gq)
 *     d_i[n] = x[n] + gq_i * h_i                                            (the write)
 *     w   = ((s_0 - s_1) + (s_2 - s_3)) + ((s_4 - s_5) + (s_6 - s_7))       (the wet sum)
 *     out[n] = dry * x[n] + wet * w
 * Why the state stays finite: write g_i = sqrt(8) gq_i < 1 and g_max for the largest. The butterfly is sqrt(8) times an orthogonal
 * matrix, so the feedback path of a frame is an orthogonal mix, scaled per line by g_i <= g_max, of FIR outputs no larger than the
 * larger of their two taps: round the loop every component of the signal loses at least the factor g_max at every frequency, and by
 * the small-gain argument the energy the lines hold is bounded by that of the input over 1 - g_max. The input is clamped to 2^64, so
 * the lines stay some sixty binary orders below the fp32 range; each rounding moves a value by at most 2^-24 of itself, which a loop
 * gain of 1 - 1e-5 or less (every designed record: rt60 <= 20 s) absorbs.
 * Independence: frame n reads nothing younger than n - min m_i, so the frames n .. n + K - 1 are independent of one another for
 * K <= min m_i. The rule depends neither on how a pass is cut into chunks nor on how the host cuts the signal into blocks.
 * The memories move only with reverberated passes: not with a pass of 0 frames, not while the buses or the stage are off (frames
 * mixed meanwhile never enter the lines). The epoch is set to the next pass's first frame — the tail is cut, and the change is NOT
 * click-free — when a bus's reverb goes on, when any m[i] changes, and by aidax_pool_reset_bus_reverb. A change of only gq, a, wet or
 * dry keeps the memories and acts at the block boundary.
 * Position wrap: the stage stays right beyond 2^32 issued frames. The device compares positions modulo 2^32, so the host moves an epoch
 * that has fallen 2^30 frames behind forward to the longest admitted delay + 1 behind the position (any epoch older than that gives
 * the same result): one record upload every few hours.
 * aidax_bus_reverb_design     pure, host only, any thread: the record of `params` at `samplerate`, in fp64. rt60_s 0.1 .. 20, size
 *                             0.05 .. 2, damping 0 .. 1, wet and dry finite with magnitude <= 4, variant 0 .. 3. m_i = max(64,
 *                             floor(base[variant][i] * size * samplerate / 48000 + 0.5)) | 1, then + 2 while equal to an earlier
 *                             line's; base is four fixed tables of eight lengths between 1400 and 3000 frames (variant 0: 1423, 1637,
 *                             1871, 2087, 2311, 2539, 2767, 2999), and two buses with different variants make a decorrelated stereo
 *                             pair. gq_i = (float)(pow(10, -3 m_i / (rt60_s * samplerate)) / sqrt(8)), a = (float)(damping * 0.5),
 *                             on = 1, epoch = 0 (the pool sets it). AIDAX_ERR_ARG for a null pointer, anything outside the ranges (a NaN
 *                             is), a samplerate that is not positive, a delay beyond AIDAX_BUS_REVERB_MAX_DELAY; `out` is untouched then.
 * aidax_pool_set_bus_reverbs  SET-UP side. The first call with on != 0 allocates everything the feature ever needs — eight ring rows
 *                             per bus (zeroed), the records (every reverb off) and their snapshots — all or nothing, fixes the delay
 *                             capacity (max_delay_frames 64 .. 32768: no record with a longer delay is accepted; a ring row is the
 *                             smallest power of two >= capacity + 1 + max_frames floats), switches the stage on, and may wait. Later
 *                             calls only flip a host record of the audio side: on != 0 with another capacity is AIDAX_ERR_STATE, on
 *                             == 0 ignores it. AIDAX_ERR_STATE before aidax_pool_set_buses, AIDAX_ERR_ARG for a null pool or a capacity
 *                             out of range.
 * aidax_pool_bus_reverbs      1 while the stage is on, else 0 (0 for a null pool).
 * aidax_pool_set_bus_reverb   AUDIO thread, between passes: `bus` (AIDAX_ALL_BUSES: every bus) is reverberated with `params`, designed
 *                             at aidax_pool_samplerate, from the next pass on; params == NULL switches its reverb off. Host records
 *                             only (they reach the device from a ring of snapshots ahead of the next reverberated pass): no allocation,
 *                             no free, no wait. AIDAX_ERR_ARG for a null pool, a bus out of range, whatever aidax_bus_reverb_design
 *                             refuses and a delay beyond the capacity (a refused call changes nothing); AIDAX_ERR_STATE before the
 *                             stage's first enabling.
 * aidax_pool_set_bus_reverb_rec  the same with a record of the caller's own (a host's own tuning); its `on` and `epoch` are ignored.
 *                             AIDAX_ERR_ARG also for a record outside the conditions above; rec == NULL switches the reverb off.
 * aidax_pool_bus_reverb       the bus's host record (any pointer may be NULL): its parameters as last set (zeros while off or set by a
 *                             record), its record (zeros while off), whether its reverb is on, and the reverberated frames issued
 *                             since its epoch (0 while off).
 * aidax_pool_reset_bus_reverb AUDIO thread, between passes: the memories of `bus` (AIDAX_ALL_BUSES: every bus) are cut at the next
 *                             pass's first frame (its epoch is set). Host records only. Errors as aidax_pool_set_bus_reverb's.
 * Not covered: hub seats and so the LV2 shell, click-free changes, a wet-only return to another bus, modulation of the delays, a
 * meter of its own (the limiter's bus meter sees the reverberated block). */
#define AIDAX_BUS_REVERB_LINES 8
#define AIDAX_BUS_REVERB_MIN_DELAY 64
#define AIDAX_BUS_REVERB_MAX_DELAY 32768
typedef struct { float rt60_s, size, damping, wet, dry; uint32_t variant; } aidax_bus_reverb_params;
typedef struct {
    uint32_t m[AIDAX_BUS_REVERB_LINES];    /* the delays in frames                                 */
    float    gq[AIDAX_BUS_REVERB_LINES];   /* the feedback gains, 1/sqrt(8) included               */
    float    a, wet, dry;
    uint32_t on;
    uint32_t epoch;                        /* the pool's: every d_i is 0 before this frame         */
    uint32_t reserved[3];
} aidax_bus_reverb_rec;                    /* 96 bytes, no padding */
AIDAX_API int      aidax_bus_reverb_design(const aidax_bus_reverb_params* params, double samplerate, aidax_bus_reverb_rec* out);
AIDAX_API int      aidax_pool_set_bus_reverbs(aidax_pool* p, int on, uint32_t max_delay_frames);
AIDAX_API int      aidax_pool_bus_reverbs(const aidax_pool* p);
AIDAX_API int      aidax_pool_set_bus_reverb(aidax_pool* p, int32_t bus, const aidax_bus_reverb_params* params);
AIDAX_API int      aidax_pool_set_bus_reverb_rec(aidax_pool* p, int32_t bus, const aidax_bus_reverb_rec* rec);
AIDAX_API int      aidax_pool_bus_reverb(const aidax_pool* p, uint32_t bus, aidax_bus_reverb_params* params, aidax_bus_reverb_rec* rec, int* on, uint64_t* frames_since_epoch);
AIDAX_API int      aidax_pool_reset_bus_reverb(aidax_pool* p, int32_t bus);

/* Stream delays: the player's own time effect — an echo, a slap-back, a chorus, a flanger — per stream, computed where the blocks are
 * (k_delay, aidax_delay.hip): behind the cabinet IR stage and ahead of the meters' output side and the mix buses, which then see the
 * DELAYED block. Opt-in: a pool that never calls aidax_pool_set_delays, or has the stage off or every delay off, allocates and
 * launches exactly what it did before these calls existed, bit for bit. While the stage is on and a delay is on, one launch of k_delay
 * behind every pass of n_frames > 0 works in place on the block the pass returns.
 * The rule, normative (tests/delayhelp.py restates it in numpy, frame by frame; the kernel agrees with it bit for bit). Each stream has
 * a record (aidax_delay_rec) and a state (aidax_delay_state, all zero after a restart). The record: m, the delay in frames
 * (AIDAX_DELAY_MIN = 64 <= m); depth_q16, the modulation depth in frames * 2^16 (at most AIDAX_DELAY_MAX_DEPTH = 4096 frames); lfo_step,
 * the phase increment per frame of a 32-bit phase; fade, the crossfade length in frames (0 .. AIDAX_DELAY_MAX_FADE = 2^20); fb (fp32,
 * |fb| <= 0.98; negative feedback is allowed: a flanger uses it); damp (fp32, 0 .. 0.5); wet and dry (fp32, finite, magnitude <= 4);
 * on. The pool's capacity `cap` bounds m + ceil(depth) <= cap.
 * At the FIRST FRAME OF A PASS, for a stream that plays (below): if m_cur == 0 (a fresh line) m_cur = m, no fade; else if m != m_cur
 * then m_old = m_cur, m_cur = m, fade_len = fade_left = fade. A fade still in progress at that moment is dropped at its target: the
 * second change of time inside a fade is NOT click-free.
 * Then FOR EVERY FRAME, with n = pos its index in the line's own time, x_raw the sample in the block, x the SANITISED sample (NaN and
 * +-Inf replaced by +0.0f, then clamped to +-2^64) and d[k] the line's memory, 0 for k < 0. Every fp32 operation below is ONE operation
 * rounded to nearest; there is no fma anywhere:
 *     u   = (phase >> 8) & 0xffffff;   tri = u < 2^23 ? u : 2^24 - u                              (a triangle, 0 .. 2^23)
 *     off = ((uint64)depth_q16 * tri) >> 23                                                       (Q16 frames, >= 0)
 *     tap(M): D = ((uint64)M << 16) + off;   i = min(D >> 16, cap);   fr = (float)(D & 0xffff) * 2^-16
 *             a = d[n - i], b = d[n - i - 1], c = d[n - i - 2]
 *             p0 = a + fr * (b - a);   p1 = b + fr * (c - b);   tap = p0 + damp * (p1 - p0)
 *     f = tap(m_cur)
 *     if fade_left > 0:   w = (float)((double)(fade_len - fade_left) / (double)fade_len)
 *                         f = tap(m_old) + w * (f - tap(m_old));   fade_left -= 1
 *     d[n]   = x + fb * f
 *     out[n] = dry * x + wet * f
 *     pos += 1;   phase += lfo_step (mod 2^32);   replaced += (x_raw is NaN or +-Inf)
 * (min(.., cap) changes nothing for the record's own delay, whose reach fits the capacity; it bounds the OLD delay of a fade under a
 * record whose depth has grown at the same time.) What follows: a frame reads nothing younger than n - min(m_cur, m_old while fading),
 * so the frames of a chunk of K <= that minimum are independent of one another; every tap is a convex combination, so |fb| <= 0.98
 * bounds the line and every output of a playing stream is finite (below 2^72 under a constant 2^64 input at fb = 0.98, wet = dry = 4);
 * the output does not depend on how the host cuts the stream into blocks; wet = 0 and dry = 1 return the bits of a finite input
 * below 2^64 (a -0.0f may come back as +0.0f).
 * Which streams play: those whose delay is on and whose control record is enabled (not a disabled plugin, not a parked seat). Any
 * other row is left untouched bit for bit and its state does not move. A line restarts — its state is zeroed on the pool's own stream,
 * behind every pass issued so far; its memory needs no clearing — when its delay goes from off to on, when the stage goes from off to
 * on (every line), by aidax_pool_reset_delay and by aidax_pool_reset_stream. A change of fb, damp, wet, dry, depth_q16, lfo_step or fade
 * acts at the next pass's first frame and keeps the line; only m fades.
 * aidax_delay_design        pure, host only, any thread: the record of `params` at `samplerate`, in fp64. m = llround(time_ms *
 *                           samplerate / 1000), 64 .. AIDAX_DELAY_MAX; fb = feedback, |fb| <= 0.98; damp = (float)(damping * 0.5),
 *                           damping 0 .. 1; wet and dry finite with magnitude <= 4; depth_q16 = llround(mod_depth_ms * samplerate /
 *                           1000 * 65536), mod_depth_ms >= 0 and at most 4096 frames; lfo_step = llround(mod_rate_hz / samplerate *
 *                           2^32), 0 <= mod_rate_hz <= 1000 and at most samplerate / 2; fade = llround(fade_ms * samplerate / 1000),
 *                           0 .. 2^20; on = 1. AIDAX_ERR_ARG for a null pointer, anything outside these bounds (a NaN is), a
 *                           samplerate that is not positive; `out` is untouched then.
 * aidax_pool_set_delays     SET-UP side. The first call with on != 0 allocates everything the feature ever needs — a ring row per
 *                           stream (the smallest power of two >= capacity + 3 + max_frames floats), the records (every delay off),
 *                           the states and their snapshots — all or nothing, fixes the capacity (max_delay_frames 64 ..
 *                           AIDAX_DELAY_MAX = 1 << 18), switches the stage on, and may wait. Later calls only flip a host record of
 *                           the audio side (off -> on restarts every line): on != 0 with another capacity is AIDAX_ERR_STATE, on == 0
 *                           ignores it. AIDAX_ERR_ARG for a null pool or a capacity out of range.
 * aidax_pool_delays         1 while the stage is on, else 0 (0 for a null pool).
 * aidax_pool_set_delay      AUDIO thread, between passes: `stream` (AIDAX_ALL_STREAMS: every stream) is delayed with `params`,
 *                           designed at aidax_pool_samplerate, from the next pass on; params == NULL switches its delay off. Host
 *                           records only (they reach the device from a ring of snapshots ahead of the next delayed pass; a restart
 *                           is one memset on the pool's own stream): no allocation, no free, no wait. AIDAX_ERR_ARG for a null
 *                           pool, a stream out of range, whatever aidax_delay_design refuses and a record beyond the capacity (a
 *                           refused call changes nothing); AIDAX_ERR_STATE before the stage's first enabling.
 * aidax_pool_set_delay_rec  the same with a record of the caller's own; its `on` is ignored. AIDAX_ERR_ARG also for a record outside
 *                           the conditions above; rec == NULL switches the delay off.
 * aidax_pool_stream_delay   the stream's host record (any pointer may be NULL): its parameters as last set (zeros while off or set
 *                           by a record), its record (zeros while off), whether its delay is on.
 * aidax_pool_read_delays    AUDIO thread, waits like aidax_pool_read_gate: the states of `count` streams from `first`, behind every
 *                           pass issued so far.
 * aidax_pool_reset_delay    AUDIO thread, between passes: the line of `stream` (AIDAX_ALL_STREAMS: every stream) restarts at the
 *                           next pass's first frame. Errors as aidax_pool_set_delay's.
 * Not covered: hub seats and so the LV2 shell, a fade that survives a second change of time, ping-pong / stereo, tempo sync (the host
 * converts BPM to ms), a line per IR side. */
#define AIDAX_DELAY_MIN 64
#define AIDAX_DELAY_MAX (1 << 18)
#define AIDAX_DELAY_MAX_DEPTH 4096
#define AIDAX_DELAY_MAX_FADE (1 << 20)
typedef struct { float time_ms, feedback, damping, wet, dry, mod_rate_hz, mod_depth_ms, fade_ms; } aidax_delay_params;
typedef struct {
    uint32_t m;                /* the delay in frames                                  */
    uint32_t depth_q16;        /* the modulation depth in frames * 2^16                */
    uint32_t lfo_step;         /* the phase increment per frame                        */
    uint32_t fade;             /* the crossfade length in frames                       */
    float    fb, damp, wet, dry;
    uint32_t on;
    uint32_t reserved[3];
} aidax_delay_rec;             /* 48 bytes, no padding */
typedef struct {
    uint64_t pos;              /* frames the line has taken                            */
    uint32_t m_cur, m_old;     /* the delay in force, the one a fade comes from        */
    uint32_t fade_len, fade_left;
    uint32_t phase;
    uint32_t replaced;         /* NaN and +-Inf samples replaced by 0 (modulo 2^32)    */
} aidax_delay_state;           /* 32 bytes, no padding */
AIDAX_API int      aidax_delay_design(const aidax_delay_params* params, double samplerate, aidax_delay_rec* out);
AIDAX_API int      aidax_pool_set_delays(aidax_pool* p, int on, uint32_t max_delay_frames);
AIDAX_API int      aidax_pool_delays(const aidax_pool* p);
AIDAX_API int      aidax_pool_set_delay(aidax_pool* p, int32_t stream, const aidax_delay_params* params);
AIDAX_API int      aidax_pool_set_delay_rec(aidax_pool* p, int32_t stream, const aidax_delay_rec* rec);
AIDAX_API int      aidax_pool_stream_delay(const aidax_pool* p, uint32_t stream, aidax_delay_params* params, aidax_delay_rec* rec, int* on);
AIDAX_API int      aidax_pool_read_delays(aidax_pool* p, uint32_t first, uint32_t count, aidax_delay_state* out);
AIDAX_API int      aidax_pool_reset_delay(aidax_pool* p, int32_t stream);

/* Threads. A pool is driven by ONE audio-side caller at a time (set_controls, set_loading, activate,
 * reset_stream, commit_model, commit_ir, assign_ir, assign_ir_b, set_ir_mix, assign_model, set_ir_fade, set_metering after its first enabling call, read_meters, set_gate after its first enabling call, read_gate, set_buses after its first enabling call, set_send, read_buses, set_bus_limiting after its first enabling call, set_bus_limiter, read_bus_meters, set_bus_reverbs after its first enabling call, set_bus_reverb, set_bus_reverb_rec, reset_bus_reverb, set_delays after its first enabling call, set_delay, set_delay_rec, reset_delay, read_delays, process*, sync; around a wrapped pool also aidax_rate_process,
 * aidax_rate_process_device, aidax_rate_reset_stream) plus, concurrently, ONE worker-side caller (prepare_model,
 * prepare_model_slot, prepare_ir, prepare_ir_slot, staged_free). set_ir_capacity is a set-up side call, made before the first prepare_ir / prepare_ir_slot and
 * before the two threads start, and so is the first aidax_pool_set_metering with on != 0 (it allocates; aidax_pool_metering reads a host record of the audio side) and the first aidax_pool_set_gate with parameters (it allocates too; aidax_pool_stream_gate reads a host record of the audio side) and the first aidax_pool_set_buses with a count (it allocates as well; aidax_pool_buses and aidax_pool_stream_send read host records of the audio side) and the first aidax_pool_set_bus_limiting with on != 0 (it allocates; aidax_pool_bus_limiting and aidax_pool_bus_limiter read host records of the audio side) and the first aidax_pool_set_bus_reverbs with on != 0 (it allocates; aidax_pool_bus_reverbs and aidax_pool_bus_reverb read host records of the audio side) and the first aidax_pool_set_delays with on != 0 (it allocates; aidax_pool_delays and aidax_pool_stream_delay read host records of the audio side); aidax_gate_design, aidax_mix_gain, aidax_bus_limit_design, aidax_bus_reverb_design and aidax_delay_design are pure: any thread; aidax_ir_resample and aidax_ir_load_wav are host only and touch no pool: any thread, the worker by
 * habit. aidax_rate_create and aidax_rate_destroy are set-up side calls (the adapter's blocks are the audio side's, above), a bare
 * aidax_resampler belongs to one caller at a time, and aidax_rate_latency and aidax_resampler_row touch nothing: any thread. None of the audio-side calls allocates or frees device or pinned memory, and only
 * aidax_pool_process / aidax_pool_process_buses / aidax_pool_sync / aidax_rate_process / aidax_pool_read_meters / aidax_pool_read_gate / aidax_pool_read_buses / aidax_pool_read_bus_meters / aidax_pool_read_delays wait for the GPU (for the stream that carries the pass, never for the
 * device) — with one exception in every pass: changed control records, a changed IR plan (after an assign_ir, an assign_ir_b, a set_ir_mix or a commit_ir, and when a ramp ends on 0 or 1) changed model-bank records (after an assign_model) changed gate records (after a set_gate), a changed mix plan (after a set_send) changed bus limiter records (after a set_bus_limiter) and changed bus reverb records (after a set_bus_reverb, a set_bus_reverb_rec or a reset_bus_reverb, and once in 2^30 frames when an epoch is moved forward) and changed delay records (after a set_delay or a set_delay_rec), go
 * to the device from a ring of four pinned snapshots, and a pass waits for the upload issued four changes before its own if that has
 * not run yet. That happens only to a caller that issues passes far ahead of the GPU (process_device, submit) with a change before
 * each of five passes in a row. */

/* One stream becomes a fresh plugin instance with the pool's model: instantiate() state for its DSP
 * members (:283-321; gain smoothers pre = 1 / master = 0 cleared, biquad states 0) and a fresh DynamicModel
 * (:1035-1079: reset, PARAM smoothers rebuilt, warm-up per start_mode), loading cleared if the pool has a
 * model. Used when a host attaches a new instance to a running pool (aidax_hub below). */
AIDAX_API int  aidax_pool_reset_stream(aidax_pool* p, uint32_t stream, int start_mode);

/* The plugin-owned DSP members of one stream — what RtNeuralGeneric keeps in itself rather than in its DynamicModel
 * (rt-neural-generic.h:311-317: seven Biquads, preGain, masterGain) and therefore keeps across a model swap (:868-875) —
 * plus the PARAM targets of the playing model, which work() hands to the next one (:822-825). */
typedef struct {
    double z[7][2];            /* Biquad z1, z2 (common/Biquad.h:50): in_lpf, dc_blocker, depth, bass, mid, treble, presence */
    float  pre_mem, master_mem, pre_target, master_target;     /* ExponentialValueSmoother mem / target as last set */
    float  param_target[2];    /* LinearValueSmoother targets of the playing model (0 / 0 without one) */
} aidax_stream_dsp;

/* Read / write those members of one stream. Both wait for the pool's passes (worker / main thread, tests); the
 * audio-thread way of moving a plugin instance between pools is aidax_hub_adopt below. import leaves the PARAM
 * smoothers alone (they belong to the pool's model) and, like a model swap, arms no activate(). */
AIDAX_API int  aidax_pool_export_stream_dsp(aidax_pool* p, uint32_t stream, aidax_stream_dsp* out);
AIDAX_API int  aidax_pool_import_stream_dsp(aidax_pool* p, uint32_t stream, const aidax_stream_dsp* in);

/* The `loading` flag (:318, :576, :889): while set, the master gain target is 0. */
AIDAX_API int  aidax_pool_set_loading(aidax_pool* p, int32_t stream, int loading);

/* Latch the control-port values run() reads at :489-502 for one stream or
 * AIDAX_ALL_STREAMS. Biquad coefficients are recomputed on the host exactly
 * where the reference's change detection would (:68-127, :514-517). */
AIDAX_API int  aidax_pool_set_controls(aidax_pool* p, int32_t stream, const aidax_controls* c);

/* activate() (:337-351): clear both gain smoothers to their current targets and
 * re-arm paramFirstRun. Recurrent state is NOT reset (the reference's reset is #if 0). */
AIDAX_API int  aidax_pool_activate(aidax_pool* p, int32_t stream);

/* run(), audio half (:607-659), for all streams: `in`/`out` are host buffers
 * laid out [n_streams][n_frames] (in-place allowed). Blocking: waits for the pool's stream. n_frames == 0 is
 * the legal "pre-run" (:606-609) and only latches targets. The block travels through pinned staging that the
 * pool allocated at creation (blocks of <= 64 KiB — the one-instance plugin — are read and written by the
 * kernels in place in pinned host memory, no copy engine involved; AIDAX_ZEROCOPY=0 turns that off — and such
 * a pool learns of the pass's end from a word the stream writes into pinned host memory, which the caller polls:
 * no interrupt and no wake-up on the way back; AIDAX_SPIN_WAIT=0 waits with hipStreamSynchronize instead). */
AIDAX_API int  aidax_pool_process(aidax_pool* p, const float* in, float* out, uint32_t n_frames);

/* The same pass for a host that streams blocks: submit() stages block k (pinned copy, upload on a copy stream, the
 * pass, download on another copy stream) and returns; collect() waits for the OLDEST submitted block and copies it
 * out. With one block kept in flight — submit(k+1) before collect(k) — the upload of k+1 and the download of k-1 run
 * under the pass of k; with two — submit(k+2) before collect(k) — the host's own round trip (a download, the caller's
 * turn-around, an upload) is off the GPU's critical path as well and the pass is what bounds the rate. At most three
 * blocks between submit and collect (AIDAX_ERR_STATE beyond); collect's n_frames is the submitted block's. One caller
 * thread. The first submit allocates the staging sets: make it before going real-time. */
AIDAX_API int  aidax_pool_submit(aidax_pool* p, const float* in, uint32_t n_frames);
AIDAX_API int  aidax_pool_collect(aidax_pool* p, float* out, uint32_t n_frames);

/* A host that hands over the SAME buffers block after block (the reference's run() gets the host's port buffers,
 * rt-neural-generic.cpp:484-487) can have them pinned once: register_host() page-locks a range of the caller's memory
 * for the pool's device (set-up side: it allocates and may block; the range must stay mapped until unregister_host() or
 * the pool's end). submit() then uploads a block that lies inside a registered range straight out of it — no copy into
 * the pool's staging — and submit_to() names the block's destination up front, so that the download lands there as well
 * and collect() (same `out`) only waits. Buffers outside any registered range take the staged path as before.
 * OWNERSHIP: a block that lies inside a registered range is read by the copy engine AFTER submit() has returned, and a
 * registered `out` is written BEFORE collect() returns — such buffers belong to the pool from submit()/submit_to() until the
 * collect() of that block. With one block kept in flight the host therefore alternates TWO in/out buffer pairs (write block
 * k+1's input while block k's is still the pool's); a host with a single pair collects before it reuses it. (Unregistered
 * buffers are copied into the pool's staging inside submit() and out of it inside collect(): theirs is the usual lifetime.) */
AIDAX_API int  aidax_pool_register_host(aidax_pool* p, void* base, size_t bytes);
AIDAX_API int  aidax_pool_unregister_host(aidax_pool* p, void* base);
AIDAX_API int  aidax_pool_submit_to(aidax_pool* p, const float* in, float* out, uint32_t n_frames);

/* Same pass with device-resident buffers, asynchronous on `hip_stream`
 * (a hipStream_t; NULL = the pool's own stream). No host sync inside. The pool's control pokes (activate,
 * reset_stream, commit_model) run on its own stream; when consecutive operations sit on different streams the
 * pool puts an event edge between them, so program order is kept. A stream handed in here must stay valid
 * until a later call names another one (or NULL), or the pool is destroyed. */
AIDAX_API int  aidax_pool_process_device(aidax_pool* p, const float* d_in, float* d_out,
                                         uint32_t n_frames, void* hip_stream);
/* Waits for the pool's passes. AIDAX_ERR_DEVICE also when a pass since the last report went wrong on the device:
 * the stacked-model kernel k_mfma_lp runs a stream group's layers on separate workgroups that wait for each other, and
 * gives a wait up after 250 ms (another process holding the GPU's CUs); the blocking aidax_pool_process reports the same
 * for its own block and returns silence. The pool serves the model with the one-workgroup-per-group kernel from then on. */
AIDAX_API int  aidax_pool_sync(aidax_pool* p);

/* testModel() (:900-955) on the GPU: input_batch through the bare model from
 * reset state with gains forced to 1 and params forced to 0, compared with
 * output_batch at TEST_MODEL_THR = 1e-5 (rt-neural-generic.h:182). Uses a
 * scratch single-stream pool on `device_id`. out_opt (n_golden floats) may be NULL. */
AIDAX_API int  aidax_model_self_test(const aidax_model* m, int device_id, int32_t* n_errors,
                                     float* max_error, float* out_opt);

/* Bare applyModel (:148-240) from reset state for arbitrary conditioned input:
 * X is [n][input_size] (audio, p1, p2 per sample), y is [n]; gains and skip per
 * the model unless unit_gains != 0. For parity tests against NN-only fixtures. */
AIDAX_API int  aidax_model_forward(const aidax_model* m, int device_id, const float* X, float* y,
                                   uint32_t n, int unit_gains);

/* Introspection for tests: copies one stream's recurrent state (h then c of
 * rnn layer `layer`) to host. Returns hidden size or <0. */
AIDAX_API int  aidax_pool_read_state(aidax_pool* p, uint32_t stream, int layer, float* h, float* c, uint32_t cap);

/* Name of the kernel instantiation a loaded pool dispatches to (profiling aid). */
AIDAX_API const char* aidax_pool_kernel_name(const aidax_pool* p);

/* --------------------------------------------------------------------- hub
 * Host-side stream aggregator (new relative to the reference, whose seam is the
 * per-instance DSP section rt-neural-generic.cpp:621-659). Many plugin instances of ONE process share one
 * pool: each instance attaches to a slot and calls aidax_hub_run() from its run(); the hub launches one
 * pool pass per audio period for everybody.
 *
 * Hosts call the instances of a period one after another on one thread, or in parallel on several; a
 * rendezvous inside run() would deadlock the first kind, so the hub is pipelined by ONE period instead:
 * run() of period p stages the instance's input block and returns the output of period p-1 (silence in the
 * first period). The pass of a period is launched (asynchronously: H2D, kernels, D2H) by the hub's launcher
 * thread as soon as every attached instance has submitted — or when the period's DEADLINE passes (by default
 * half the period after its first submission, aidax_hub_set_deadline_us), so an instance that stalls or
 * stops calling cannot hold the others: they keep their one period of latency, the straggler's stream simply
 * does not advance in that pass. An instance that comes around again before the period was closed, or a change
 * of block size, closes it on the spot. An instance reads the output of the pass that carried ITS previous block
 * while that is at most two passes old and of the same length (a period that was closed in pieces), silence
 * otherwise. run() itself waits only for the event of that pass, outside the hub's lock; the staging buffers
 * rotate over four passes, and a host that closes periods faster than the GPU finishes them waits for the pass
 * four back before its staging is reused. Controls, the loading flag and activate() of an instance whose block still
 * waits for its pass close the period first: a submitted block plays under what was in force when it was submitted. Report aidax_hub_latency_frames() to the host as the plugin's latency. Thread-safe. */
typedef struct aidax_hub aidax_hub;

AIDAX_API int  aidax_hub_create(uint32_t max_instances, uint32_t max_frames, double host_samplerate,
                                int device_id, aidax_hub** out);
AIDAX_API void aidax_hub_destroy(aidax_hub* h);
/* every attached instance plays this model (instances with another model belong to another hub) */
AIDAX_API int  aidax_hub_set_model(aidax_hub* h, const aidax_model* m, int start_mode);
/* a new instance: *slot receives its index; its stream starts from instantiate() + warm-up state */
AIDAX_API int  aidax_hub_attach(aidax_hub* h, int32_t* slot);
/* An instance that plays on (prev, prev_slot) and changes its model file moves to the hub of the new file — a model
 * swap of the reference (work() :807-836, work_response() :859-893) spread over two hubs:
 *   aidax_hub_attach_successor   worker thread: a seat in `h` whose fresh DynamicModel is built (and warmed up) around
 *                                the PARAM targets the predecessor's model holds (:822-825); launches the
 *                                predecessor's pending block and waits for it, outside the hubs' locks. prev may be
 *                                NULL (first load: plain attach).
 *   aidax_hub_adopt              audio thread, at the swap: the new seat takes over the plugin's own DSP members
 *                                (aidax_stream_dsp: biquad memories, gain smoothers) by a device-side copy ordered
 *                                behind the predecessor's last pass. No wait, no allocation. The predecessor's seat
 *                                is detached afterwards (worker), as the old DynamicModel is freed there (:838-840). */
AIDAX_API int  aidax_hub_attach_successor(aidax_hub* h, aidax_hub* prev, int32_t prev_slot, int32_t* slot);
AIDAX_API int  aidax_hub_adopt(aidax_hub* h, int32_t slot, aidax_hub* prev, int32_t prev_slot);
AIDAX_API int  aidax_hub_detach(aidax_hub* h, int32_t slot);
AIDAX_API int  aidax_hub_set_controls(aidax_hub* h, int32_t slot, const aidax_controls* c);
/* the instance's `loading` flag and activate(), as aidax_pool_set_loading / aidax_pool_activate for its stream */
AIDAX_API int  aidax_hub_set_loading(aidax_hub* h, int32_t slot, int loading);
AIDAX_API int  aidax_hub_activate(aidax_hub* h, int32_t slot);
/* the instance's run(): in/out are its n_frames-long port buffers (may alias) */
AIDAX_API int  aidax_hub_run(aidax_hub* h, int32_t slot, const float* in, float* out, uint32_t n_frames);
/* deadline of a period, measured from its first submission: < 0 half the period (default), 0 none
 * (passes are launched only when everybody submitted, on re-entry, or by aidax_hub_flush) */
AIDAX_API int  aidax_hub_set_deadline_us(aidax_hub* h, int64_t microseconds);
/* close the period being collected now (hosts that know their graph is done; tests) */
AIDAX_API int  aidax_hub_flush(aidax_hub* h);
AIDAX_API uint32_t aidax_hub_latency_frames(const aidax_hub* h);
AIDAX_API uint32_t aidax_hub_attached(const aidax_hub* h);
/* the longest block aidax_hub_run accepts (callers slice longer host blocks: the LV2 shell does) */
AIDAX_API uint32_t aidax_hub_max_frames(const aidax_hub* h);
/* number of pool passes launched so far (tests, statistics) */
AIDAX_API uint64_t aidax_hub_launches(const aidax_hub* h);
/* ... of which were launched by the deadline with somebody missing */
AIDAX_API uint64_t aidax_hub_deadline_launches(const aidax_hub* h);
/* Diagnostic: hand-over give-ups of the stacked-model kernel (see aidax_pool_sync) that the hub could attribute to no pass of a chained
 * kernel — nothing was silenced for them; a non-zero count on a healthy system is a bug report. */
AIDAX_API uint64_t aidax_hub_faults_unmapped(const aidax_hub* h);

#ifdef __cplusplus
}
#endif
#endif /* AIDAX_H */
