// aidax_pool_model.cpp — everything that builds or commits an aidax_staged (aidax_pool.h): a model, a model-bank slot or a cabinet IR on
// its way into a pool — prepared on the worker thread, committed on the audio thread — and the entry points that ask which form and
// kernel serve a model. Host logic only.
#include <hip/hip_runtime_api.h>

#include <cmath>

#include "aidax_pool.h"
#include "aidax_load_form.h"

namespace aidax {

void staged_release(aidax_staged* s)
{
    if (!s) return;
    (void)hipSetDevice(s->device);
    if (s->fenced) (void)hipEventSynchronize(s->fence.get());   // passes that still read the retired buffers
    if (s->slot.lp_owner) lp_gate().release(s->device, s->slot.lp_owner);
    DevBuf<uint32_t>::adopt(s->ir.d_frag);                      // (the two records' blocks; the owning members go back with the object)
    DevBuf<float>::adopt(s->bank.d_wpack);
    delete s;
}

StagedPtr new_staged(const aidax_pool& p, aidax_staged::Payload payload)
{
    StagedPtr sg(new aidax_staged(), staged_release);
    sg->device = p.device; sg->n_streams = p.n_streams; sg->payload = payload;
    sg->fence.create();
    return sg;
}

namespace {

// what prepare_impl uploads and allocates next to the slot: the weights in the chosen kernel's layout, k_lstm_q4's record where asked for; lp: the
// model gets a hand-over ring (and, stacked, a hold on the device's LpGate) — k_mfma_ls's for ring_streams streams where ls, else k_mfma_lp's
struct Packed { std::vector<float> wp, wq4; bool lp = false, ls = false; uint32_t ring_streams = 0; };

// The test switches of the load-form decision (aidax_load_form.h), read on every load and every ABI call: tests switch forms within one
// process. The ONE place that reads the environment for these names; the shipped library compiles every read to "unset".
FormHooks read_form_hooks()
{
    auto tri = [](const char* e) { return !e ? -1 : e[0] != '0' ? 1 : 0; };
    auto is0 = [](const char* e) { return e && e[0] == '0'; };
    auto one_of = [](const char* e, char a, char b) { return e && (e[0] == a || e[0] == b) ? e[0] : '\0'; };
    FormHooks h;
    h.ls1 = tri(AIDAX_HOOK_ENV("AIDAX_LS1"));
    h.lstm_gs = tri(AIDAX_HOOK_ENV("AIDAX_LSTM_GS"));
    h.gru_gm = one_of(AIDAX_HOOK_ENV("AIDAX_GRU_GM"), '0', 'f');
    h.mfma_lp = tri(AIDAX_HOOK_ENV("AIDAX_MFMA_LP"));
    h.lp_split = one_of(AIDAX_HOOK_ENV("AIDAX_LP_SPLIT"), '0', '9');
    h.lp_fused_off = is0(AIDAX_HOOK_ENV("AIDAX_LP_FUSED"));
    const char* rg = AIDAX_HOOK_ENV("AIDAX_LP_ROUND_GROUPS");
    h.round_groups_set = rg != nullptr;
    h.round_groups = rg ? std::atoi(rg) : 0;
    const char* np = AIDAX_HOOK_ENV("AIDAX_GS_PRODUCTS");
    h.gs_products = np && np[0] == '9' ? 9 : 6;
    h.conv_ms_off = is0(AIDAX_HOOK_ENV("AIDAX_CONV_MS"));
    h.conv_st_off = is0(AIDAX_HOOK_ENV("AIDAX_CONV_ST"));
    h.conv_fused = tri(AIDAX_HOOK_ENV("AIDAX_CONV_FUSED"));
    return h;
}

// Which kernel form serves model m in pool p: packs the weights in the layout of the kind that load_kind names, gathers the facts the packed
// descriptor gives, lets aidax_load_form.h decide and fills the slot's host fields, its SlotForm among them. No allocation, no launch; the
// CU count is the pool's (aidax_pool_create asked the device), the occupancy answers are the kernels' own. A chained form holds while the
// slot has its ring (PassFacts::ring_ready): prepare_impl may not get one.
int choose_form(const aidax_pool& p, const aidax_model* m, ModelSlot& ms, Packed& pk)
{
    constexpr size_t kCuLds = 160 * 1024;
    const FormHooks h = read_form_hooks();
    const LoadPool pool{ p.n_streams, p.max_frames, p.cus, p.force, p.packed_fits };
    const ModelShape shape{ m->cell, m->hidden, m->n_rnn, is_conv_model(*m), is_stack_model(*m), find_kernel(m->cell, m->hidden) != nullptr, mfma_form_fits(*m) };
    std::vector<float>& wp = pk.wp;
    uint32_t state_floats = 0;
    switch (load_kind(pool, h, shape, quad_lds_bytes(m->hidden, p.max_frames) <= kCuLds)) {
    case LoadKind::Conv: {
        ms.kind = ModelSlot::CONV;
        wp = pack_conv(*m, &ms.cdesc, &state_floats);
        const ConvFamily fam = conv_family(pool, h, convm_lds_bytes(ms.cdesc, p.ext_chunk()) <= kCuLds, ms.cdesc.ms_ok != 0, conv_lds_bytes(ms.cdesc, p.max_frames) <= kCuLds);
        if (fam.refused) return fail(AIDAX_ERR_ARG, "conv model: pool max_frames too large for the LDS activation planes");
        if (fam.clear_st) ms.cdesc.st_ok = 0;
        if (fam.ms) state_floats = ms.cdesc.ms_state_floats;
        const int resident = !fam.by_size ? 0 : fam.ms ? convs_resident_streams(p.device, ms.cdesc.st_ok - 1) : convm_resident_streams(ms.cdesc, p.ext_chunk(), p.device);
        ms.form = conv_form(fam, pool, h, resident);
        break;
    }
    case LoadKind::Quad:
        ms.kind = ModelSlot::QUAD;
        ms.form = SlotForm::quad();
        wp = pack_quad(*m, &ms.qdesc.bias_off, &ms.qdesc.dense_off);
        state_floats = static_cast<uint32_t>(m->cell == AIDAX_CELL_LSTM ? 2 * m->hidden : m->hidden);
        break;
    case LoadKind::Mfma: {
        ms.kind = ModelSlot::MFMA;
        wp = pack_mfma(*m, &ms.mdesc, &state_floats);
        const MfmaDesc& d = ms.mdesc;
        MfmaFacts f{};
        f.n_layers = d.n_layers; f.hidden = d.hidden; f.cell0 = d.L[0].cell;
        f.lp_serves = mfma_lp_serves(d); f.lp_fused_serves = mfma_lp_fused_serves(d, p.max_frames);
        f.ls_serves = mfma_ls_serves(d); f.ls_fused_serves = mfma_ls_fused_serves(d, p.max_frames);
        f.gru_gm_serves = gru_gm_serves(d); f.gru_gs_serves = gru_gs_serves(d); f.lstm_gs_serves = lstm_gs_serves(d);
        // (a kernel's LDS is asked of the descriptors it serves only)
        f.lp_lds_ok = f.lp_serves && mfma_lp_lds_bytes(d, p.max_frames) <= kCuLds;
        f.lp_fused_lds_ok = f.lp_fused_serves && mfma_lp_lds_bytes(d, p.max_frames, true) <= kCuLds;
        f.ls_lds_ok = f.ls_serves && mfma_ls_lds_bytes(d, p.max_frames) <= kCuLds;
        f.ls_fused_lds_ok = f.ls_fused_serves && mfma_ls_lds_bytes(d, p.max_frames, true) <= kCuLds;
        f.gru_gm_lds_ok = f.gru_gm_serves && gru_gm_lds_bytes(d, p.max_frames) <= kCuLds;
        f.gru_gs_lds_ok = f.gru_gs_serves && gru_gs_lds_bytes(d, p.max_frames) <= kCuLds;
        f.lstm_gs_lds_ok = f.lstm_gs_serves && lstm_gs_lds_bytes(d, p.max_frames) <= kCuLds;
        const MfmaChoice c = mfma_form(pool, h, shape, f);
        ms.form = c.form;
        pk.lp = c.lp; pk.ls = c.ls; pk.ring_streams = c.ring_streams;
        break;
    }
    case LoadKind::Stack:
        ms.kind = ModelSlot::STACK;
        ms.form = SlotForm::stack();
        wp = pack_stack(*m, &ms.sdesc, &state_floats);
        if (stack_lds_bytes(ms.sdesc, p.max_frames) > kCuLds)
            return fail(AIDAX_ERR_ARG, "stacked model: pool max_frames too large for the LDS block buffers");
        break;
    case LoadKind::Table: {
        ms.kind = ModelSlot::TABLE;
        ms.kernel = find_kernel(m->cell, m->hidden);
        wp = pack_weights(*m);
        const int alt = (m->cell == AIDAX_CELL_LSTM && lstm_has_alt_pack(m->hidden)) ? lstm_pack_regs(m->hidden, false) * kWave : 0;   // a natural-order copy for k_nn
        if (static_cast<int>(wp.size()) != ms.kernel->pack_regs * kWave + m->hidden + 1 + alt) return fail(AIDAX_ERR_STATE, "weight pack size mismatch");
        state_floats = static_cast<uint32_t>(ms.kernel->state_floats);
        // AIDAX_KERNEL=q4 (A/B runs and tests only): LSTM-32 snapshot models, four streams per workgroup with the cell on the
        // matrix cores; the table kernels' record stays for warm-ups and the bare-model modes
        if (q4_serves(m->cell, m->hidden, m->input_size) && p.force == Force::Q4 && q4_lds_bytes(m->hidden, p.max_frames) <= 64 * 1024) pk.wq4 = pack_q4(*m);
        ms.form = SlotForm::table(pipe_resident_streams(ms.kernel, p.max_frames, p.device), split_form_pays(ms.kernel, p.max_frames), !pk.wq4.empty());
        break;
    }
    }
    ms.nn_stride = (state_floats + 3u) & ~3u;
    ms.cell = m->cell;
    ms.hidden = m->hidden;
    ms.input_size = m->input_size;
    ms.input_skip = m->input_skip;
    ms.in_gain = m->input_gain;
    ms.out_gain = m->output_gain;
    ms.model_sr = m->samplerate;
    ms.has_model = true;
    return AIDAX_OK;
}

// loadModelFromPath's device half (rt-neural-generic.cpp:1034-1079) into buffers of its own. Worker thread:
// packs, allocates, uploads and warms up on the pool's worker stream and waits for it; touches nothing the
// audio side uses except for reading each stream's PARAM targets (as work() reads them at :822-825).
int prepare_impl(aidax_pool& p, const aidax_model* m, int start_mode, aidax_staged** out)
{
    HIP_TRY(hipSetDevice(p.device));
    StagedPtr sg = new_staged(p, aidax_staged::MODEL);
    if (!m) {                                             // unload: an empty slot to swap in
        *out = sg.release();
        return AIDAX_OK;
    }
    if (!model_supported(*m)) return fail(AIDAX_ERR_ARCH, "Unable to identify a known model architecture! (no kernel)");
    ModelSlot& ms = sg->slot;
    Packed pk;                                            // (lives until the stream has been waited for below)
    if (const int rc = choose_form(p, m, ms, pk)) return rc;
    const std::vector<float>& wp = pk.wp;
    ms.d_wpack.alloc(wp.size());
    ms.d_nn.alloc(static_cast<size_t>(p.n_streams) * ms.nn_stride);
    sg->d_pst.alloc(p.n_streams);
    const bool lp_chained = ms.mdesc.n_layers >= 2;       // (only a hand-over between layers needs the hold on the device's gate)
    if (pk.lp && !(lp_chained && p.lp_off.load()) && (!lp_chained || lp_gate().acquire(p.device, &p, &p.lp_off))) {
        if (lp_chained) ms.lp_owner = &p;
        const size_t ring_bytes = pk.ls ? mfma_ls_ring_bytes(ms.mdesc, pk.ring_streams) : mfma_lp_ring_bytes(ms.mdesc, p.n_streams);
        ms.d_ring.alloc((ring_bytes + sizeof(float) - 1) / sizeof(float));
        ms.d_counters.alloc((mfma_lp_counter_bytes(ms.mdesc, p.n_streams) + sizeof(uint32_t) - 1) / sizeof(uint32_t));
        HIP_TRY(hipMemsetAsync(ms.d_counters.get(), 0, mfma_lp_counter_bytes(ms.mdesc, p.n_streams), p.wq));
    }
    HIP_TRY(hipMemcpyAsync(ms.d_wpack.get(), wp.data(), wp.size() * sizeof(float), hipMemcpyHostToDevice, p.wq));
    if (!pk.wq4.empty()) {
        ms.d_wq4.alloc(pk.wq4.size());
        HIP_TRY(hipMemcpyAsync(ms.d_wq4.get(), pk.wq4.data(), pk.wq4.size() * sizeof(float), hipMemcpyHostToDevice, p.wq));
    }
    // fresh DynamicModel per stream: reset() + param smoothers around the targets the playing model holds now
    // (:822-825, :1035, :1053-1061) ...
    HIP_TRY(launch_stage_params(p.d_st.get(), sg->d_pst.get(), p.n_streams, p.wq));
    HIP_TRY(launch_reset_for_model(sg->d_pst.get(), ms.d_nn.get(), p.n_streams, ms.nn_stride, ms.p_den(), p.wq));
    if (start_mode == AIDAX_START_WARMUP) {               // ... and 2048 zeros through applyModel (:1077-1078)
        const uint32_t chunk = p.launch_chunk(ms, kWarmupFrames);
        for (uint32_t done = 0; done < kWarmupFrames; done += chunk) {
            LaunchArgs a = p.args(ms, sg->d_pst.get(), nullptr, nullptr, std::min(chunk, kWarmupFrames - done), MODE_WARMUP);
            HIP_TRY(p.launch(ms, a, p.wq));
        }
    }
    HIP_TRY(hipStreamSynchronize(p.wq));                  // `wp` is pageable; the audio side must find the model complete
    *out = sg.release();
    return AIDAX_OK;
}

// work_response() (:859-893): swap, loading = false. Audio thread: host assignments plus one tiny kernel on the
// pool's stream; no allocation, no free, no wait.
int commit_impl(aidax_pool& p, aidax_staged* sg)
{
    if (sg->slot.has_model) HIP_TRY(launch_install_params(p.d_st.get(), sg->d_pst.get(), p.n_streams, p.q));
    HIP_TRY(hipEventRecord(sg->fence.get(), p.q));              // the retired buffers are free once this has passed
    sg->fenced = true;
    std::swap(p.cur, sg->slot);
    const uint8_t loading = p.cur.has_model ? 0 : 1;      // :889 (unload: loading = true)
    for (uint32_t s = 0; s < p.n_streams; ++s) {
        p.loading[s] = loading;
        p.patch_model_fields(s);
    }
    p.ctl_dirty.mark(0, p.n_streams - 1);
    return AIDAX_OK;
}

}  // namespace
}  // namespace aidax

extern "C" {

AIDAX_API int aidax_pool_prepare_model(aidax_pool* p, const aidax_model* m, int start_mode, aidax_staged** out)
{
    if (!p || !out) return fail(AIDAX_ERR_ARG, "null argument");
    *out = nullptr;
    if (start_mode != AIDAX_START_WARMUP && start_mode != AIDAX_START_RESET) return fail(AIDAX_ERR_ARG, "bad start_mode");
    return guarded([&]() { return prepare_impl(*p, m, start_mode, out); });
}

AIDAX_API int aidax_pool_commit_model(aidax_pool* p, aidax_staged* staged)
{
    if (!p || !staged) return fail(AIDAX_ERR_ARG, "null argument");
    if (staged->payload == aidax_staged::IR) return fail(AIDAX_ERR_ARG, "staged object holds an IR: commit it with aidax_pool_commit_ir");
    if (staged->fenced) return fail(AIDAX_ERR_STATE, "staged model was committed already");
    if (staged->device != p->device || staged->n_streams != p->n_streams) return fail(AIDAX_ERR_ARG, "staged model belongs to another pool");
    ModelBank* b = p->bank.adopt();
    if (staged->payload == aidax_staged::BANK_SLOT) {
        // a bank slot's content: host integers, then the swap and the fence behind everything that may still read the retired weights
        if (!b) return fail(AIDAX_ERR_STATE, "the pool has no model bank");
        if (const int rc = b->may_commit_slot(staged->bank_slot, staged->bank, p->cur.arch())) return rc;
        return p->on_own_stream([&]() -> int {
            HIP_TRY(hipEventRecord(staged->fence.get(), p->q));
            staged->fenced = true;
            b->commit_slot(staged->bank_slot, staged->bank);
            return AIDAX_OK;
        });
    }
    if (const int rc = b ? b->may_commit_pool_model(staged->slot.arch()) : AIDAX_OK) return rc;
    return p->on_own_stream([&] { return commit_impl(*p, staged); });
}

// Worker thread: the slot's weights in the pool model's layout, uploaded on the worker stream; the first call allocates the bank.
AIDAX_API int aidax_pool_prepare_model_slot(aidax_pool* p, uint32_t slot, const aidax_model* m, aidax_staged** out)
{
    if (out) *out = nullptr;
    if (!p || !out) return fail(AIDAX_ERR_ARG, "null argument");
    if (slot >= static_cast<uint32_t>(AIDAX_MODEL_SLOTS)) return fail(AIDAX_ERR_ARG, "model slot must be 0 .. 63");
    const ModelSlot& cur = p->cur;
    if (!cur.has_model) return fail(AIDAX_ERR_STATE, "the pool has no model: the bank holds variants of the pool model");
    const char* other_kernel = !m || (cur.kind == ModelSlot::TABLE && cur.kernel) ? nullptr : aidax_pool_kernel_name(p);
    if (const int rc = m ? bank_may_stage(*m, cur.arch(), other_kernel, pipe_lds_bytes(cur.hidden, p->max_frames) <= 64 * 1024) : AIDAX_OK) return rc;
    return guarded([&]() -> int {
        HIP_TRY(hipSetDevice(p->device));
        StagedPtr sg = new_staged(*p, aidax_staged::BANK_SLOT);
        sg->bank_slot = slot;
        const int alt = (m && m->cell == AIDAX_CELL_LSTM && lstm_has_alt_pack(m->hidden)) ? lstm_pack_regs(m->hidden, false) * kWave : 0;
        p->bank.prepare(p->n_streams, m, m ? cur.kernel->pack_regs * kWave + m->hidden + 1 + alt : 0, sg->bank, p->wq);
        *out = sg.release();
        return AIDAX_OK;
    });
}

// The set-up side's one-call forms: prepared content (rc: its prepare's result) committed at once, and what the swap retired (or, on
// failure, the unused content) freed
static int commit_and_free(aidax_pool* p, int rc, aidax_staged* sg, int (*commit)(aidax_pool*, aidax_staged*))
{
    if (rc == AIDAX_OK) rc = commit(p, sg);
    aidax_staged_free(sg);
    return rc;
}

AIDAX_API int aidax_pool_set_model_slot(aidax_pool* p, uint32_t slot, const aidax_model* m)
{
    aidax_staged* sg = nullptr;
    const int rc = aidax_pool_prepare_model_slot(p, slot, m, &sg);
    return commit_and_free(p, rc, sg, aidax_pool_commit_model);
}

// Audio side, between passes: the stream becomes a fresh DynamicModel of the slot's model (:822-825, :1046-1079) — host records plus
// the launches aidax_pool_reset_stream issues for the same purpose, on the pool's stream behind every pass issued so far.
AIDAX_API int aidax_pool_assign_model(aidax_pool* p, int32_t stream, int32_t slot, int start_mode)
{
    if (!p) return fail(AIDAX_ERR_ARG, "null pool");
    if (stream < 0 || static_cast<uint32_t>(stream) >= p->n_streams) return fail(AIDAX_ERR_ARG, "stream out of range (one stream per call)");
    if (slot != AIDAX_MODEL_POOL && (slot < 0 || slot >= AIDAX_MODEL_SLOTS)) return fail(AIDAX_ERR_ARG, "model slot must be the pool model (-1) or 0 .. 63");
    if (start_mode != AIDAX_START_WARMUP && start_mode != AIDAX_START_RESET) return fail(AIDAX_ERR_ARG, "bad start_mode");
    ModelBank* b = p->bank.adopt();
    if (slot >= 0 && (!b || !b->slot[slot].loaded)) return fail(AIDAX_ERR_STATE, "model bank slot " + std::to_string(slot) + " is empty");
    if (!p->cur.has_model) return fail(AIDAX_ERR_STATE, "the pool has no model");
    const uint32_t s = static_cast<uint32_t>(stream);
    return p->on_own_stream([&]() -> int {
        const ModelSlot& m = p->cur;
        p->fresh_stream_model(m, s, start_mode, slot >= 0 ? ModelBank::rec_of(b->slot[slot]) : m.rec(), p->q);
        if (b) b->assign_stream(s, slot, m.rec());          // (no bank: the stream was and stays on the pool model)
        return AIDAX_OK;
    });
}

AIDAX_API int aidax_pool_stream_model(const aidax_pool* p, uint32_t stream, int32_t* slot)
{
    if (!p || !slot) return fail(AIDAX_ERR_ARG, "null argument");
    if (stream >= p->n_streams) return fail(AIDAX_ERR_ARG, "stream out of range");
    const ModelBank* b = p->bank.adopt();
    *slot = b ? b->assign[stream] : AIDAX_MODEL_POOL;
    return AIDAX_OK;
}

AIDAX_API void aidax_staged_free(aidax_staged* staged) { staged_release(staged); }

AIDAX_API int aidax_pool_set_model(aidax_pool* p, const aidax_model* m, int start_mode)
{
    aidax_staged* sg = nullptr;
    const int rc = aidax_pool_prepare_model(p, m, start_mode, &sg);
    return commit_and_free(p, rc, sg, aidax_pool_commit_model);
}

// The cabinet IR, split between the threads like a model swap (IrStage::prepare on the worker, IrStage::commit on the audio thread).
static int prepare_ir_impl(aidax_pool* p, int32_t slot, const float* taps, uint32_t n_taps, double samplerate, aidax_staged** out)
{
    if (!p || !out) return fail(AIDAX_ERR_ARG, "null argument");
    *out = nullptr;
    if (slot != AIDAX_IR_POOL && (slot < 0 || slot >= AIDAX_IR_SLOTS)) return fail(AIDAX_ERR_ARG, "IR slot must be 0 .. 63");
    if (taps) {
        const uint32_t capacity = p->ir.capacity.load(std::memory_order_relaxed);
        if (n_taps == 0 || n_taps > capacity)
            return fail(AIDAX_ERR_ARG, "IR length must be 1 .. " + std::to_string(capacity) + " taps" + (capacity != kIrMaxTaps ? " (the pool's IR capacity)" : ""));
        for (uint32_t k = 0; k < n_taps; ++k)
            if (!std::isfinite(taps[k])) return fail(AIDAX_ERR_ARG, "IR tap " + std::to_string(k) + " is not finite");
        if (samplerate != p->host_sr)
            return fail(AIDAX_ERR_ARG, "IR sample rate " + std::to_string(samplerate) + " differs from the pool's " + std::to_string(p->host_sr) + " (no resampling)");
    }
    return guarded([&]() -> int {
        HIP_TRY(hipSetDevice(p->device));
        StagedPtr sg = new_staged(*p, aidax_staged::IR);
        sg->ir_slot = slot;
        p->ir.prepare(taps, n_taps, sg->ir);
        *out = sg.release();
        return AIDAX_OK;
    });
}

AIDAX_API int aidax_pool_prepare_ir(aidax_pool* p, const float* taps, uint32_t n_taps, double samplerate, aidax_staged** out) { return prepare_ir_impl(p, AIDAX_IR_POOL, taps, n_taps, samplerate, out); }

AIDAX_API int aidax_pool_prepare_ir_slot(aidax_pool* p, uint32_t slot, const float* taps, uint32_t n_taps, double samplerate, aidax_staged** out)
{
    if (slot >= static_cast<uint32_t>(AIDAX_IR_SLOTS)) {
        if (out) *out = nullptr;
        return fail(AIDAX_ERR_ARG, "IR slot must be 0 .. 63");
    }
    return prepare_ir_impl(p, static_cast<int32_t>(slot), taps, n_taps, samplerate, out);
}

AIDAX_API int aidax_pool_commit_ir(aidax_pool* p, aidax_staged* staged)
{
    if (!p || !staged) return fail(AIDAX_ERR_ARG, "null argument");
    if (staged->payload != aidax_staged::IR) return fail(AIDAX_ERR_ARG, "staged object holds a model: commit it with aidax_pool_commit_model");
    if (staged->fenced) return fail(AIDAX_ERR_STATE, "staged IR was committed already");
    if (staged->device != p->device || staged->n_streams != p->n_streams) return fail(AIDAX_ERR_ARG, "staged IR belongs to another pool");
    return p->on_own_stream([&]() -> int {
        p->ir.commit(staged->ir_slot, staged->ir, staged->fence.get(), p->q);
        staged->fenced = true;
        return AIDAX_OK;
    });
}

AIDAX_API int aidax_pool_set_ir(aidax_pool* p, const float* taps, uint32_t n_taps, double samplerate)
{
    aidax_staged* sg = nullptr;
    const int rc = aidax_pool_prepare_ir(p, taps, n_taps, samplerate, &sg);
    return commit_and_free(p, rc, sg, aidax_pool_commit_ir);
}

AIDAX_API int aidax_pool_set_ir_slot(aidax_pool* p, uint32_t slot, const float* taps, uint32_t n_taps, double samplerate)
{
    aidax_staged* sg = nullptr;
    const int rc = aidax_pool_prepare_ir_slot(p, slot, taps, n_taps, samplerate, &sg);
    return commit_and_free(p, rc, sg, aidax_pool_commit_ir);
}

// Audio thread: host assignments only (the plan is rebuilt by the next pass).
AIDAX_API int aidax_pool_assign_ir(aidax_pool* p, int32_t stream, int32_t slot)
{
    if (!p) return fail(AIDAX_ERR_ARG, "null pool");
    if (stream != AIDAX_ALL_STREAMS && (stream < 0 || static_cast<uint32_t>(stream) >= p->n_streams))
        return fail(AIDAX_ERR_ARG, "stream out of range");
    if (slot != AIDAX_IR_POOL && slot != AIDAX_IR_NONE && (slot < 0 || slot >= AIDAX_IR_SLOTS))
        return fail(AIDAX_ERR_ARG, "IR slot must be the pool IR (-1), none (-2) or 0 .. 63");
    IrPlan& plan = p->ir.plan;
    if (stream == AIDAX_ALL_STREAMS) std::fill(plan.assign.begin(), plan.assign.end(), slot);
    else plan.assign[stream] = slot;
    plan.dirty = true;
    return AIDAX_OK;
}

// Audio thread: a host record (the plan is rebuilt by the next pass that finds a change).
AIDAX_API int aidax_pool_set_ir_fade(aidax_pool* p, uint32_t frames)
{
    if (frames > kIrMaxTaps) return fail(AIDAX_ERR_ARG, "IR fade length must be 0 .. 8192 frames");
    if (!p) return fail(AIDAX_ERR_ARG, "null pool");
    p->ir.plan.fade = frames;
    return AIDAX_OK;
}

AIDAX_API uint32_t aidax_pool_ir_fade(const aidax_pool* p) { return p ? p->ir.plan.fade : 0; }

// Audio thread: host assignments only. A stream at rest on A does not play its B side: the plan stands.
AIDAX_API int aidax_pool_assign_ir_b(aidax_pool* p, int32_t stream, int32_t slot)
{
    if (slot != AIDAX_IR_POOL && slot != AIDAX_IR_NONE && (slot < 0 || slot >= AIDAX_IR_SLOTS))
        return fail(AIDAX_ERR_ARG, "IR slot must be the pool IR (-1), none (-2) or 0 .. 63");
    if (!p) return fail(AIDAX_ERR_ARG, "null pool");
    if (stream != AIDAX_ALL_STREAMS && (stream < 0 || static_cast<uint32_t>(stream) >= p->n_streams))
        return fail(AIDAX_ERR_ARG, "stream out of range");
    IrPlan& plan = p->ir.plan;
    const uint32_t lo = stream == AIDAX_ALL_STREAMS ? 0u : static_cast<uint32_t>(stream), hi = stream == AIDAX_ALL_STREAMS ? p->n_streams : lo + 1u;
    for (uint32_t s = lo; s < hi; ++s) {
        if (plan.assign_b[s] == slot) continue;
        plan.assign_b[s] = slot;
        if (plan.rest(s) != 0) plan.dirty = true;
    }
    return AIDAX_OK;
}

// Audio thread: host records (every stream's ramp starts from its own weight of the last frame issued).
AIDAX_API int aidax_pool_set_ir_mix(aidax_pool* p, int32_t stream, float mix, uint32_t ramp_frames)
{
    if (!(mix >= 0.f && mix <= 1.f)) return fail(AIDAX_ERR_ARG, "IR mix must be a finite value in [0, 1]");
    if (ramp_frames > kIrMaxRamp) return fail(AIDAX_ERR_ARG, "IR mix ramp must be 0 .. 16777216 frames");
    if (!p) return fail(AIDAX_ERR_ARG, "null pool");
    if (stream != AIDAX_ALL_STREAMS && (stream < 0 || static_cast<uint32_t>(stream) >= p->n_streams))
        return fail(AIDAX_ERR_ARG, "stream out of range");
    IrPlan& plan = p->ir.plan;
    const uint32_t lo = stream == AIDAX_ALL_STREAMS ? 0u : static_cast<uint32_t>(stream), hi = stream == AIDAX_ALL_STREAMS ? p->n_streams : lo + 1u;
    for (uint32_t s = lo; s < hi; ++s) plan.set_mix(s, mix, ramp_frames);
    return AIDAX_OK;
}

AIDAX_API int aidax_pool_stream_ir_mix(const aidax_pool* p, uint32_t stream, int32_t* slot_b, float* mix_now, float* mix_target, uint32_t* frames_left)
{
    if (!p) return fail(AIDAX_ERR_ARG, "null pool");
    if (stream >= p->n_streams) return fail(AIDAX_ERR_ARG, "stream out of range");
    const IrPlan& plan = p->ir.plan;
    if (slot_b) *slot_b = plan.assign_b[stream];
    if (mix_now) *mix_now = plan.ramp[stream].now;
    if (mix_target) *mix_target = plan.ramp[stream].m1;
    if (frames_left) *frames_left = plan.frames_left(stream);
    return AIDAX_OK;
}

// Set-up side: a host record that the first prepare reads when it sizes the history ring (R >= capacity + max_frames); the kernels take
// the ring's mask and row, and every IR's diagonal count, at run time.
AIDAX_API int aidax_pool_set_ir_capacity(aidax_pool* p, uint32_t max_taps)
{
    if (max_taps < kIrMaxTaps || max_taps > AIDAX_IR_MAX_CAPACITY) return fail(AIDAX_ERR_ARG, "IR capacity must be 8192 .. 65536 taps");
    if (!p) return fail(AIDAX_ERR_ARG, "null pool");
    if (p->ir.has_history())
        return fail(AIDAX_ERR_STATE, "IR capacity is fixed once the first aidax_pool_prepare_ir / _ir_slot has allocated the history");
    p->ir.capacity.store(max_taps, std::memory_order_relaxed);
    return AIDAX_OK;
}

AIDAX_API uint32_t aidax_pool_ir_capacity(const aidax_pool* p) { return p ? p->ir.capacity.load(std::memory_order_relaxed) : 0; }

AIDAX_API int aidax_pool_stream_ir(const aidax_pool* p, uint32_t stream, int32_t* slot)
{
    if (!p || !slot) return fail(AIDAX_ERR_ARG, "null argument");
    if (stream >= p->n_streams) return fail(AIDAX_ERR_ARG, "stream out of range");
    *slot = p->ir.plan.assign[stream];
    return AIDAX_OK;
}

AIDAX_API int aidax_many_streams_form(int cell, int hidden, uint32_t n_streams, int compute_units)
{
    return static_cast<int>(many_streams_form(cell, hidden, n_streams, compute_units, 256, read_form_hooks()));
}
AIDAX_API int aidax_many_streams_form_at(int cell, int hidden, uint32_t n_streams, int compute_units, uint32_t max_frames)
{
    return static_cast<int>(many_streams_form(cell, hidden, n_streams, compute_units, max_frames, read_form_hooks()));
}

AIDAX_API int aidax_model_conv_form(const aidax_model* m)
{
    if (!m || !is_conv_model(*m)) return 0;
    ConvDesc d;
    uint32_t state_floats = 0;
    (void)pack_conv(*m, &d, &state_floats);
    if (convm_lds_bytes(d, 256) > 160 * 1024) return 1;
    return d.st_ok ? 4 : d.ms_ok ? 3 : 2;
}

// What a MODE_CHAIN pass of the pool's full block length runs, with the controls, the bank and the chained kernels' flags as they stand
AIDAX_API const char* aidax_pool_kernel_name(const aidax_pool* p) { return p ? p->playing_form(p->max_frames).name : "k_nomodel"; }

AIDAX_API int aidax_model_forward(const aidax_model* m, int device_id, const float* X, float* y, uint32_t n, int unit_gains)
{
    if (!m || !X || !y) return fail(AIDAX_ERR_ARG, "null argument");
    aidax_pool* p = nullptr;
    int rc = aidax_pool_create(1, 4, 48000.0, device_id, &p);
    if (rc != AIDAX_OK) return rc;
    rc = aidax_pool_set_model(p, m, AIDAX_START_RESET);
    if (rc == AIDAX_OK) {
        rc = guarded([&]() -> int {
            DevBuf<float> x_buf, y_buf;                         // (freed behind the wait below, ahead of the pool)
            const size_t xn = static_cast<size_t>(n) * m->input_size;
            x_buf.alloc(xn ? xn : 1);
            y_buf.alloc(n ? n : 1);
            float* d_x = x_buf.get();
            float* d_y = y_buf.get();
            HIP_TRY(hipMemcpyAsync(d_x, X, sizeof(float) * xn, hipMemcpyHostToDevice, p->q));
            hipError_t le = hipSuccess;
            const uint32_t chunk = p->launch_chunk(p->cur, n ? n : 1);
            for (uint32_t done = 0; done < n && le == hipSuccess; done += chunk) {
                LaunchArgs a = p->args(p->cur, p->d_st.get(), d_x + static_cast<size_t>(done) * m->input_size, d_y + done,
                                       std::min(chunk, n - done), MODE_NN_ONLY);
                if (unit_gains) { a.in_gain = 1.f; a.out_gain = 1.f; }
                le = p->launch(p->cur, a, p->q);
            }
            if (le == hipSuccess) {
                (void)hipMemcpyAsync(y, d_y, sizeof(float) * n, hipMemcpyDeviceToHost, p->q);
            }
            const hipError_t se = hipStreamSynchronize(p->q);
            HIP_TRY(le);
            HIP_TRY(se);
            return AIDAX_OK;
        });
    }
    aidax_pool_destroy(p);
    return rc;
}

AIDAX_API int aidax_model_self_test(const aidax_model* m, int device_id, int32_t* n_errors, float* max_error, float* out_opt)
{
    if (!m || !n_errors || !max_error) return fail(AIDAX_ERR_ARG, "null argument");
    const size_t n = m->golden_in.size();
    if (n == 0) return fail(AIDAX_ERR_STATE, "model carries no input_batch/output_batch");
    // params forced to 0, gains forced to 1 (rt-neural-generic.cpp:903-915)
    std::vector<float> X(n * static_cast<size_t>(m->input_size), 0.f);
    for (size_t t = 0; t < n; ++t) X[t * m->input_size] = m->golden_in[t];
    std::vector<float> y(n);
    const int rc = aidax_model_forward(m, device_id, X.data(), y.data(), static_cast<uint32_t>(n), 1);
    if (rc != AIDAX_OK) return rc;
    int32_t errs = 0;
    float worst = 0.f;
    for (size_t t = 0; t < n; ++t) {
        const float e = std::fabs(y[t] - m->golden_out[t]);
        if (e > worst) worst = e;
        if (static_cast<double>(e) > 1.0e-5) ++errs;          // TEST_MODEL_THR, rt-neural-generic.h:182
    }
    *n_errors = errs;
    *max_error = worst;
    if (out_opt) std::memcpy(out_opt, y.data(), n * sizeof(float));
    return AIDAX_OK;
}

}  // extern "C"
