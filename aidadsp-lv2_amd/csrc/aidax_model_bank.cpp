// aidax_model_bank.cpp — the host-only half of the model bank (aidax_model_bank.h). No HIP call: tests/asan_bank_harness.cpp runs it
// without a device.
#include <string>
#include <utility>

#include "aidax_model_bank.h"

namespace aidax {

const char* bank_arch_diff(const BankArch& a, const BankArch& b)
{
    return a.cell != b.cell ? "cell" : a.hidden != b.hidden ? "hidden" : a.input_size != b.input_size ? "input_size" : a.sr != b.sr ? "samplerate" : nullptr;
}
bool bank_table_model(const aidax_model& m) { return !is_conv_model(m) && !is_stack_model(m) && m.n_rnn == 1 && (m.cell == AIDAX_CELL_LSTM || m.cell == AIDAX_CELL_GRU); }
BankSlot bank_slot_of(const aidax_model& m)
{
    BankSlot k;
    k.loaded = true;
    k.cell = m.cell; k.hidden = m.hidden; k.input_size = m.input_size; k.input_skip = m.input_skip;
    k.in_gain = m.input_gain; k.out_gain = m.output_gain; k.model_sr = m.samplerate;
    return k;
}

int bank_may_stage(const aidax_model& m, const BankArch& pool, const char* other_kernel, bool lds_fits)
{
    if (!bank_table_model(m)) return fail(AIDAX_ERR_ARCH, "model bank: the model is not a one-layer LSTM / GRU model of the table");
    if (other_kernel) return fail(AIDAX_ERR_ARCH, std::string("model bank: the pool's model runs ") + other_kernel + " at this pool size, not a table kernel");
    if (const char* f = bank_arch_diff(pool, { m.cell, m.hidden, m.input_size, m.samplerate }))
        return fail(AIDAX_ERR_ARCH, std::string("model bank: the model differs from the pool's model in ") + f);
    if (!pool.bank_kernel) return fail(AIDAX_ERR_ARCH, "model bank: this cell has no three-wave pipeline kernel (LSTM-64 / LSTM-80)");
    if (!lds_fits) return fail(AIDAX_ERR_ARCH, "model bank: the pool's max_frames is too large for the pipeline's LDS block buffer");
    return AIDAX_OK;
}

int ModelBank::may_commit_slot(uint32_t k, const BankSlot& staged, const BankArch& pool) const
{
    if (users[k] != 0) return fail(AIDAX_ERR_STATE, "model bank slot " + std::to_string(k) + " has streams assigned: move them first");
    if (staged.loaded && (!pool.bank_kernel || bank_arch_diff(pool, { staged.cell, staged.hidden, staged.input_size, staged.model_sr })))
        return fail(AIDAX_ERR_STATE, "the pool's model changed since aidax_pool_prepare_model_slot: prepare the slot again");
    return AIDAX_OK;
}

// a pool model (or an unload) under a bank in use: the slots are variants of the model that plays
int ModelBank::may_commit_pool_model(const BankArch& next) const
{
    bool ok = n_assigned.load(std::memory_order_relaxed) == 0 && (n_loaded == 0 || next.bank_kernel);
    for (const BankSlot& k : slot)
        if (ok && k.loaded) ok = !bank_arch_diff(next, { k.cell, k.hidden, k.input_size, k.model_sr });
    if (!ok) return fail(AIDAX_ERR_STATE, "empty the model bank first (streams are assigned to it, or a loaded slot does not fit the model being committed)");
    return AIDAX_OK;
}

void ModelBank::commit_slot(uint32_t k, BankSlot& staged)
{
    std::swap(slot[k], staged);
    n_loaded += (slot[k].loaded ? 1u : 0u) - (staged.loaded ? 1u : 0u);
}

void ModelBank::assign_stream(uint32_t s, int32_t to, const ModelRec& pool_rec)
{
    const int32_t old = assign[s];
    if (old >= 0) { --users[old]; n_assigned.fetch_sub(1, std::memory_order_relaxed); }
    assign[s] = to;
    if (to >= 0) ++users[to];
    if (to >= 0 && n_assigned.fetch_add(1, std::memory_order_relaxed) == 0) {
        // the bank comes into force: the records of the streams on the pool model are written now, around the model that plays
        // (it cannot change while a stream is assigned)
        std::fill(rec.begin(), rec.end(), pool_rec);
        dirty.mark(0, static_cast<uint32_t>(rec.size()) - 1);
    }
    rec[s] = to >= 0 ? rec_of(slot[to]) : pool_rec;
    dirty.mark(s, s);
}

}  // namespace aidax

extern "C" AIDAX_API int aidax_model_bank_compatible(const aidax_model* pool_model, const aidax_model* m)
{
    using namespace aidax;
    if (!pool_model || !m) return fail(AIDAX_ERR_ARG, "null model");
    if (!bank_table_model(*pool_model)) return fail(AIDAX_ERR_ARCH, "model bank: the pool model is not a one-layer LSTM / GRU model of the table");
    if (!bank_table_model(*m)) return fail(AIDAX_ERR_ARCH, "model bank: the model is not a one-layer LSTM / GRU model of the table");
    if (const char* f = bank_arch_diff({ pool_model->cell, pool_model->hidden, pool_model->input_size, pool_model->samplerate },
                                       { m->cell, m->hidden, m->input_size, m->samplerate }))
        return fail(AIDAX_ERR_ARCH, std::string("model bank: the models differ in ") + f);
    return AIDAX_OK;
}
