// aidax_model_bank.h — the model bank of a pool (include/aidax.h, "Per-stream amp models"): weight variants of the pool model's
// architecture, one per slot, and per stream the slot it plays. ModelBank is the host-only half (aidax_model_bank.cpp, no HIP call),
// ModelBankStage the device half around it. Issues HIP calls: include it last.
#pragma once

#include <atomic>
#include <memory>
#include <vector>

#include "aidax_snapshot_ring.h"

namespace aidax {

// A slot's content: what a table model's prepare uploads (pack_weights) plus the file's three scalars; the architecture fields are kept
// for the re-checks at commit time. The host half never dereferences d_wpack.
struct BankSlot {
    bool loaded = false;
    float* d_wpack = nullptr;
    int cell = 0, hidden = 0, input_size = 0, input_skip = 0;
    float in_gain = 1.f, out_gain = 1.f, model_sr = 48000.f;
};
// what two models must share to sit in one bank (bank_arch_diff: the first field that differs, or nullptr); bank_kernel: a pool model runs a kernel with a k_*_pipe_bank partner
struct BankArch { int cell, hidden, input_size; float sr; bool bank_kernel = true; };
const char* bank_arch_diff(const BankArch& a, const BankArch& b);
bool bank_table_model(const aidax_model& m);
BankSlot bank_slot_of(const aidax_model& m);             // loaded, its weights not uploaded yet
// may m be staged for a slot of a pool whose model is `pool`? other_kernel: what that model runs where it is no table kernel (else
// nullptr); lds_fits: the pipeline's block buffer holds the pool's max_frames. AIDAX_OK or the refusal through fail()
int bank_may_stage(const aidax_model& m, const BankArch& pool, const char* other_kernel, bool lds_fits);

// what the kernels read of a stream's model, and the same into launch arguments built for another model of the architecture
inline ModelRec model_rec(const float* w, float in_gain, float out_gain, int32_t skip) { ModelRec r{}; r.wpack = w; r.in_gain = in_gain; r.out_gain = out_gain; r.input_skip = skip; return r; }
inline void apply_model_rec(LaunchArgs& a, const ModelRec& r) { a.wpack = r.wpack; a.in_gain = r.in_gain; a.out_gain = r.out_gain; a.input_skip = r.input_skip; }

// The per-stream records are valid while a stream is assigned to a slot — the assignment that makes the first one rewrites them all —
// and `dirty` is what of them the device has not seen. All of it is the audio side's; n_assigned is read by other threads too.
struct ModelBank {
    BankSlot slot[AIDAX_MODEL_SLOTS];
    uint32_t users[AIDAX_MODEL_SLOTS] = {};              // streams assigned to each slot
    uint32_t n_loaded = 0;
    std::atomic<uint32_t> n_assigned{0};                 // streams on any slot
    std::vector<int32_t> assign;                         // per stream: AIDAX_MODEL_POOL or a slot
    std::vector<ModelRec> rec;
    DirtyRange dirty;

    explicit ModelBank(uint32_t n_streams) : assign(n_streams, AIDAX_MODEL_POOL), rec(n_streams) {}
    static ModelRec rec_of(const BankSlot& k) { return model_rec(k.d_wpack, k.in_gain, k.out_gain, k.input_skip); }
    // The commit rules, AIDAX_OK or the refusal through fail(): may `staged` become slot k's content under the pool model `pool`, and
    // may `next` (bank_kernel false also for an unload) become the pool model under this bank?
    int may_commit_slot(uint32_t k, const BankSlot& staged, const BankArch& pool) const;
    int may_commit_pool_model(const BankArch& next) const;
    void commit_slot(uint32_t k, BankSlot& staged);      // `staged` becomes slot k's content and gets back what is to be freed
    void assign_stream(uint32_t s, int32_t slot, const ModelRec& pool_rec);      // s plays `slot`, or the pool model (whose record is pool_rec)
};

// The device half: the host half, the records' device copy and the snapshots they leave from, allocated by the first prepare (worker
// side) and published ONCE; the audio side picks it up through adopt() and owns flush. HIP failures leave as HipFail.
class ModelBankStage {
    struct Shared {
        ModelBank host;
        DevBuf<ModelRec> d_rec;
        SnapshotRing ring;
        explicit Shared(uint32_t n) : host(n) {}
        ~Shared() { for (BankSlot& k : host.slot) DevBuf<float>::adopt(k.d_wpack); }      // (the slots' weights: BankSlot is a record of the host half)
    };
    std::atomic<Shared*> pub_{nullptr};

  public:
    ModelBank* adopt() const { Shared* b = pub_.load(std::memory_order_acquire); return b ? &b->host : nullptr; }
    // is a stream assigned to a bank slot? Then every MODE_CHAIN pass is one launch of k_*_pipe_bank over the per-stream records
    ModelBank* in_force() const { ModelBank* b = adopt(); return b && b->n_assigned.load(std::memory_order_relaxed) != 0 ? b : nullptr; }
    // worker side: slot content from model m (nullptr: the content that empties a slot), its pack_floats weights uploaded on wq; on
    // first use the bank itself, so that no audio-side call ever allocates; wq waited for
    void prepare(uint32_t n_streams, const aidax_model* m, size_t pack_floats, BankSlot& k, hipStream_t wq)
    {
        std::vector<float> wpack;
        if (m) {
            wpack = pack_weights(*m);
            if (wpack.size() != pack_floats) throw std::runtime_error("weight pack size mismatch");
            k = bank_slot_of(*m);
            DevBuf<float> w;
            w.alloc(wpack.size());
            k.d_wpack = w.release();                      // (the staged object's from here: staged_release)
            HIP_TRY(hipMemcpyAsync(k.d_wpack, wpack.data(), wpack.size() * sizeof(float), hipMemcpyHostToDevice, wq));
        }
        if (!adopt()) {
            auto nb = std::make_unique<Shared>(n_streams);
            nb->d_rec.alloc(n_streams);
            HIP_TRY(hipMemsetAsync(nb->d_rec.get(), 0, sizeof(ModelRec) * n_streams, wq));
            nb->ring.alloc(sizeof(ModelRec) * n_streams);
            HIP_TRY(hipStreamSynchronize(wq));
            pub_.store(nb.release(), std::memory_order_release);
        }
        HIP_TRY(hipStreamSynchronize(wq));                // `wpack` is pageable; the audio side must find the slot complete
    }
    // ahead of a pass of a bank in force: the changed records, stream-ordered with it; returns the device records
    const ModelRec* flush(hipStream_t s)
    {
        Shared* b = pub_.load(std::memory_order_acquire);
        b->ring.upload_dirty(b->d_rec.get(), b->host.rec.data(), b->host.dirty, s);
        return b->d_rec.get();
    }
    ~ModelBankStage() { delete pub_.exchange(nullptr); }
};

}  // namespace aidax
