// The model bank's host half under AddressSanitizer + UndefinedBehaviorSanitizer (`make asan_bank`, tests/test_asan_bank.py): ModelBank
// (aidax_model_bank.cpp: who plays which slot, the per-stream records, the commit rules) held against a direct restatement of its rules
// over seeded random slot commits, assignments, pool-model commits and flushes. CPU only: device pointers are made-up numbers.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "aidax.h"
#include "../aidadsp-lv2_amd/csrc/aidax_model_bank.h"

namespace aidax {
// (aidax_model.cpp, linked for fail() and aidax_last_error(), asks the pool which models have a kernel: no model is loaded here)
bool model_supported(const aidax_model&) { return true; }
}  // namespace aidax

static int failures = 0, steps = 0;
#define EXPECT(c) do { if (!(c)) { std::fprintf(stderr, "asan_bank_harness: %s failed at line %d (%s)\n", #c, __LINE__, aidax_last_error()); ++failures; } } while (0)

using aidax::BankArch;
using aidax::BankSlot;
using aidax::ModelBank;
using aidax::ModelRec;
constexpr int kSlots = AIDAX_MODEL_SLOTS;

static uint32_t lcg_state = 88172645u;
static uint32_t rnd(uint32_t n) { lcg_state = lcg_state * 1664525u + 1013904223u; return (lcg_state >> 8) % n; }

static bool same(const ModelRec& a, const ModelRec& b) { return std::memcmp(&a, &b, sizeof(ModelRec)) == 0; }
static bool same(const BankSlot& a, const BankSlot& b)
{
    return a.loaded == b.loaded && a.d_wpack == b.d_wpack && a.cell == b.cell && a.hidden == b.hidden && a.input_size == b.input_size &&
           a.input_skip == b.input_skip && a.in_gain == b.in_gain && a.out_gain == b.out_gain && a.model_sr == b.model_sr;
}

// content of `arch` with weights, gains and skip of its own (the pointer is never dereferenced); not loaded: the content that empties a slot
static BankSlot content(const BankArch& arch, bool loaded)
{
    static uintptr_t next = 0x10000;
    BankSlot k;
    if (!loaded) return k;
    next += 0x1000;
    k.loaded = true;
    k.d_wpack = reinterpret_cast<float*>(next);
    k.cell = arch.cell; k.hidden = arch.hidden; k.input_size = arch.input_size; k.model_sr = arch.sr;
    k.input_skip = static_cast<int>(rnd(2));
    k.in_gain = 0.25f * static_cast<float>(1 + rnd(16)); k.out_gain = -0.5f * static_cast<float>(1 + rnd(9));
    return k;
}
static BankArch other_arch(const BankArch& a, int field)
{
    BankArch o = a;
    if (field == 0) o.cell = a.cell == AIDAX_CELL_LSTM ? AIDAX_CELL_GRU : AIDAX_CELL_LSTM;
    if (field == 1) o.hidden = a.hidden + 4;
    if (field == 2) o.input_size = a.input_size % 3 + 1;
    if (field == 3) o.sr = a.sr == 48000.f ? 44100.f : 48000.f;
    return o;
}
static const char* const kField[4] = { "cell", "hidden", "input_size", "samplerate" };

// what the harness knows: the slots' contents, who plays what, the pool model's record, and the records as the device holds them
struct Want {
    std::vector<BankSlot> slot = std::vector<BankSlot>(kSlots);
    std::vector<int32_t> assign;
    ModelRec pool_rec{};
    std::vector<ModelRec> device;                         // the device copy as of the last simulated flush
};

// (the restatement's own copy of the four fields, not the product's model_rec)
static ModelRec rec_from(const BankSlot& k)
{
    ModelRec r;
    std::memset(&r, 0, sizeof r);
    r.wpack = k.d_wpack;
    r.in_gain = k.in_gain;
    r.out_gain = k.out_gain;
    r.input_skip = k.input_skip;
    return r;
}
static ModelRec want_rec(const Want& w, uint32_t s) { return w.assign[s] >= 0 ? rec_from(w.slot[w.assign[s]]) : w.pool_rec; }

static void expect_state(const ModelBank& b, const Want& w)
{
    const uint32_t n = static_cast<uint32_t>(w.assign.size());
    uint32_t sum = 0, loaded = 0;
    for (int k = 0; k < kSlots; ++k) {
        EXPECT(b.users[k] == static_cast<uint32_t>(std::count(w.assign.begin(), w.assign.end(), k)));
        EXPECT(same(b.slot[k], w.slot[k]));
        sum += b.users[k];
        loaded += w.slot[k].loaded ? 1u : 0u;
    }
    EXPECT(b.n_assigned.load() == sum && b.n_loaded == loaded);
    EXPECT(b.assign.size() == n && b.rec.size() == n && std::equal(w.assign.begin(), w.assign.end(), b.assign.begin()));
    if (sum == 0) return;                                   // the records count only while the bank is in force
    for (uint32_t s = 0; s < n; ++s) {
        EXPECT(same(b.rec[s], want_rec(w, s)));
        // what differs from the device's copy lies inside the dirty range
        if (!same(b.rec[s], w.device[s])) EXPECT(!b.dirty.empty() && b.dirty.lo <= s && s <= b.dirty.hi);
    }
    EXPECT(b.dirty.empty() || (b.dirty.lo <= b.dirty.hi && b.dirty.hi < n));
}

// a frozen copy of every field, for "a refusal changes nothing"
struct Frozen {
    std::vector<BankSlot> slot; std::vector<uint32_t> users; uint32_t n_loaded, n_assigned; std::vector<int32_t> assign; std::vector<ModelRec> rec;
    uint32_t lo, hi;
    explicit Frozen(const ModelBank& b)
        : slot(b.slot, b.slot + kSlots), users(b.users, b.users + kSlots), n_loaded(b.n_loaded), n_assigned(b.n_assigned.load()), assign(b.assign),
          rec(b.rec), lo(b.dirty.lo), hi(b.dirty.hi) {}
    bool holds(const ModelBank& b) const
    {
        bool ok = std::equal(users.begin(), users.end(), b.users) && n_loaded == b.n_loaded && n_assigned == b.n_assigned.load() && assign == b.assign &&
                  lo == b.dirty.lo && hi == b.dirty.hi && rec.size() == b.rec.size();
        for (int k = 0; ok && k < kSlots; ++k) ok = same(slot[k], b.slot[k]);
        for (size_t s = 0; ok && s < rec.size(); ++s) ok = same(rec[s], b.rec[s]);
        return ok;
    }
};

static bool refused(int rc, const char* text) { return rc == AIDAX_ERR_STATE && std::strstr(aidax_last_error(), text) != nullptr; }

static void run(uint32_t n, uint32_t seed, int n_steps)
{
    lcg_state = seed;
    ModelBank b(n);
    Want w;
    w.assign.assign(n, AIDAX_MODEL_POOL);
    w.device.assign(n, ModelRec{});
    BankArch arch{ AIDAX_CELL_LSTM, 16, 1, 48000.f };
    BankSlot pool_model = content(arch, true);
    w.pool_rec = rec_from(pool_model);
    expect_state(b, w);
    const uint32_t keys[] = { 0, 1, 5, 63 };
    for (int step = 0; step < n_steps; ++step, ++steps) {
        const uint32_t op = rnd(16);
        const Frozen before(b);
        if (op < 4) {                                                           // a slot commit: load, replace or empty
            const uint32_t k = keys[rnd(4)];
            BankSlot sg = content(arch, rnd(4) != 0);
            const BankSlot staged = sg;
            const int rc = b.may_commit_slot(k, sg, arch);
            if (std::count(w.assign.begin(), w.assign.end(), static_cast<int32_t>(k)) != 0) {
                EXPECT(refused(rc, ("model bank slot " + std::to_string(k) + " has streams assigned").c_str()) && before.holds(b));
            } else {
                EXPECT(rc == AIDAX_OK);
                b.commit_slot(k, sg);
                EXPECT(same(sg, w.slot[k]));                                    // what is to be freed: the slot's content until now
                w.slot[k] = staged;
            }
        } else if (op == 4) {                                                   // content of another architecture, in each of the four fields; no bankable pool model
            const uint32_t k = keys[rnd(4)];
            if (std::count(w.assign.begin(), w.assign.end(), static_cast<int32_t>(k)) == 0) {
                for (int f = 0; f < 4; ++f) {
                    const BankSlot sg = content(other_arch(arch, f), true);
                    EXPECT(refused(b.may_commit_slot(k, sg, arch), "the pool's model changed since aidax_pool_prepare_model_slot") && before.holds(b));
                    EXPECT(std::string(aidax::bank_arch_diff(arch, { sg.cell, sg.hidden, sg.input_size, sg.model_sr })) == kField[f]);
                }
                BankArch none = arch;                                           // a pool model without a bank kernel (or no pool model)
                none.bank_kernel = false;
                EXPECT(refused(b.may_commit_slot(k, content(arch, true), none), "the pool's model changed") && before.holds(b));
                EXPECT(b.may_commit_slot(k, content(arch, false), none) == AIDAX_OK && before.holds(b));      // emptying needs no pool model
            }
        } else if (op < 12) {                                                   // an assignment (to a loaded slot or back to the pool model)
            const uint32_t s = rnd(n), k = keys[rnd(4)];
            const int32_t to = rnd(3) == 0 || !w.slot[k].loaded ? AIDAX_MODEL_POOL : static_cast<int32_t>(k);
            const bool comes_into_force = to >= 0 && std::count(w.assign.begin(), w.assign.end(), AIDAX_MODEL_POOL) == static_cast<long>(n);
            b.assign_stream(s, to, w.pool_rec);
            w.assign[s] = to;
            if (comes_into_force) EXPECT(b.dirty.lo == 0 && b.dirty.hi == n - 1);
            EXPECT(!b.dirty.empty() && b.dirty.lo <= s && s <= b.dirty.hi);
        } else if (op < 14) {                                                   // a pool-model commit: refused, or another model of the architecture
            const bool assigned = std::count(w.assign.begin(), w.assign.end(), AIDAX_MODEL_POOL) != static_cast<long>(n);
            const bool any_loaded = std::any_of(w.slot.begin(), w.slot.end(), [](const BankSlot& k) { return k.loaded; });
            const char* text = "empty the model bank first";
            for (int f = 0; f < 4; ++f) {
                const BankArch o = other_arch(arch, f);
                const int rc = b.may_commit_pool_model(o);
                EXPECT((assigned || any_loaded ? refused(rc, text) : rc == AIDAX_OK) && before.holds(b));
            }
            BankArch none = arch;                                               // an unload, or a model without a bank kernel
            none.bank_kernel = false;
            EXPECT((assigned || any_loaded ? refused(b.may_commit_pool_model(none), text) : b.may_commit_pool_model(none) == AIDAX_OK) && before.holds(b));
            const int rc = b.may_commit_pool_model(arch);
            EXPECT((assigned ? refused(rc, text) : rc == AIDAX_OK) && before.holds(b));
            if (!assigned) {
                if (!any_loaded && rnd(2)) arch = other_arch(arch, static_cast<int>(rnd(4)));      // an empty bank takes any architecture
                pool_model = content(arch, true);
                w.pool_rec = rec_from(pool_model);
            }
        } else {                                                                // a flush, as ModelBankStage::flush does it while the bank is in force
            if (b.n_assigned.load() != 0 && !b.dirty.empty()) {
                std::copy(b.rec.begin() + b.dirty.lo, b.rec.begin() + b.dirty.hi + 1, w.device.begin() + b.dirty.lo);
                b.dirty.clear();
            }
        }
        expect_state(b, w);
    }
}

int main()
{
    for (uint32_t n : { 1u, 5u, 64u, 70u })
        for (uint32_t seed : { 1u, 77u, 2024u }) run(n, seed * 2654435761u + n, 400);
    std::printf("asan_bank_harness: %d steps, %d failures\n", steps, failures);
    return failures ? 1 : 0;
}
