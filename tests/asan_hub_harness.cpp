// The hub's host half under AddressSanitizer + UndefinedBehaviorSanitizer (`make asan_hub`, tests/test_asan_hub.py): HubBook
// (aidax_hub_book.h: who is attached and has submitted, the rotating buffers and the pass each holds, the pass that carried a seat's latest
// block, when a period is closed early, what a failed launch drops, which passes a k_mfma_lp give-up condemns) played the way
// aidax_hub.cpp plays it, against a plain restatement: per pass the set of (seat, block number) it carried, per seat the list of blocks it
// submitted, and a "GPU" that has finished the passes up to some id. Literal rows first, for the cases the code's comments name, then
// seeded random scripts over hubs of 1, 3 and 70 seats. After every step:
//   1. a seat is handed the row of exactly the pass that carried its previous block, at that block's length, or silence — never another
//      pass's row and never one from the buffer being collected into;
//   2. cur == (launches + 1) % kHubBuffers, and a buffer whose pass the GPU has not finished is never staged into without its guard raised;
//   3. n_submitted and n_attached are the counts of their flags; hi_slot never falls and covers every attached seat;
//   4. after a failed launch no seat is marked submitted, launches is unchanged and those seats' next read is silence;
//   5. a pass in [bad_from, bad_upto] is never delivered, nor one that did give up; clean_upto never falls (and names finished passes only);
//      bad_upto <= min(launches, last_chained); every report condemns at least one pass or bumps faults_unmapped;
//   6. the book allocates nothing after init (a counting global operator new). CPU only.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <new>
#include <utility>
#include <vector>

#include "../aidadsp-lv2_amd/csrc/aidax_hub_book.h"

static uint64_t g_news = 0;
void* operator new(std::size_t n)
{
    ++g_news;
    if (void* p = std::malloc(n ? n : 1)) return p;
    throw std::bad_alloc();
}
void operator delete(void* p) noexcept { std::free(p); }
void operator delete(void* p, std::size_t) noexcept { std::free(p); }

static int failures = 0, steps = 0;
#define EXPECT(c) do { if (!(c)) { std::fprintf(stderr, "asan_hub_harness: %s failed at line %d\n", #c, __LINE__); ++failures; } } while (0)

using aidax::HubBook;
using aidax::kHubBuffers;

static uint32_t lcg_state = 88172645u;
static uint32_t rnd(uint32_t n) { lcg_state = lcg_state * 1664525u + 1013904223u; return (lcg_state >> 8) % n; }

struct Quiet {                                   // a call into the book allocates nothing
    uint64_t n = g_news;
    ~Quiet() { EXPECT(g_news == n); }
};

static const uint32_t kLens[] = { 64, 32, 0 };
enum Closer { LAUNCHER, SETTER, API };
enum Fail { GOOD, FAIL_PARK, FAIL_LAUNCH };

struct Sim {
    HubBook b;
    // the restatement
    struct Pass { uint32_t frames; bool chained, gave_up; std::vector<std::pair<uint32_t, uint32_t>> carried; };
    struct Read { bool open; int buf; uint64_t pass; uint32_t frames, block; };
    uint32_t cap;
    std::vector<uint8_t> att, sub, pool_parked;
    std::vector<std::vector<uint32_t>> blocks;   // per seat: the length of every block it submitted
    std::vector<uint64_t> carrier;               // per seat: the pass that carried its latest block (0: none did)
    std::vector<Read> reads;                     // per seat: a run() that has submitted and not yet taken its output
    std::vector<Pass> pass;                      // [id]; [0] is nobody's
    uint64_t gpu_done = 0;                       // the GPU has finished the passes up to this id
    uint32_t period_frames = 0, hi_seen = 0;
    uint64_t clean_seen = 0, deadline_closes = 0;
    bool word = false, lp_off = false;           // a give-up report waits to be taken; the pool has fallen back (no chained pass from here on)
    int launcher_error = 0;
    uint32_t fail_one_in = 0;                    // a period that run() closes itself fails to launch once in so many (0: never)
    // what the last submit / resolve answered (the literal rows look at them)
    int last_prev_buf = -1;
    uint64_t last_prev_pass = 0;
    HubBook::Verdict last_verdict = HubBook::SILENCE;

    explicit Sim(uint32_t seats) : cap(seats), att(seats, 0), sub(seats, 0), pool_parked(seats, 0), blocks(seats), carrier(seats, 0), reads(seats, Read{}), pass(1, Pass{})
    {
        b.init(seats);
        for (uint32_t s = 0; s < seats; ++s) {   // aidax_hub_create: nobody is attached yet, every stream rests disabled
            Quiet q;
            pool_parked[s] = 1;
            b.parked(s, true);
        }
        check();
    }
    uint64_t launches() const { return pass.size() - 1; }
    uint32_t count(const std::vector<uint8_t>& v) const { return static_cast<uint32_t>(std::count(v.begin(), v.end(), 1)); }
    uint64_t held(int buf) const                 // the pass whose rows buffer `buf` holds: the latest one with that residue
    {
        for (uint64_t id = launches(); id >= 1 && id + kHubBuffers > launches(); --id)
            if (static_cast<int>(id % kHubBuffers) == buf) return id;
        return 0;
    }
    uint64_t last_chained() const
    {
        for (uint64_t id = launches(); id >= 1; --id)
            if (pass[id].chained) return id;
        return 0;
    }

    void check()
    {
        ++steps;
        const uint64_t L = launches();
        EXPECT(b.launches == L && b.cur == static_cast<int>((L + 1) % kHubBuffers));
        EXPECT(b.n_attached == count(att) && b.n_submitted == count(sub) && b.deadline_launches == deadline_closes);
        EXPECT(b.hi_slot >= hi_seen && b.hi_slot <= cap);
        hi_seen = b.hi_slot;
        for (uint32_t s = 0; s < cap; ++s) {
            EXPECT(b.attached[s] == att[s] && b.submitted[s] == sub[s] && (b.forced_off[s] != 0) == (pool_parked[s] != 0));
            EXPECT(!att[s] || s < b.hi_slot);
            EXPECT(!sub[s] || att[s]);
            if (att[s]) EXPECT(b.last_pass[s] == carrier[s]);
            EXPECT(b.seated(static_cast<int32_t>(s)) == (att[s] != 0));
        }
        EXPECT(!b.seated(-1) && !b.seated(static_cast<int32_t>(cap)));
        for (int i = 0; i < kHubBuffers; ++i) {
            const uint64_t id = held(i);
            EXPECT(b.pass_id[i] == id && (id == 0 || b.out_frames[i] == pass[id].frames));
        }
        const uint64_t staged = held(b.cur);     // (2) the buffer being collected into
        if (staged > gpu_done) EXPECT(b.guard[b.cur]);
        EXPECT(b.clean_upto >= clean_seen && b.clean_upto <= gpu_done);
        clean_seen = b.clean_upto;
        EXPECT(b.last_chained == last_chained() && b.bad_upto <= std::min(L, b.last_chained));
        if (L) EXPECT(b.latency == pass[L].frames);
    }

    int attach()
    {
        int32_t want = -1;
        for (uint32_t s = 0; s < cap && want < 0; ++s)
            if (!att[s]) want = static_cast<int32_t>(s);
        int32_t s;
        { Quiet q; s = b.free_seat(); }
        EXPECT(s == want);
        if (s >= 0) {
            { Quiet q; b.attach(static_cast<uint32_t>(s)); }
            att[s] = 1;
            carrier[s] = 0;
        }
        check();
        return s;
    }
    void detach(uint32_t s)
    {
        resolve(s);
        att[s] = 0;
        sub[s] = 0;                              // its submission is taken back: no pass carries that block
        bool complete;
        { Quiet q; complete = b.detach(s); }
        EXPECT(complete == (count(sub) != 0 && count(sub) == count(att)));
        if (complete) close(API, GOOD);
        else check();
    }

    // flush_locked + launch_period; false: the period could not be launched
    bool close(Closer who, Fail how, bool chained = false)
    {
        if (who == LAUNCHER && !b.flush_requested) {
            if (count(sub) == 0) return true;    // (the launcher is not timed without a submission)
            ++deadline_closes;
            ++b.deadline_launches;
        }
        bool any;
        { Quiet q; any = b.begin_flush(); }
        EXPECT(any == (count(sub) != 0) && !b.flush_requested);
        if (!any) { check(); return true; }
        const uint64_t L = launches();
        const uint32_t stop_at = how == FAIL_PARK ? rnd(b.hi_slot + 1) : b.hi_slot;
        bool failed = how == FAIL_LAUNCH;
        for (uint32_t s = 0; s < b.hi_slot && !failed; ++s) {
            bool off = false, change;
            { Quiet q; change = b.park_change(s, &off); }
            EXPECT(off == (!att[s] || !sub[s]) && change == (off != (pool_parked[s] != 0)));
            if (!change) continue;
            if (s >= stop_at) { failed = true; break; }      // pool_park_stream failed: the book is not told
            pool_parked[s] = off;
            { Quiet q; b.parked(s, off); }
        }
        if (failed) {                            // (4)
            { Quiet q; b.dropped(); }
            for (uint32_t s = 0; s < cap; ++s)
                if (sub[s]) { sub[s] = 0; carrier[s] = 0; }
            if (who == LAUNCHER) { launcher_error = -3; b.last_error = -3; }
            EXPECT(b.n_submitted == 0 && b.launches == L);
            check();
            return false;
        }
        for (uint32_t s = 0; s < cap; ++s) EXPECT((pool_parked[s] != 0) == (!att[s] || !sub[s]));
        Pass p{ period_frames, chained && !lp_off, false, {} };
        EXPECT(b.period_frames == period_frames);
        for (uint32_t s = 0; s < cap; ++s)
            if (sub[s]) {
                p.carried.emplace_back(s, static_cast<uint32_t>(blocks[s].size() - 1));
                EXPECT(blocks[s].back() == period_frames);
                carrier[s] = L + 1;
                sub[s] = 0;
            }
        int next;
        bool before;
        { Quiet q; next = b.next_staging(); before = b.staged_before(next); }
        EXPECT(next == static_cast<int>((L + 2) % kHubBuffers) && before == (held(next) != 0));
        const bool busy = before && held(next) > gpu_done;   // the caller's event query
        const bool is_chained = p.chained;
        pass.push_back(std::move(p));
        { Quiet q; b.passed(is_chained, busy); }
        EXPECT(b.guard[b.cur] == busy);
        check();
        return true;
    }

    // aidax_hub_run up to the point where it leaves the first lock; false: it returned an error ahead of submitting
    bool submit(uint32_t s, uint32_t n, bool defer = false)
    {
        resolve(s);
        if (b.last_error != 0) {                 // a pass the launcher could not issue
            int rc;
            { Quiet q; rc = b.take_error(); }
            EXPECT(rc == launcher_error && b.last_error == 0);
            launcher_error = 0;
            check();
            return false;
        }
        bool must;
        { Quiet q; must = b.must_close(s, n); }
        EXPECT(must == (sub[s] || (count(sub) != 0 && n != period_frames)));
        if (must && !close(API, fail_one_in && rnd(fail_one_in) == 0 ? FAIL_LAUNCH : GOOD, rnd(3) == 0)) return false;
        if (b.guard[b.cur]) {                    // the wait for the buffer's previous pass, outside the lock
            gpu_done = std::max(gpu_done, held(b.cur));
            b.guard[b.cur] = false;
        }
        EXPECT(held(b.cur) <= gpu_done);         // (2) the rows staged there have left for the device
        const bool first = count(sub) == 0;
        if (first) period_frames = n;
        const uint64_t e = carrier[s], L = launches();
        // its previous block's row is readable for kHubBuffers - 2 further passes: not once its buffer is collected into again
        const bool readable = n != 0 && e != 0 && pass[e].frames == n && L - e <= static_cast<uint64_t>(kHubBuffers - 2);
        blocks[s].push_back(n);
        sub[s] = 1;
        HubBook::Submitted r;
        { Quiet q; r = b.submit(s, n); }
        EXPECT(r.first == first && r.complete == (count(sub) == count(att)));
        EXPECT(!r.complete || b.flush_requested);
        EXPECT((r.prev_buf >= 0) == readable);
        if (r.prev_buf >= 0) {                   // (1)
            EXPECT(r.prev_pass == e && r.prev_buf == static_cast<int>(e % kHubBuffers) && r.prev_buf != b.cur && held(r.prev_buf) == e);
            const auto& c = pass[e].carried;
            EXPECT(std::find(c.begin(), c.end(), std::make_pair(s, static_cast<uint32_t>(blocks[s].size() - 2))) != c.end());
        }
        last_prev_buf = r.prev_buf;
        last_prev_pass = r.prev_pass;
        reads[s] = Read{ true, r.prev_buf, r.prev_pass, n, static_cast<uint32_t>(blocks[s].size() - 1) };
        check();
        if (!defer) resolve(s);
        return true;
    }

    void take_word()                             // pool_take_lp_fault answered true
    {
        const uint64_t unmapped = b.faults_unmapped, clean = b.clean_upto;
        { Quiet q; b.gave_up(); }
        word = false;
        EXPECT(b.bad_from == clean + 1 && b.bad_upto <= std::min(launches(), last_chained()));
        EXPECT((b.bad_upto >= b.bad_from) != (b.faults_unmapped == unmapped + 1) && b.faults_unmapped <= unmapped + 1);      // (5)
        for (uint64_t id = clean + 1; id <= launches(); ++id)
            if (pass[id].gave_up) EXPECT(id >= b.bad_from && id <= b.bad_upto);
    }
    // ... and the rest of it: the wait for the previous block's pass, the second lock, the verdict
    void resolve(uint32_t s)
    {
        Read& r = reads[s];
        if (!r.open) return;
        r.open = false;
        if (r.frames == 0) return;
        if (r.buf >= 0) gpu_done = std::max(gpu_done, r.pass);
        if (word) take_word();
        last_verdict = HubBook::SILENCE;
        if (r.buf >= 0) {
            const bool condemned = r.pass >= b.bad_from && r.pass <= b.bad_upto;
            HubBook::Verdict v;
            { Quiet q; v = b.verdict(r.pass, r.buf); }
            EXPECT((v == HubBook::FAULT) == condemned);
            if (v == HubBook::DELIVER) {         // (1), (5)
                EXPECT(held(r.buf) == r.pass && !pass[r.pass].gave_up && pass[r.pass].frames == r.frames);
                const auto& c = pass[r.pass].carried;
                EXPECT(std::find(c.begin(), c.end(), std::make_pair(s, r.block - 1)) != c.end());
            }
            if (v == HubBook::SILENCE) EXPECT(held(r.buf) != r.pass);      // the buffer was reused while the seat waited
            if (v != HubBook::FAULT) EXPECT(b.clean_upto >= r.pass);
            last_verdict = v;
        }
        check();
    }

    void gpu_behind(uint64_t k) { gpu_done = std::max(gpu_done, launches() > k ? launches() - k : 0); check(); }
    // some chained pass that the GPU has not run yet gives up (the GPU runs up to it); none outstanding: only a report (`spurious`)
    void give_up(bool spurious)
    {
        std::vector<uint64_t> out;
        for (uint64_t id = gpu_done + 1; id <= launches(); ++id)
            if (pass[id].chained) out.push_back(id);
        if (!out.empty() && !spurious) {
            const uint64_t f = out[rnd(static_cast<uint32_t>(out.size()))];
            pass[f].gave_up = true;
            gpu_done = f;
            word = true;
            lp_off = true;
        } else if (spurious) {
            word = true;
        }
        check();
    }
    void finish()
    {
        for (uint32_t s = 0; s < cap; ++s) resolve(s);
    }
};

// the cases the comments of aidax_hub.cpp and aidax_hub_book.h name
static void literal_rows()
{
    {   // a seat that re-enters before its period closed: it closes the period itself, the other seat is parked for that pass
        Sim m(3);
        EXPECT(m.attach() == 0 && m.attach() == 1);
        EXPECT(m.submit(0, 64) && m.b.launches == 0);
        EXPECT(m.submit(0, 64) && m.b.launches == 1 && m.pass[1].carried.size() == 1 && m.pool_parked[1] == 1 && m.pool_parked[0] == 0);
        EXPECT(m.last_prev_buf == 1 && m.last_prev_pass == 1 && m.last_verdict == HubBook::DELIVER);
    }
    {   // a block-length change mid-period closes the period at the old length; the new length starts the next one
        Sim m(3);
        m.attach(); m.attach();
        EXPECT(m.submit(0, 64) && m.submit(1, 32));
        EXPECT(m.b.launches == 1 && m.pass[1].frames == 64 && m.b.period_frames == 32 && m.b.n_submitted == 1 && m.b.submitted[1] == 1);
        EXPECT(m.submit(0, 32) && m.b.flush_requested && m.last_prev_buf == -1);      // (its last block was 64 frames long: silence)
        EXPECT(m.close(LAUNCHER, GOOD) && m.b.launches == 2 && m.b.deadline_launches == 0);
    }
    {   // a deadline that splits a period in two, then three pieces: a seat's previous block is not in the most recent buffer
        Sim m(3);
        m.attach(); m.attach(); m.attach();
        for (uint32_t s = 0; s < 3; ++s) EXPECT(m.submit(s, 64) && m.close(LAUNCHER, GOOD));      // three pieces
        EXPECT(m.b.launches == 3 && m.b.deadline_launches == 3);
        EXPECT(m.submit(0, 64) && m.last_prev_pass == 1 && m.last_prev_buf == 1 && m.last_verdict == HubBook::DELIVER);
        EXPECT(m.close(LAUNCHER, GOOD) && m.b.launches == 4);                        // two pieces this time: {0}, {1, 2}
        EXPECT(m.submit(1, 64) && m.last_prev_pass == 2 && m.last_verdict == HubBook::DELIVER);
        EXPECT(m.submit(2, 64) && m.last_prev_pass == 3 && m.last_verdict == HubBook::DELIVER);
        EXPECT(m.close(LAUNCHER, GOOD) && m.b.launches == 5 && m.b.deadline_launches == 5 && m.pass[5].carried.size() == 2);
        // a seat whose read waits while kHubBuffers further pieces close finds its buffer reused: silence, not the later pass's row
        EXPECT(m.submit(0, 64, true) && m.last_prev_pass == 4);
        for (int i = 0; i < kHubBuffers; ++i) EXPECT(m.submit(1, 64) && m.close(API, GOOD));
        m.resolve(0);
        EXPECT(m.last_verdict == HubBook::SILENCE);
    }
    {   // a host that closes kHubBuffers periods before the first has run: the buffer it comes back to is guarded
        Sim m(1);
        m.attach();
        for (int i = 1; i <= kHubBuffers; ++i) {
            EXPECT(!m.b.guard[m.b.cur]);
            EXPECT(m.submit(0, 64, true) && m.close(LAUNCHER, GOOD) && m.b.launches == static_cast<uint64_t>(i) && m.gpu_done == 0);
            m.reads[0].open = false;             // (a host that does not even wait for its output)
        }
        EXPECT(m.b.cur == 1 && m.b.guard[1] && m.b.pass_id[1] == 1);
        EXPECT(m.submit(0, 64) && m.gpu_done >= 1 && !m.b.guard[1]);
    }
    {   // detach of the last missing seat closes the period
        Sim m(3);
        m.attach(); m.attach();
        EXPECT(m.submit(0, 64) && m.b.launches == 0);
        m.detach(1);
        EXPECT(m.b.launches == 1 && m.b.n_attached == 1 && m.pass[1].carried.size() == 1);
        m.attach();
        m.detach(1);                             // nobody has submitted: nothing to close
        EXPECT(m.b.launches == 1);
    }
    {   // a failed launch followed by a good one
        Sim m(1);
        m.attach();
        EXPECT(m.submit(0, 64) && m.close(LAUNCHER, GOOD));
        EXPECT(m.submit(0, 64) && m.last_verdict == HubBook::DELIVER && !m.close(LAUNCHER, FAIL_LAUNCH));
        EXPECT(m.b.launches == 1 && m.b.n_submitted == 0 && m.b.last_error != 0);
        EXPECT(!m.submit(0, 64) && m.b.last_error == 0);                             // the error is reported by its next run() ...
        EXPECT(m.submit(0, 64) && m.last_prev_buf == -1);                            // ... and the dropped block reads as silence
        EXPECT(m.close(LAUNCHER, GOOD) && m.b.launches == 2);
        EXPECT(m.submit(0, 64) && m.last_prev_pass == 2 && m.last_verdict == HubBook::DELIVER);
    }
    {   // a give-up with last_chained behind clean_upto: counted, nothing silenced
        Sim m(1);
        m.attach();
        EXPECT(m.submit(0, 64) && m.close(LAUNCHER, GOOD, true));
        EXPECT(m.submit(0, 64) && m.close(LAUNCHER, GOOD) && m.submit(0, 64) && m.close(LAUNCHER, GOOD));
        EXPECT(m.b.last_chained == 1 && m.b.clean_upto == 2 && m.b.launches == 3);
        m.give_up(true);
        EXPECT(m.submit(0, 64) && m.last_verdict == HubBook::DELIVER && m.b.faults_unmapped == 1 && m.b.bad_from == 3 && m.b.bad_upto == 1);
    }
    {   // a give-up in a chained pass: that pass and the chained ones behind it read as silence with a fault, the later plain ones play
        Sim m(1);
        m.attach();
        EXPECT(m.submit(0, 64) && m.close(LAUNCHER, GOOD, true));
        m.give_up(false);
        EXPECT(m.pass[1].gave_up && m.submit(0, 64) && m.last_verdict == HubBook::FAULT && m.b.faults_unmapped == 0 && m.b.clean_upto == 0);
        EXPECT(m.close(LAUNCHER, GOOD, true) && !m.pass[2].chained);
        EXPECT(m.submit(0, 64) && m.last_verdict == HubBook::DELIVER && m.b.clean_upto == 2);
    }
}

static void run(uint32_t seats, uint32_t seed, int n_steps, bool spurious)
{
    lcg_state = seed;
    Sim m(seats);
    m.fail_one_in = 16;
    const uint32_t first = 1u + rnd(seats);
    for (uint32_t i = 0; i < first; ++i) m.attach();
    for (int step = 0; step < n_steps; ++step) {
        const uint32_t op = rnd(32), s = rnd(seats);
        if (op < 2) {
            m.attach();
        } else if (op < 4) {
            if (m.att[s]) m.detach(s);
        } else if (op < 20) {
            // mostly the period's length; a seat that is skipped, comes back early or changes the length now and then
            if (m.att[s]) m.submit(s, rnd(8) == 0 ? kLens[rnd(3)] : kLens[(seed >> 4) % 2u], rnd(4) == 0);
        } else if (op < 24) {                    // the launcher: the period is complete, or its deadline has passed
            m.close(LAUNCHER, rnd(12) == 0 ? (rnd(2) ? FAIL_PARK : FAIL_LAUNCH) : GOOD, rnd(2) == 0);
        } else if (op < 26) {                    // a setter on a seat that has submitted closes the period first
            if (m.att[s]) {
                bool must;
                { Quiet q; must = m.b.must_close(s); }
                EXPECT(must == (m.sub[s] != 0));
                if (must) m.close(SETTER, rnd(12) == 0 ? FAIL_LAUNCH : GOOD, rnd(2) == 0);
            }
        } else if (op < 29) {
            m.gpu_behind(rnd(kHubBuffers + 3));
        } else if (op < 31) {
            m.give_up(spurious);
        } else if (m.att[s]) {
            m.resolve(s);
        }
    }
    m.finish();
}

int main()
{
    literal_rows();
    for (uint32_t seats : { 1u, 3u, 70u })
        for (uint32_t k = 0; k < 24; ++k)
            run(seats, 2654435761u * (k + 1u) + seats, seats == 70u ? 400 : 250, k % 3u == 2u);
    std::printf("asan_hub_harness: %d steps, %d failures\n", steps, failures);
    return failures ? 1 : 0;
}
