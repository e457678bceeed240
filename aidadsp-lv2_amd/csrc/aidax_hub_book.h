// aidax_hub_book.h — the hub's host-only half: which seats are attached and have submitted, which of the rotating buffers is collected
// into and which pass each one holds, which pass carried a seat's latest block, when a period must be closed early, what a failed launch
// drops and which passes a k_mfma_lp give-up condemns. No HIP, no threads, no locks, no clocks: plain facts in, plain facts out. Every
// member is called with the hub's mutex held (aidax_hub.cpp: the device half, which does the waits, the copies and the pool calls that the
// answers require). Sized once by init(): no later call allocates. tests/asan_hub_harness.cpp plays it against a restatement on the CPU.
#pragma once

#include <algorithm>
#include <cstdint>
#include <vector>

#include "../../include/aidax.h"

namespace aidax {

// Staging buffers in rotation. One pass per period needs two (collect into one while the other's output is read); the
// deadline may close a period in pieces (a host whose submissions span more than the deadline), and then an
// instance's output of the last period sits in the buffer of the piece IT was part of, not in the most recent one —
// so every slot remembers the pass that carried its last block, and a buffer is reused only kHubBuffers passes later
// (its output stays readable for kHubBuffers - 2 further passes: not while it is being collected into again).
constexpr int kHubBuffers = 4;

struct HubBook {
    uint32_t cap = 0;
    std::vector<uint8_t> attached, submitted, forced_off;
    std::vector<uint64_t> last_pass;             // per slot: id of the pass that carried its latest block (0: none)
    std::vector<aidax_controls> ctl;             // what each instance set (the hub fills in the defaults)
    uint32_t n_attached = 0, n_submitted = 0, period_frames = 0, out_frames[kHubBuffers] = {};
    uint64_t pass_id[kHubBuffers] = {};          // which pass a buffer holds
    bool guard[kHubBuffers] = {};                // the buffer's previous pass may still be reading its input staging: whoever
                                                 // stages into it next waits for that pass first — outside the lock (aidax_hub_run)
    int cur = 1;                                 // the buffer being collected into: always (id of the next pass) % kHubBuffers
    uint32_t hi_slot = 0;                        // rows [0, hi_slot) can be attached: what a pass moves and launches
    uint32_t latency = 0;
    uint64_t launches = 0, deadline_launches = 0;
    uint64_t last_chained = 0;                   // the latest pass that went out on a chained kernel (k_mfma_lp / k_mfma_ls): later ones cannot have given up
    uint64_t clean_upto = 0;                     // passes up to this id are known to carry no k_mfma_lp give-up
    uint64_t faults_unmapped = 0;                // give-up reports that mapped to no chained pass (nothing to silence; counted so that none vanishes)
    uint64_t bad_from = 1, bad_upto = 0;         // passes in [bad_from, bad_upto] may have given up: their rows are delivered as silence
    int last_error = AIDAX_OK;                   // a pass the launcher could not issue, until a run() reports it
    bool flush_requested = false;                // the period is complete: the launcher closes it

    void init(uint32_t seats)
    {
        cap = seats;
        attached.assign(seats, 0);
        submitted.assign(seats, 0);
        forced_off.assign(seats, 0);
        last_pass.assign(seats, 0);
        ctl.resize(seats);
    }

    bool seated(int32_t slot) const { return slot >= 0 && static_cast<uint32_t>(slot) < cap && attached[slot] != 0; }
    int32_t free_seat() const
    {
        for (uint32_t s = 0; s < cap; ++s)
            if (!attached[s]) return static_cast<int32_t>(s);
        return -1;
    }
    bool complete() const { return n_submitted != 0 && n_submitted == n_attached; }
    void attach(uint32_t s)
    {
        attached[s] = 1;
        last_pass[s] = 0;
        ++n_attached;
        if (s + 1 > hi_slot) hi_slot = s + 1;
    }
    // a seat leaves and takes its submission back; true: everybody who is left has submitted, the period is closed now
    bool detach(uint32_t s)
    {
        attached[s] = 0;
        --n_attached;
        if (submitted[s]) { submitted[s] = 0; --n_submitted; }
        return complete();
    }

    // Must the period being collected be closed before ...
    // ... a setter changes what the seat plays under: the block it has submitted was played under what was in force
    bool must_close(uint32_t s) const { return submitted[s] != 0; }
    // ... the seat submits a block: it is back before the period was closed (somebody was skipped and the launcher has not got to it
    // yet), or the host changed the block size
    bool must_close(uint32_t s, uint32_t n_frames) const { return submitted[s] != 0 || (n_submitted != 0 && n_frames != period_frames); }

    struct Submitted {
        bool first;          // of a new period: the caller sets the period's deadline
        bool complete;       // every attached seat has submitted (flush_requested is raised)
        int prev_buf;        // the buffer that holds the seat's previous block at this length, -1: none (silence)
        uint64_t prev_pass;  // ... and the pass that carried it
    };
    // the seat's block of n_frames goes into buffer `cur` (the caller has copied or will copy the row, under the same lock)
    Submitted submit(uint32_t s, uint32_t n_frames)
    {
        Submitted r{ n_submitted == 0, false, -1, 0 };
        if (r.first) period_frames = n_frames;
        submitted[s] = 1;
        ++n_submitted;
        // the pass that carried this instance's previous block, if its buffer has not been reused since
        // (not from the buffer being collected into: the pass that closes this period will write its results there)
        const uint64_t lp = last_pass[s];
        const int pb = static_cast<int>(lp % kHubBuffers);
        if (n_frames != 0 && lp != 0 && pb != cur && pass_id[pb] == lp && out_frames[pb] == n_frames) {
            r.prev_buf = pb;
            r.prev_pass = lp;
        }
        r.complete = n_submitted == n_attached;
        if (r.complete) flush_requested = true;
        return r;
    }

    // Somebody closes the period: false when nothing has been submitted (no pass)
    bool begin_flush()
    {
        flush_requested = false;
        return n_submitted != 0;
    }
    // A slot that is detached, or did not take part in the period being launched, is parked for that pass (a parked stream is a raw copy:
    // its state does not move). True when row s < hi_slot has to change; the caller parks it in the pool and, on success, says parked().
    bool park_change(uint32_t s, bool* off) const
    {
        *off = !attached[s] || !submitted[s];
        return *off != (forced_off[s] != 0);
    }
    void parked(uint32_t s, bool off) { forced_off[s] = off ? 1 : 0; }
    // the buffer that is collected into once the pass being launched is out, and whether a pass has ever staged from it
    int next_staging() const { return static_cast<int>((launches + 2) % kHubBuffers); }
    bool staged_before(int b) const { return pass_id[b] != 0; }
    // The period's pass has been issued from buffer `cur`. chained: it went out on a chained kernel. next_staging_busy: the pass that last
    // used next_staging() has not finished (the caller's event query). That buffer was the staging of the pass kHubBuffers back: its rows
    // must have left for the device before the instances overwrite them. A host that closes several short periods in a row (block-size
    // changes, skipped instances) can run that far ahead of the GPU — found by tests/soak_hub.py as outputs computed from a later block's
    // input. Normally that pass is long complete; otherwise the buffer is marked and the first run() that stages into it waits.
    void passed(bool chained, bool next_staging_busy)
    {
        const int b = cur;
        ++launches;
        if (chained) last_chained = launches;
        out_frames[b] = period_frames;
        pass_id[b] = launches;
        for (uint32_t s = 0; s < hi_slot; ++s)
            if (submitted[s]) last_pass[s] = launches;
        clear_submissions();
        latency = period_frames;
        cur = static_cast<int>((launches + 1) % kHubBuffers);
        guard[cur] = pass_id[cur] != 0 && next_staging_busy;
    }
    void clear_submissions()
    {
        std::fill(submitted.begin(), submitted.end(), 0);
        n_submitted = 0;
    }
    // A period that could not be launched: nobody finds the same failing period waiting again, and its instances read silence for it — no
    // pass carried their block, so the pass of the block before it (whose row they have had) is forgotten
    void dropped()
    {
        for (uint32_t s = 0; s < hi_slot; ++s)
            if (submitted[s]) last_pass[s] = 0;
        clear_submissions();
    }
    int take_error()
    {
        const int rc = last_error;
        last_error = AIDAX_OK;
        return rc;
    }

    // The pool reports a k_mfma_lp give-up: some pass in (clean_upto, launches] gave up a layer hand-over, and only one that ran on a
    // chained kernel can have. (A report that maps to no pass still counts: aidax_hub_faults_unmapped.)
    void gave_up()
    {
        bad_from = clean_upto + 1;
        bad_upto = std::min(launches, last_chained);
        if (bad_upto < bad_from) ++faults_unmapped;
    }
    enum Verdict { DELIVER, SILENCE, FAULT };    // FAULT: silence, and the call reports the give-up
    // The event of prev_pass (submit()'s answer) has passed: may its row in prev_buf be handed out? Not if the pass is condemned, and not if
    // the buffer has been reused while the caller waited. A pass that is not condemned is clean: nothing was reported by the time it ended.
    Verdict verdict(uint64_t prev_pass, int prev_buf)
    {
        if (prev_pass >= bad_from && prev_pass <= bad_upto) return FAULT;
        if (prev_pass > clean_upto) clean_upto = prev_pass;
        return pass_id[prev_buf] == prev_pass ? DELIVER : SILENCE;
    }
};

}  // namespace aidax
