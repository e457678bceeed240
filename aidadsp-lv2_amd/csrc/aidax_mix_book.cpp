// aidax_mix_book.cpp — the mix buses' host half (aidax_mix_stage.h: MixBook) and aidax_mix_gain, the pure function behind a ramp
// frame's gain. Host logic only: no HIP call in here.
#include <hip/hip_runtime_api.h>

#include <cmath>

#include "aidax_mix_stage.h"

namespace aidax {

void MixBook::init(uint32_t streams, uint32_t buses)
{
    n_streams = streams;
    n_buses = buses;
    sends.assign(static_cast<size_t>(streams) * AIDAX_SENDS, Send{});
    bus_start.assign(static_cast<size_t>(buses) + 1u, 0u);
    entries.assign(static_cast<size_t>(streams) * AIDAX_SENDS, MixEntry{});
    n_entries = max_entries = since_build = n_unsettled = moving_left = 0;
    moving_hi = -1;
    dirty = true;
}

void MixBook::set(uint32_t stream, uint32_t send, int32_t bus, float gain, uint32_t len)
{
    Send& x = at(stream, send);
    const bool was = unsettled(x);
    x.bus = bus;
    x.g0 = gain_now(x);                                            // (another bus, or none: from 0, a new send fades in)
    x.g1 = bus == AIDAX_BUS_NONE ? 0.f : gain + 0.f;               // (-0 is 0)
    x.len = len;
    x.k = 0;
    if (x.g0 == x.g1) x.len = 0, x.k = 1;                          // between equal gains a ramp has ended when it is set
    n_unsettled += static_cast<uint32_t>(unsettled(x)) - static_cast<uint32_t>(was);
    dirty = true;
}

void MixBook::rebuild()
{
    // a counting sort by bus that keeps the (stream, send) order: the counts, their running sum, then every entry into its bus's next place
    std::fill(bus_start.begin(), bus_start.end(), 0u);
    for (const Send& x : sends)
        if (x.bus != AIDAX_BUS_NONE) ++bus_start[static_cast<size_t>(x.bus) + 1u];
    max_entries = 0;
    for (uint32_t b = 0; b < n_buses; ++b) {
        max_entries = std::max(max_entries, bus_start[b + 1u]);
        bus_start[b + 1u] += bus_start[b];
    }
    n_entries = bus_start[n_buses];
    moving_hi = -1;
    moving_left = 0;
    for (uint32_t s = 0; s < n_streams; ++s)
        for (uint32_t j = 0; j < AIDAX_SENDS; ++j) {
            const Send& x = at(s, j);
            if (x.bus == AIDAX_BUS_NONE) continue;
            entries[bus_start[x.bus]++] = MixEntry{ s, x.g0, x.g1, x.len, x.k };
            if (frames_left(x) != 0) moving_hi = s, moving_left = std::max(moving_left, frames_left(x));
        }
    // (every bus's start now stands at its end, the next bus's start: shift them back)
    for (uint32_t b = n_buses; b > 0; --b) bus_start[b] = bus_start[b - 1u];
    bus_start[0] = 0;
    since_build = 0;
    dirty = false;
}

void MixBook::advance(uint32_t n_active, uint32_t n_frames)
{
    if (n_frames == 0) return;
    // A prefix pass: the streams it left out are where they were, while since_build moves on for every entry. An entry at rest does
    // not mind (behind its ramp's end it carries g1 at any offset); one that may still be moving needs the plan rebuilt. Once
    // moving_left frames have been issued since the rebuild, every ramp the plan holds has ended (a prefix pass before that has
    // forced a rebuild), and a prefix pass uploads nothing.
    if (moving_hi >= static_cast<int64_t>(n_active) && since_build < moving_left) dirty = true;
    since_build = std::min(since_build + n_frames, kMixMaxRampOffset);
    if (n_unsettled == 0) return;
    for (uint32_t s = 0; s < n_active; ++s)
        for (uint32_t j = 0; j < AIDAX_SENDS; ++j) {
            Send& x = at(s, j);
            if (!unsettled(x)) continue;
            x.played_bus = x.bus;
            x.k += std::min(n_frames, frames_left(x));
            x.now = x.bus == AIDAX_BUS_NONE ? 0.f : static_cast<float>(ramp_value(x.g0, x.g1, x.len, x.k - 1u));
            if (!unsettled(x)) --n_unsettled;
        }
}

size_t MixBook::serialise(uint8_t* snapshot) const
{
    std::memcpy(snapshot, bus_start.data(), entries_off());
    std::memcpy(snapshot + entries_off(), entries.data(), sizeof(MixEntry) * n_entries);
    return entries_off() + sizeof(MixEntry) * n_entries;
}

}  // namespace aidax

using namespace aidax;

extern "C" {

AIDAX_API int aidax_mix_gain(float g0, float g1, uint32_t ramp_frames, uint32_t k, float* gain)
{
    if (!gain) return fail(AIDAX_ERR_ARG, "null gain");
    if (!std::isfinite(g0) || !std::isfinite(g1) || std::fabs(g0) > AIDAX_MIX_MAX_GAIN || std::fabs(g1) > AIDAX_MIX_MAX_GAIN)
        return fail(AIDAX_ERR_ARG, "a send's gain is finite and at most 16 in magnitude");
    if (ramp_frames > kIrMaxRamp) return fail(AIDAX_ERR_ARG, "ramp_frames exceeds 2^24");
    *gain = k >= ramp_frames ? g1 : static_cast<float>(ramp_value(g0, g1, ramp_frames, k));      // (k + 1 does not wrap)
    return AIDAX_OK;
}

}  // extern "C"
