// aidax_pool_stages.cpp — the C ABI of a pool's opt-in stages (aidax_pool.h): the stream meters, the noise gate, the stream tuners, the
// mix buses, the bus limiters, the bus reverbs and the stream delays, from aidax_pool_set_metering to aidax_pool_reset_delay. Every call
// tests its arguments in an order of its own, which callers see in the code and text it fails with (tests/fuzz_abi.py and
// tests/test_abi_host.py hold them), then does one of a few things: it changes host records of the audio side, or one of the moves
// written once below: the set-up side's first enable of a stage, a restart of the streams that went from off to on, a read of a span of
// records that waits. Where in a pass the stages run is pool_process_prefix's business (aidax_pool.cpp).
#include <hip/hip_runtime_api.h>

#include "aidax_pool.h"

// the records [first, first + count) that a read names lie within the n there are, and are at least one
static bool in_span(uint32_t first, uint32_t count, uint32_t n) { return count != 0 && first <= n && count <= n - first; }

// The first call that switches a stage on is the set-up side's: `enable` allocates (and waits), all or nothing
template <class Enable>
static int first_enable(aidax_pool* p, Enable&& enable)
{
    return guarded([&]() -> int {
        HIP_TRY(hipSetDevice(p->device));
        enable();
        return AIDAX_OK;
    });
}

// The runs of streams that a change took from off to on restart: `clear(first, count)` zeroes their device state on the pool's own stream,
// behind every pass issued so far (the next pass, on whatever stream, is ordered behind that). No run: no HIP call.
template <class Clear>
static int restart_runs(aidax_pool* p, const std::vector<Run>& runs, Clear&& clear)
{
    if (runs.empty()) return AIDAX_OK;
    return p->on_own_stream([&]() -> int {
        for (const Run& r : runs) clear(r.first, r.second - r.first);
        return AIDAX_OK;
    });
}

extern "C" {

// The stream meters and the noise gate (aidax_stream_stages.h). The first call that switches either on is the set-up side's (it
// allocates); every later call changes host records of the audio side. A stream whose gate goes from off to on has its state zeroed on
// the pool's own stream, behind every pass issued so far (the next pass, on whatever stream, is ordered behind that).
AIDAX_API int aidax_pool_set_metering(aidax_pool* p, int on)
{
    if (!p) return fail(AIDAX_ERR_ARG, "null pool");
    if (!on || p->meter.enabled()) {
        p->meter.on = on != 0;
        return AIDAX_OK;
    }
    return first_enable(p, [&] { p->meter.enable(p->n_streams, p->q); });
}

AIDAX_API int aidax_pool_metering(const aidax_pool* p) { return p && p->meter.on ? 1 : 0; }

// Audio side, waits: the copy (and the clear behind it) enters the pool's own stream behind every pass issued so far, whatever stream carried it
AIDAX_API int aidax_pool_read_meters(aidax_pool* p, uint32_t first, uint32_t count, aidax_stream_meter* out, int clear)
{
    if (!p || !out) return fail(AIDAX_ERR_ARG, "null argument");
    if (!in_span(first, count, p->n_streams)) return fail(AIDAX_ERR_ARG, "stream range out of the pool's streams");
    if (!p->meter.enabled()) return fail(AIDAX_ERR_STATE, "metering was never enabled (aidax_pool_set_metering)");
    return p->on_own_stream([&]() -> int { p->meter.read(first, count, out, clear != 0, p->q); return AIDAX_OK; });
}

AIDAX_API int aidax_pool_set_gate(aidax_pool* p, int32_t stream, const aidax_gate_params* params)
{
    if (!p) return fail(AIDAX_ERR_ARG, "null pool");
    uint32_t lo = 0, hi = 0;
    if (!named_range(stream, p->n_streams, &lo, &hi)) return fail(AIDAX_ERR_ARG, "stream out of range");
    aidax_gate_rec designed{};
    if (params)
        if (const int rc = aidax_gate_design(params, aidax_pool_samplerate(p), &designed)) return rc;
    GateStage& g = p->gate;
    if (!g.enabled()) {
        if (!params) return AIDAX_OK;                       // (off before any on: nothing to change)
        if (const int rc = first_enable(p, [&] { g.enable(p->n_streams, p->max_frames, p->q); })) return rc;
    }
    return restart_runs(p, g.set(lo, hi, params ? &designed : nullptr, params), [&](uint32_t first, uint32_t count) { g.clear_states(first, count, p->q); });
}

AIDAX_API int aidax_pool_stream_gate(const aidax_pool* p, uint32_t stream, aidax_gate_params* out, int* on)
{
    if (!p) return fail(AIDAX_ERR_ARG, "null pool");
    if (stream >= p->n_streams) return fail(AIDAX_ERR_ARG, "stream out of range");
    const GateStage& g = p->gate;
    if (out) *out = g.enabled() ? g.book.params[stream] : aidax_gate_params{};
    if (on) *on = g.enabled() && g.book.h_rec[stream].on ? 1 : 0;
    return AIDAX_OK;
}

// Audio side, waits: the copy enters the pool's own stream behind every pass issued so far, whatever stream carried it
AIDAX_API int aidax_pool_read_gate(aidax_pool* p, uint32_t first, uint32_t count, aidax_gate_state* out)
{
    if (!p || !out) return fail(AIDAX_ERR_ARG, "null argument");
    if (!in_span(first, count, p->n_streams)) return fail(AIDAX_ERR_ARG, "stream range out of the pool's streams");
    if (!p->gate.enabled()) return fail(AIDAX_ERR_STATE, "no gate was ever enabled (aidax_pool_set_gate)");
    return p->on_own_stream([&]() -> int { p->gate.read(first, count, out, p->q); return AIDAX_OK; });
}

// The stream tuners (aidax_stream_stages.h: TunerStage). The first aidax_pool_set_tuning with parameters is the set-up side's (it
// allocates and fixes the design); everything else changes or reads host records of the audio side, and the reads wait like
// aidax_pool_read_meters. A stream whose tuner goes from off to on has its count, reading and curve zeroed on the pool's own stream.
AIDAX_API int aidax_pool_set_tuning(aidax_pool* p, const aidax_tuner_params* params)
{
    if (!p) return fail(AIDAX_ERR_ARG, "null pool");
    TunerStage& t = p->tuner;
    if (!params) { t.on = false; return AIDAX_OK; }
    aidax_tuner_rec designed{};
    if (const int rc = aidax_tuner_design(aidax_pool_samplerate(p), params, &designed)) return rc;
    if (t.enabled()) {
        if (std::memcmp(&designed, &t.book.rec, sizeof designed) != 0) return fail(AIDAX_ERR_STATE, "the pool's tuner design is fixed once set");
        t.on = true;
        return AIDAX_OK;
    }
    return first_enable(p, [&] { t.enable(p->n_streams, p->max_frames, designed, p->q); });
}

AIDAX_API int aidax_pool_tuning(const aidax_pool* p, aidax_tuner_rec* out)
{
    if (out) *out = p && p->tuner.enabled() ? p->tuner.book.rec : aidax_tuner_rec{};
    return p && p->tuner.on ? 1 : 0;
}

AIDAX_API int aidax_pool_set_tuner(aidax_pool* p, int32_t stream, int on)
{
    if (!p) return fail(AIDAX_ERR_ARG, "null pool");
    uint32_t lo = 0, hi = 0;
    if (!named_range(stream, p->n_streams, &lo, &hi)) return fail(AIDAX_ERR_ARG, "stream out of range");
    TunerStage& t = p->tuner;
    if (!t.enabled()) return fail(AIDAX_ERR_STATE, "the tuners were never set up (aidax_pool_set_tuning)");
    return restart_runs(p, t.book.apply(lo, hi, on != 0), [&](uint32_t first, uint32_t count) { t.clear_streams(first, count, p->q); });
}

AIDAX_API int aidax_pool_stream_tuner(const aidax_pool* p, uint32_t stream, int* on, uint64_t* pos)
{
    if (!p) return fail(AIDAX_ERR_ARG, "null pool");
    if (stream >= p->n_streams) return fail(AIDAX_ERR_ARG, "stream out of range");
    const TunerStage& t = p->tuner;
    if (on) *on = t.enabled() && t.book.h_on[stream] ? 1 : 0;
    if (pos) *pos = t.enabled() ? t.book.pos[stream] : 0u;
    return AIDAX_OK;
}

AIDAX_API int aidax_pool_read_tuners(aidax_pool* p, uint32_t first, uint32_t count, aidax_tuner_reading* out)
{
    if (!p || !out) return fail(AIDAX_ERR_ARG, "null argument");
    if (!in_span(first, count, p->n_streams)) return fail(AIDAX_ERR_ARG, "stream range out of the pool's streams");
    if (!p->tuner.enabled()) return fail(AIDAX_ERR_STATE, "the tuners were never set up (aidax_pool_set_tuning)");
    return p->on_own_stream([&]() -> int { p->tuner.read(first, count, out, p->q); return AIDAX_OK; });
}

AIDAX_API int aidax_pool_read_tuner_curve(aidax_pool* p, uint32_t stream, float* out, uint32_t count)
{
    if (!p || !out) return fail(AIDAX_ERR_ARG, "null argument");
    if (stream >= p->n_streams) return fail(AIDAX_ERR_ARG, "stream out of range");
    if (!p->tuner.enabled()) return fail(AIDAX_ERR_STATE, "the tuners were never set up (aidax_pool_set_tuning)");
    if (count == 0 || count > p->tuner.curve_row) return fail(AIDAX_ERR_ARG, "the curve has lags 0 .. tmax + 1");
    return p->on_own_stream([&]() -> int { p->tuner.read_curve(stream, out, count, p->q); return AIDAX_OK; });
}

// The mix buses (aidax_mix_stage.h). The first aidax_pool_set_buses with a count is the set-up side's (it allocates); everything else
// changes or reads host records of the audio side, and the reads of the bus block wait like aidax_pool_read_meters.
AIDAX_API int aidax_pool_set_buses(aidax_pool* p, uint32_t n_buses)
{
    if (!p) return fail(AIDAX_ERR_ARG, "null pool");
    if (n_buses > AIDAX_MAX_BUSES) return fail(AIDAX_ERR_ARG, "more than 4096 buses");
    MixStage& m = p->mix;
    if (n_buses == 0 || m.enabled()) {
        if (n_buses != 0 && n_buses != m.book.n_buses) return fail(AIDAX_ERR_STATE, "the pool's bus count is fixed once set");
        m.on = n_buses != 0;                                // (off before any on: nothing to change)
        return AIDAX_OK;
    }
    return first_enable(p, [&] { m.enable(p->n_streams, p->max_frames, n_buses, p->q); });
}

AIDAX_API uint32_t aidax_pool_buses(const aidax_pool* p) { return p ? p->mix.book.n_buses : 0; }

AIDAX_API int aidax_pool_set_send(aidax_pool* p, int32_t stream, uint32_t send, int32_t bus, float gain, uint32_t ramp_frames)
{
    if (!p) return fail(AIDAX_ERR_ARG, "null pool");
    uint32_t lo = 0, hi = 0;
    if (!named_range(stream, p->n_streams, &lo, &hi)) return fail(AIDAX_ERR_ARG, "stream out of range");
    if (send >= AIDAX_SENDS) return fail(AIDAX_ERR_ARG, "send out of range");
    float checked = 0.f;
    if (const int rc = aidax_mix_gain(0.f, gain, ramp_frames, 0, &checked)) return rc;      // (the gain and the ramp length, by the one rule)
    MixBook& b = p->mix.book;
    if (!p->mix.enabled()) return fail(AIDAX_ERR_STATE, "the pool has no buses (aidax_pool_set_buses)");
    if (bus != AIDAX_BUS_NONE && (bus < 0 || static_cast<uint32_t>(bus) >= b.n_buses)) return fail(AIDAX_ERR_ARG, "bus out of range");
    for (uint32_t s = lo; s < hi; ++s) b.set(s, send, bus, gain, ramp_frames);
    return AIDAX_OK;
}

AIDAX_API int aidax_pool_stream_send(const aidax_pool* p, uint32_t stream, uint32_t send, int32_t* bus, float* gain_now, float* gain_target, uint32_t* frames_left)
{
    if (!p) return fail(AIDAX_ERR_ARG, "null pool");
    if (stream >= p->n_streams) return fail(AIDAX_ERR_ARG, "stream out of range");
    if (send >= AIDAX_SENDS) return fail(AIDAX_ERR_ARG, "send out of range");
    const MixBook::Send x = p->mix.enabled() ? p->mix.book.at(stream, send) : MixBook::Send{};
    if (bus) *bus = x.bus;
    if (gain_now) *gain_now = MixBook::gain_now(x);
    if (gain_target) *gain_target = x.g1;
    if (frames_left) *frames_left = MixBook::frames_left(x);
    return AIDAX_OK;
}

AIDAX_API int aidax_pool_read_buses(aidax_pool* p, uint32_t first, uint32_t count, float* out, size_t cap_floats, uint32_t* n_frames)
{
    if (!p || !out) return fail(AIDAX_ERR_ARG, "null argument");
    MixStage& m = p->mix;
    if (!m.enabled()) return fail(AIDAX_ERR_STATE, "the pool has no buses (aidax_pool_set_buses)");
    if (!in_span(first, count, m.book.n_buses)) return fail(AIDAX_ERR_ARG, "bus range out of the pool's buses");
    if (static_cast<size_t>(count) * m.last_frames > cap_floats) return fail(AIDAX_ERR_ARG, "buffer too small for the rows at the last pass's n_frames");
    if (n_frames) *n_frames = m.last_frames;
    return p->on_own_stream([&]() -> int { m.read(first, count, out, p->q); return AIDAX_OK; });
}

AIDAX_API int aidax_pool_buses_device(aidax_pool* p, float** d_ptr)
{
    if (!p || !d_ptr) return fail(AIDAX_ERR_ARG, "null argument");
    if (!p->mix.enabled()) return fail(AIDAX_ERR_STATE, "the pool has no buses (aidax_pool_set_buses)");
    *d_ptr = p->mix.d_bus.get();
    return AIDAX_OK;
}

// The bus limiters and bus meters (aidax_limit_stage.h). The first aidax_pool_set_bus_limiting with on != 0 is the set-up side's (it
// allocates); everything else changes or reads host records of the audio side, and the read of the meters waits like aidax_pool_read_meters.
AIDAX_API int aidax_pool_set_bus_limiting(aidax_pool* p, int on, uint32_t max_lookahead_frames, uint32_t max_hold_frames)
{
    if (!p) return fail(AIDAX_ERR_ARG, "null pool");
    if (!p->mix.enabled()) return fail(AIDAX_ERR_STATE, "the pool has no buses (aidax_pool_set_buses)");
    LimitStage& l = p->limit;
    if (!on) {
        l.on = false;                                       // (off before any on: nothing to change)
        return AIDAX_OK;
    }
    if (max_lookahead_frames < 1u || max_lookahead_frames > AIDAX_BUS_LOOKAHEAD_MAX || max_hold_frames > AIDAX_BUS_HOLD_MAX)
        return fail(AIDAX_ERR_ARG, "the look-ahead capacity is 1 .. 512 frames, the hold capacity at most 4096");
    if (l.enabled()) {
        if (max_lookahead_frames != l.book.max_lookahead || max_hold_frames != l.book.max_hold) return fail(AIDAX_ERR_STATE, "the bus limiters' capacities are fixed once set");
        l.on = true;
        return AIDAX_OK;
    }
    return first_enable(p, [&] { l.enable(p->mix.book.n_buses, p->max_frames, max_lookahead_frames, max_hold_frames, p->q); });
}

AIDAX_API int aidax_pool_bus_limiting(const aidax_pool* p) { return p && p->limit.on ? 1 : 0; }

AIDAX_API int aidax_pool_set_bus_limiter(aidax_pool* p, int32_t bus, const aidax_bus_limit_params* params)
{
    if (!p) return fail(AIDAX_ERR_ARG, "null pool");
    LimitStage& l = p->limit;
    if (!l.enabled()) return fail(AIDAX_ERR_STATE, "bus limiting was never enabled (aidax_pool_set_bus_limiting)");
    uint32_t lo = 0, hi = 0;
    if (!named_range(bus, l.book.n_buses, &lo, &hi)) return fail(AIDAX_ERR_ARG, "bus out of range");
    aidax_bus_limit_rec designed{};
    if (params)
        if (const int rc = aidax_bus_limit_design(params, aidax_pool_samplerate(p), &designed)) return rc;
    if (!l.book.set(lo, hi, params ? &designed : nullptr, params)) return fail(AIDAX_ERR_ARG, "the limiter's look-ahead or hold exceeds the capacities of aidax_pool_set_bus_limiting");
    return AIDAX_OK;
}

AIDAX_API int aidax_pool_bus_limiter(const aidax_pool* p, uint32_t bus, aidax_bus_limit_params* out, int* on, uint32_t* latency_frames)
{
    if (!p) return fail(AIDAX_ERR_ARG, "null pool");
    if (bus >= p->mix.book.n_buses) return fail(AIDAX_ERR_ARG, "bus out of range");
    const LimitStage& l = p->limit;
    const bool is_on = l.enabled() && l.book.h_rec[bus].on;
    if (out) *out = is_on ? l.book.params[bus] : aidax_bus_limit_params{};
    if (on) *on = is_on ? 1 : 0;
    if (latency_frames) *latency_frames = l.enabled() ? l.book.latency(bus) : 0u;
    return AIDAX_OK;
}

AIDAX_API int aidax_pool_read_bus_meters(aidax_pool* p, uint32_t first, uint32_t count, aidax_bus_meter* out, int clear)
{
    if (!p || !out) return fail(AIDAX_ERR_ARG, "null argument");
    LimitStage& l = p->limit;
    if (!l.enabled()) return fail(AIDAX_ERR_STATE, "bus limiting was never enabled (aidax_pool_set_bus_limiting)");
    if (!in_span(first, count, l.book.n_buses)) return fail(AIDAX_ERR_ARG, "bus range out of the pool's buses");
    return p->on_own_stream([&]() -> int { l.read(first, count, out, clear != 0, p->q); return AIDAX_OK; });
}

// The bus reverbs (aidax_reverb_stage.h). The first aidax_pool_set_bus_reverbs with on != 0 is the set-up side's (it allocates);
// everything else changes or reads host records of the audio side.
AIDAX_API int aidax_pool_set_bus_reverbs(aidax_pool* p, int on, uint32_t max_delay_frames)
{
    if (!p) return fail(AIDAX_ERR_ARG, "null pool");
    if (!p->mix.enabled()) return fail(AIDAX_ERR_STATE, "the pool has no buses (aidax_pool_set_buses)");
    ReverbStage& r = p->reverb;
    if (!on) {
        r.on = false;                                       // (off before any on: nothing to change)
        return AIDAX_OK;
    }
    if (max_delay_frames < AIDAX_BUS_REVERB_MIN_DELAY || max_delay_frames > AIDAX_BUS_REVERB_MAX_DELAY)
        return fail(AIDAX_ERR_ARG, "the bus reverbs' delay capacity is 64 .. 32768 frames");
    if (r.enabled()) {
        if (max_delay_frames != r.book.max_delay) return fail(AIDAX_ERR_STATE, "the bus reverbs' delay capacity is fixed once set");
        r.on = true;
        return AIDAX_OK;
    }
    return first_enable(p, [&] { r.enable(p->mix.book.n_buses, p->max_frames, max_delay_frames, p->q); });
}

AIDAX_API int aidax_pool_bus_reverbs(const aidax_pool* p) { return p && p->reverb.on ? 1 : 0; }

// the range of buses a call names, or an error
static int reverb_buses(aidax_pool* p, int32_t bus, uint32_t* lo, uint32_t* hi)
{
    if (!p) return fail(AIDAX_ERR_ARG, "null pool");
    const ReverbStage& r = p->reverb;
    if (!r.enabled()) return fail(AIDAX_ERR_STATE, "the bus reverbs were never enabled (aidax_pool_set_bus_reverbs)");
    return named_range(bus, r.book.n_buses, lo, hi) ? AIDAX_OK : fail(AIDAX_ERR_ARG, "bus out of range");
}

AIDAX_API int aidax_pool_set_bus_reverb(aidax_pool* p, int32_t bus, const aidax_bus_reverb_params* params)
{
    uint32_t lo = 0, hi = 0;
    if (const int rc = reverb_buses(p, bus, &lo, &hi)) return rc;
    aidax_bus_reverb_rec designed{};
    if (params)
        if (const int rc = aidax_bus_reverb_design(params, aidax_pool_samplerate(p), &designed)) return rc;
    if (!p->reverb.book.set(lo, hi, params ? &designed : nullptr, params)) return fail(AIDAX_ERR_ARG, "a delay of the reverb exceeds the capacity of aidax_pool_set_bus_reverbs");
    return AIDAX_OK;
}

AIDAX_API int aidax_pool_set_bus_reverb_rec(aidax_pool* p, int32_t bus, const aidax_bus_reverb_rec* rec)
{
    uint32_t lo = 0, hi = 0;
    if (const int rc = reverb_buses(p, bus, &lo, &hi)) return rc;
    if (rec && !ReverbBook::valid(*rec)) return fail(AIDAX_ERR_ARG, "bus reverb record: delays 64 .. 32768, 0 <= gq < 1/sqrt(8), 0 <= a <= 0.5, wet and dry finite and at most 4 in magnitude");
    if (!p->reverb.book.set(lo, hi, rec, nullptr)) return fail(AIDAX_ERR_ARG, "a delay of the reverb exceeds the capacity of aidax_pool_set_bus_reverbs");
    return AIDAX_OK;
}

AIDAX_API int aidax_pool_bus_reverb(const aidax_pool* p, uint32_t bus, aidax_bus_reverb_params* params, aidax_bus_reverb_rec* rec, int* on, uint64_t* frames_since_epoch)
{
    if (!p) return fail(AIDAX_ERR_ARG, "null pool");
    if (bus >= p->mix.book.n_buses) return fail(AIDAX_ERR_ARG, "bus out of range");
    const ReverbStage& r = p->reverb;
    const bool is_on = r.enabled() && r.book.h_rec[bus].on;
    if (params) *params = is_on ? r.book.params[bus] : aidax_bus_reverb_params{};
    if (rec) {
        *rec = aidax_bus_reverb_rec{};
        if (is_on) std::memcpy(rec, &r.book.h_rec[bus], sizeof *rec);
    }
    if (on) *on = is_on ? 1 : 0;
    if (frames_since_epoch) *frames_since_epoch = is_on ? r.book.since_epoch(bus) : 0u;
    return AIDAX_OK;
}

AIDAX_API int aidax_pool_reset_bus_reverb(aidax_pool* p, int32_t bus)
{
    uint32_t lo = 0, hi = 0;
    if (const int rc = reverb_buses(p, bus, &lo, &hi)) return rc;
    p->reverb.book.reset(lo, hi);
    return AIDAX_OK;
}

// The stream delays (aidax_delay_stage.h). The first aidax_pool_set_delays with on != 0 is the set-up side's (it allocates); everything
// else changes or reads host records of the audio side, a restart is a memset on the pool's own stream behind every pass issued so far,
// and the read of the states waits like aidax_pool_read_gate.
AIDAX_API int aidax_pool_set_delays(aidax_pool* p, int on, uint32_t max_delay_frames)
{
    if (!p) return fail(AIDAX_ERR_ARG, "null pool");
    DelayStage& d = p->delay;
    if (!on) {
        d.on = false;                                       // (off before any on: nothing to change)
        return AIDAX_OK;
    }
    if (max_delay_frames < AIDAX_DELAY_MIN || max_delay_frames > AIDAX_DELAY_MAX) return fail(AIDAX_ERR_ARG, "the stream delays' capacity is 64 .. 262144 frames");
    if (d.enabled()) {
        if (max_delay_frames != d.book.cap) return fail(AIDAX_ERR_STATE, "the stream delays' capacity is fixed once set");
        if (d.on) return AIDAX_OK;
        d.on = true;                                        // off -> on: every line restarts
        return p->on_own_stream([&]() -> int { d.clear_states(0, p->n_streams, p->q); return AIDAX_OK; });
    }
    return first_enable(p, [&] { d.enable(p->n_streams, p->max_frames, max_delay_frames, p->q); });
}

AIDAX_API int aidax_pool_delays(const aidax_pool* p) { return p && p->delay.on ? 1 : 0; }

// the range of streams a call names, or an error
static int delay_streams(aidax_pool* p, int32_t stream, uint32_t* lo, uint32_t* hi)
{
    if (!p) return fail(AIDAX_ERR_ARG, "null pool");
    if (!p->delay.enabled()) return fail(AIDAX_ERR_STATE, "the stream delays were never enabled (aidax_pool_set_delays)");
    return named_range(stream, p->n_streams, lo, hi) ? AIDAX_OK : fail(AIDAX_ERR_ARG, "stream out of range");
}

// the record (or nullptr: off) into the book; the runs that went from off to on restart
static int delay_set(aidax_pool* p, uint32_t lo, uint32_t hi, const aidax_delay_rec* rec, const aidax_delay_params* params)
{
    DelayStage& d = p->delay;
    bool ok = true;
    const auto& restart = d.book.set(lo, hi, rec, params, &ok);
    if (!ok) return fail(AIDAX_ERR_ARG, "the delay and its modulation depth exceed the capacity of aidax_pool_set_delays");
    return restart_runs(p, restart, [&](uint32_t first, uint32_t count) { d.clear_states(first, count, p->q); });
}

AIDAX_API int aidax_pool_set_delay(aidax_pool* p, int32_t stream, const aidax_delay_params* params)
{
    uint32_t lo = 0, hi = 0;
    if (const int rc = delay_streams(p, stream, &lo, &hi)) return rc;
    aidax_delay_rec designed{};
    if (params)
        if (const int rc = aidax_delay_design(params, aidax_pool_samplerate(p), &designed)) return rc;
    return delay_set(p, lo, hi, params ? &designed : nullptr, params);
}

AIDAX_API int aidax_pool_set_delay_rec(aidax_pool* p, int32_t stream, const aidax_delay_rec* rec)
{
    uint32_t lo = 0, hi = 0;
    if (const int rc = delay_streams(p, stream, &lo, &hi)) return rc;
    if (rec && !DelayBook::valid(*rec))
        return fail(AIDAX_ERR_ARG, "delay record: m 64 .. 262144, depth at most 4096 frames, fade at most 1048576, |fb| <= 0.98, 0 <= damp <= 0.5, wet and dry finite and at most 4 in magnitude");
    return delay_set(p, lo, hi, rec, nullptr);
}

AIDAX_API int aidax_pool_stream_delay(const aidax_pool* p, uint32_t stream, aidax_delay_params* params, aidax_delay_rec* rec, int* on)
{
    if (!p) return fail(AIDAX_ERR_ARG, "null pool");
    if (stream >= p->n_streams) return fail(AIDAX_ERR_ARG, "stream out of range");
    const DelayStage& d = p->delay;
    const bool is_on = d.enabled() && d.book.h_rec[stream].on;
    if (params) *params = is_on ? d.book.params[stream] : aidax_delay_params{};
    if (rec) *rec = is_on ? d.book.h_rec[stream] : aidax_delay_rec{};
    if (on) *on = is_on ? 1 : 0;
    return AIDAX_OK;
}

AIDAX_API int aidax_pool_read_delays(aidax_pool* p, uint32_t first, uint32_t count, aidax_delay_state* out)
{
    if (!p || !out) return fail(AIDAX_ERR_ARG, "null argument");
    if (!in_span(first, count, p->n_streams)) return fail(AIDAX_ERR_ARG, "stream range out of the pool's streams");
    if (!p->delay.enabled()) return fail(AIDAX_ERR_STATE, "the stream delays were never enabled (aidax_pool_set_delays)");
    return p->on_own_stream([&]() -> int { p->delay.read(first, count, out, p->q); return AIDAX_OK; });
}

AIDAX_API int aidax_pool_reset_delay(aidax_pool* p, int32_t stream)
{
    uint32_t lo = 0, hi = 0;
    if (const int rc = delay_streams(p, stream, &lo, &hi)) return rc;
    return p->on_own_stream([&]() -> int { p->delay.clear_states(lo, hi - lo, p->q); return AIDAX_OK; });
}

}  // extern "C"
