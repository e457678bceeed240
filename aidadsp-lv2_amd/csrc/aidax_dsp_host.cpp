// aidax_dsp_host.cpp — control-rate DSP that stays on the host: biquad design,
// dB -> linear, the ANTIALIASING map, smoother coefficients, and the reduction
// of the 20 control ports to the per-stream record the kernels read.
//
// Built with -ffp-contract=off: the designs must round exactly like the
// reference's calcBiquad (common/Biquad.cpp:67-165) so that the fp64 biquad
// kernels are bit-exact against it. Each filter family is written as
// "denominator polynomial, numerator polynomial, normalise", keeping the
// reference's association order inside every sum and product.
#include <algorithm>
#include <cmath>

#include "aidax_internal.h"
#include <cstring>

#ifndef M_PI
#define M_PI 3.14159265358979323846
#endif

namespace aidax {

namespace {

// (1 + p*K + KK) and (1 - p*K + KK): the two quadratic forms every design uses,
// with the K-coefficient p already multiplied in by the caller where the
// reference multiplies first (p*K evaluated as written there).
inline double quad_plus(double lead, double pk, double kk) { return lead + pk + kk; }
inline double quad_minus(double lead, double pk, double kk) { return lead - pk + kk; }

}  // namespace

void design_biquad(int type, double fc, double q, double gain_db, double c[5])
{
    const double V = std::pow(10, std::fabs(gain_db) / 20.0);
    const double K = std::tan(M_PI * fc);
    const double KK = K * K;
    const bool boost = gain_db >= 0;
    double a0 = 1.0, a1 = 0.0, a2 = 0.0, b1 = 0.0, b2 = 0.0;

    if (type >= 0 && type <= 3) {
        // all-pole part shared by lowpass/highpass/bandpass/notch (Biquad.cpp:72-106)
        const double koq = K / q;
        const double norm = 1 / quad_plus(1, koq, KK);
        b1 = 2 * (KK - 1) * norm;
        b2 = quad_minus(1, koq, KK) * norm;
        switch (type) {
        case 0: a0 = KK * norm;        a1 = 2 * a0;  a2 = a0;  break;
        case 1: a0 = 1 * norm;         a1 = -2 * a0; a2 = a0;  break;
        case 2: a0 = koq * norm;       a1 = 0;       a2 = -a0; break;
        default: a0 = (1 + KK) * norm; a1 = b1;      a2 = a0;  break;   // notch: a1 == b1 term for term
        }
    } else if (type == 4) {
        // peaking EQ (Biquad.cpp:108-125): V rides on the numerator (boost) or denominator (cut)
        const double plain = 1 / q * K, gained = V / q * K;
        const double num_k = boost ? gained : plain;
        const double den_k = boost ? plain : gained;
        const double norm = 1 / quad_plus(1, den_k, KK);
        a0 = quad_plus(1, num_k, KK) * norm;
        a1 = 2 * (KK - 1) * norm;
        a2 = quad_minus(1, num_k, KK) * norm;
        b1 = a1;
        b2 = quad_minus(1, den_k, KK) * norm;
    } else if (type == 5) {
        // low shelf (Biquad.cpp:126-143): the gained side uses sqrt(2V)*K and V*K*K
        const double r2k = std::sqrt(2) * K, s2vk = std::sqrt(2 * V) * K, vkk = V * K * K;
        if (boost) {
            const double norm = 1 / quad_plus(1, r2k, KK);
            a0 = quad_plus(1, s2vk, vkk) * norm;
            a1 = 2 * (vkk - 1) * norm;
            a2 = quad_minus(1, s2vk, vkk) * norm;
            b1 = 2 * (KK - 1) * norm;
            b2 = quad_minus(1, r2k, KK) * norm;
        } else {
            const double norm = 1 / quad_plus(1, s2vk, vkk);
            a0 = quad_plus(1, r2k, KK) * norm;
            a1 = 2 * (KK - 1) * norm;
            a2 = quad_minus(1, r2k, KK) * norm;
            b1 = 2 * (vkk - 1) * norm;
            b2 = quad_minus(1, s2vk, vkk) * norm;
        }
    } else if (type == 6) {
        // high shelf (Biquad.cpp:144-161): the gained side leads with V instead of 1
        const double r2k = std::sqrt(2) * K, s2vk = std::sqrt(2 * V) * K;
        if (boost) {
            const double norm = 1 / quad_plus(1, r2k, KK);
            a0 = quad_plus(V, s2vk, KK) * norm;
            a1 = 2 * (KK - V) * norm;
            a2 = quad_minus(V, s2vk, KK) * norm;
            b1 = 2 * (KK - 1) * norm;
            b2 = quad_minus(1, r2k, KK) * norm;
        } else {
            const double norm = 1 / quad_plus(V, s2vk, KK);
            a0 = quad_plus(1, r2k, KK) * norm;
            a1 = 2 * (KK - 1) * norm;
            a2 = quad_minus(1, r2k, KK) * norm;
            b1 = 2 * (KK - V) * norm;
            b2 = quad_minus(V, s2vk, KK) * norm;
        }
    }
    c[0] = a0; c[1] = a1; c[2] = a2; c[3] = b1; c[4] = b2;
}

float db_to_coeff(float db)
{
    // DB_CO, rt-neural-generic.h:160
    return db > -90.0f ? powf(10.0f, db * 0.05f) : 0.0f;
}

float lpf_fc(float percent)
{
    // MAP(pc, 0, 100, INLPF_MAX_CO, INLPF_MIN_CO), float arithmetic (rt-neural-generic.h:167,178-179)
    const float hi = 0.99f * 0.5f, lo = 0.25f * 0.5f;
    return ((percent - 0.0f) * (lo - hi) / (100.0f - 0.0f)) + hi;
}

float exp_smoother_coef(float samplerate, float t60)
{
    // ExponentialValueSmoother::setTimeConstant + updateCoef (ValueSmoother.hpp:106-115, :147-151)
    const float tau = t60 * (float)(1.0 / 6.91);
    return std::exp(-1.f / (tau * samplerate));
}

void build_stream_ctl(const aidax_controls& c, double sr, bool has_model, bool loading,
                      float gain_coef, float p_den, StreamCtl* o)
{
    // Coefficients are a pure function of the current port values: the reference's
    // *_old change detection (rt-neural-generic.cpp:68-127, :514-517) only decides
    // WHEN setBiquad runs, and setBiquad never touches z1/z2 (Biquad.cpp:60-65).
    design_biquad(0, lpf_fc(c.in_lpf_pc), 0.707f, 0.0f, o->bq[BQ_LPF]);                    // :515
    design_biquad(1, 35.0f / sr, 0.707f, 0.0f, o->bq[BQ_DC]);                               // :293
    design_biquad(4, 75.0f / sr, 0.707f, c.depth_boost_db, o->bq[BQ_DEPTH]);                // :122
    design_biquad(5, c.bass_freq / sr, 0.707f, c.bass_boost_db, o->bq[BQ_BASS]);            // :77
    design_biquad(c.mid_type == 1.0f ? 2 : 4, c.mid_freq / sr, c.mid_q, c.mid_boost_db, o->bq[BQ_MID]);   // :98-103
    design_biquad(6, c.treble_freq / sr, 0.707f, c.treble_boost_db, o->bq[BQ_TREBLE]);      // :116
    design_biquad(6, 900.0f / sr, 0.707f, c.presence_boost_db, o->bq[BQ_PRESENCE]);         // :126

    o->pre_target = db_to_coeff(c.pregain_db);                                              // :489
    o->master_target = loading ? 0.f : db_to_coeff(c.master_db);                            // :490, :654
    o->pre_coef = gain_coef;
    o->master_coef = gain_coef;
    o->p_target[0] = c.param1;
    o->p_target[1] = c.param2;
    o->p_den = p_den;
    uint32_t f = 0;
    if (c.enabled > 0.5f) f |= CTL_ENABLED;                                                 // :495
    if (c.in_lpf_pc != 0.0f) f |= CTL_LPF_ON;                                               // :622
    if (c.eq_bypass == 0.0f && c.eq_position == 1.0f) f |= CTL_EQ_PRE;                      // :628
    if (c.eq_bypass == 0.0f && c.eq_position == 0.0f) f |= CTL_EQ_POST;                     // :651
    if (c.mid_type == 1.0f) f |= CTL_EQ_BANDPASS;                                           // :130
    if (has_model && !(c.net_bypass > 0.5f)) f |= CTL_NET_ON;                               // :631-632
    if (c.dc_blocker == 1.0f) f |= CTL_DC_ON;                                               // :646
    o->flags = f;
    o->pad[0] = o->pad[1] = 0;
}

}  // namespace aidax

using namespace aidax;

extern "C" {

AIDAX_API void aidax_controls_default(aidax_controls* c)
{
    if (!c) return;
    // lv2:default of ports 4..24 (rt-neural-generic.ttl:94-313)
    c->in_lpf_pc = 66.216f; c->pregain_db = 0.f; c->net_bypass = 0.f; c->param1 = 0.f; c->param2 = 0.f;
    c->eq_bypass = 0.f; c->eq_position = 0.f; c->bass_boost_db = 0.f; c->bass_freq = 305.f;
    c->mid_boost_db = 0.f; c->mid_freq = 750.f; c->mid_q = 0.707f; c->mid_type = 0.f;
    c->treble_boost_db = 0.f; c->treble_freq = 2000.f; c->depth_boost_db = 0.f; c->presence_boost_db = 0.f;
    c->dc_blocker = 1.f; c->master_db = 0.f; c->enabled = 1.f;
}

AIDAX_API int aidax_biquad_design(int type, double fc, double q, double gain_db, double coeffs[5])
{
    if (!coeffs || type < 0 || type > 6) return fail(AIDAX_ERR_ARG, "biquad type out of range");
    design_biquad(type, fc, q, gain_db, coeffs);
    return AIDAX_OK;
}

AIDAX_API float aidax_db_to_coeff(float db) { return db_to_coeff(db); }
AIDAX_API float aidax_lpf_fc(float percent) { return lpf_fc(percent); }

// Placement rule of include/aidax.h (pure: the device count and the loads come from the caller)
AIDAX_API int aidax_pick_device(const char* spec, int device_count, const uint32_t* load, int* device_out)
{
    if (!device_out || device_count <= 0) return fail(AIDAX_ERR_ARG, "aidax_pick_device: no device to choose from");
    bool cand[256] = {};
    const int n = device_count < 256 ? device_count : 256;
    if (!spec || !*spec) cand[0] = true;
    else if (!std::strcmp(spec, "auto")) { for (int i = 0; i < n; ++i) cand[i] = true; }
    else {
        const char* p = spec;
        while (*p) {
            if (*p < '0' || *p > '9') return fail(AIDAX_ERR_ARG, "aidax_pick_device: device list is not 'auto' or indices / ranges like 0-3,6");
            long a = 0, b;
            while (*p >= '0' && *p <= '9') { a = a * 10 + (*p++ - '0'); if (a > 100000) return AIDAX_ERR_ARG; }
            b = a;
            if (*p == '-') {
                ++p;
                if (*p < '0' || *p > '9') return AIDAX_ERR_ARG;
                b = 0;
                while (*p >= '0' && *p <= '9') { b = b * 10 + (*p++ - '0'); if (b > 100000) return AIDAX_ERR_ARG; }
                if (b < a) return AIDAX_ERR_ARG;
            }
            for (long i = a; i <= b && i < n; ++i) cand[i] = true;
            if (*p == ',') { ++p; if (!*p) return AIDAX_ERR_ARG; }
            else if (*p) return AIDAX_ERR_ARG;
        }
    }
    int best = -1;
    for (int i = 0; i < n; ++i)
        if (cand[i] && (best < 0 || (load ? load[i] : 0u) < (load ? load[best] : 0u))) best = i;
    if (best < 0) return fail(AIDAX_ERR_ARG, "aidax_pick_device: the device list names no device of this machine");
    *device_out = best;
    return AIDAX_OK;
}

AIDAX_API int aidax_pick_hub(const int* hub_device, const uint32_t* hub_free_seats, int n_hubs, int current_device,
                             const char* spec, int device_count, const uint32_t* load, int* index_out, int* device_out)
{
    if (!index_out || !device_out || n_hubs < 0 || (n_hubs > 0 && (!hub_device || !hub_free_seats))) return aidax::fail(AIDAX_ERR_ARG, "pick_hub: null argument");
    if (current_device >= device_count) return aidax::fail(AIDAX_ERR_ARG, "pick_hub: current device out of range");
    *index_out = -1;
    if (current_device >= 0) {
        // a playing instance keeps its device: its DSP state moves seat to seat on the device (aidax_hub_adopt)
        for (int i = 0; i < n_hubs; ++i)
            if (hub_device[i] == current_device && hub_free_seats[i] > 0) { *index_out = i; break; }
        *device_out = current_device;
        return AIDAX_OK;
    }
    for (int i = 0; i < n_hubs; ++i)
        if (hub_free_seats[i] > 0) { *index_out = i; *device_out = hub_device[i]; return AIDAX_OK; }
    return aidax_pick_device(spec, device_count, load, device_out);
}

// The noise gate's record (include/aidax.h, "Noise gate"): everything in fp64, the thresholds rounded once to fp32, the ramps as integer
// steps of P = 2^24 per frame, rounded up so that a ramp of n frames ends within n frames.
AIDAX_API int aidax_gate_design(const aidax_gate_params* params, double samplerate, aidax_gate_rec* out)
{
    using aidax::fail;
    if (!params || !out) return fail(AIDAX_ERR_ARG, "gate_design: null argument");
    const aidax_gate_params& g = *params;
    if (!std::isfinite(g.open_db) || !std::isfinite(g.close_db) || !std::isfinite(g.floor_db) || !std::isfinite(g.attack_ms) ||
        !std::isfinite(g.hold_ms) || !std::isfinite(g.release_ms))
        return fail(AIDAX_ERR_ARG, "gate_design: every parameter must be finite");
    if (!(g.open_db >= -120.f && g.open_db <= 0.f)) return fail(AIDAX_ERR_ARG, "gate_design: open_db must be in [-120, 0]");
    if (!(g.close_db >= -120.f && g.close_db <= 0.f)) return fail(AIDAX_ERR_ARG, "gate_design: close_db must be in [-120, 0]");
    if (g.close_db > g.open_db) return fail(AIDAX_ERR_ARG, "gate_design: close_db must not exceed open_db");
    if (g.floor_db > 0.f) return fail(AIDAX_ERR_ARG, "gate_design: floor_db must not exceed 0");
    for (const float ms : { g.attack_ms, g.hold_ms, g.release_ms })
        if (!(ms >= 0.f && ms <= 10000.f)) return fail(AIDAX_ERR_ARG, "gate_design: attack_ms, hold_ms and release_ms must be in [0, 10000]");
    if (!(samplerate > 0.0) || !std::isfinite(samplerate)) return fail(AIDAX_ERR_ARG, "gate_design: samplerate must be positive");

    constexpr long long P = 1ll << 24;
    auto frames = [&](float ms) {
        const double f = static_cast<double>(ms) * samplerate / 1000.0;
        return f >= static_cast<double>(P) ? P : std::min(P, std::max(1ll, std::llround(f)));
    };
    auto level = [](float db) { return static_cast<float>(std::pow(10.0, static_cast<double>(db) / 20.0)); };
    const long long attack = frames(g.attack_ms), release = frames(g.release_ms);
    aidax_gate_rec r;
    r.t_open = level(g.open_db);
    r.t_close = level(g.close_db);
    r.floor = g.floor_db <= -120.f ? 0.f : level(g.floor_db);
    r.span = static_cast<float>(1.0 - static_cast<double>(r.floor));
    r.hold = static_cast<uint32_t>(frames(g.hold_ms));
    r.up = static_cast<uint32_t>((P + attack - 1) / attack);
    r.down = static_cast<uint32_t>((P + release - 1) / release);
    r.on = 1u;
    *out = r;
    return AIDAX_OK;
}

// The record of a bus limiter (include/aidax.h, "Bus limiters"), in fp64: the ceiling as a level, the two times as frames.
AIDAX_API int aidax_bus_limit_design(const aidax_bus_limit_params* params, double samplerate, aidax_bus_limit_rec* out)
{
    using aidax::fail;
    if (!params || !out) return fail(AIDAX_ERR_ARG, "bus_limit_design: null argument");
    const aidax_bus_limit_params& l = *params;
    if (!std::isfinite(l.ceiling_db) || !std::isfinite(l.lookahead_ms) || !std::isfinite(l.hold_ms)) return fail(AIDAX_ERR_ARG, "bus_limit_design: every parameter must be finite");
    if (!(samplerate > 0.0) || !std::isfinite(samplerate)) return fail(AIDAX_ERR_ARG, "bus_limit_design: samplerate must be positive");
    if (!(l.ceiling_db >= -60.f && l.ceiling_db <= 12.f)) return fail(AIDAX_ERR_ARG, "bus_limit_design: ceiling_db must be in [-60, 12]");
    if (l.lookahead_ms < 0.f || l.hold_ms < 0.f) return fail(AIDAX_ERR_ARG, "bus_limit_design: lookahead_ms and hold_ms must not be negative");
    const double look = static_cast<double>(l.lookahead_ms) * samplerate / 1000.0, hold = static_cast<double>(l.hold_ms) * samplerate / 1000.0;
    // (compared as fp64 ahead of the rounding: a time of any size is refused, never wrapped)
    if (!(look < AIDAX_BUS_LOOKAHEAD_MAX + 1.0) || std::llround(look) < 1 || std::llround(look) > AIDAX_BUS_LOOKAHEAD_MAX)
        return fail(AIDAX_ERR_ARG, "bus_limit_design: the look-ahead must be 1 .. 512 frames");
    if (!(hold < AIDAX_BUS_HOLD_MAX + 1.0) || std::llround(hold) > AIDAX_BUS_HOLD_MAX) return fail(AIDAX_ERR_ARG, "bus_limit_design: the hold must be at most 4096 frames");
    aidax_bus_limit_rec r;
    r.ceiling = static_cast<float>(std::pow(10.0, static_cast<double>(l.ceiling_db) / 20.0));
    r.lookahead = static_cast<uint32_t>(std::llround(look));
    r.hold = static_cast<uint32_t>(std::llround(hold));
    r.on = 1u;
    *out = r;
    return AIDAX_OK;
}

// The record of a bus reverb (include/aidax.h, "Bus reverbs"), in fp64: eight delays out of the variant's table, scaled by size and rate
// and made odd and distinct, each line's gain for the decay time over its own length, the damping as the FIR's coefficient.
AIDAX_API int aidax_bus_reverb_design(const aidax_bus_reverb_params* params, double samplerate, aidax_bus_reverb_rec* out)
{
    using aidax::fail;
    static const double base[4][AIDAX_BUS_REVERB_LINES] = {
        { 1423, 1637, 1871, 2087, 2311, 2539, 2767, 2999 },
        { 1493, 1693, 1913, 2129, 2357, 2591, 2803, 2971 },
        { 1447, 1663, 1889, 2113, 2339, 2557, 2789, 2963 },
        { 1481, 1709, 1931, 2141, 2371, 2579, 2819, 2953 },
    };
    if (!params || !out) return fail(AIDAX_ERR_ARG, "bus_reverb_design: null argument");
    const aidax_bus_reverb_params& v = *params;
    if (!(samplerate > 0.0) || !std::isfinite(samplerate)) return fail(AIDAX_ERR_ARG, "bus_reverb_design: samplerate must be positive");
    if (!(v.rt60_s >= 0.1f && v.rt60_s <= 20.f)) return fail(AIDAX_ERR_ARG, "bus_reverb_design: rt60_s must be in [0.1, 20]");
    if (!(v.size >= 0.05f && v.size <= 2.f)) return fail(AIDAX_ERR_ARG, "bus_reverb_design: size must be in [0.05, 2]");
    if (!(v.damping >= 0.f && v.damping <= 1.f)) return fail(AIDAX_ERR_ARG, "bus_reverb_design: damping must be in [0, 1]");
    if (!(std::fabs(v.wet) <= 4.f) || !(std::fabs(v.dry) <= 4.f)) return fail(AIDAX_ERR_ARG, "bus_reverb_design: wet and dry must be finite and at most 4 in magnitude");
    if (v.variant > 3u) return fail(AIDAX_ERR_ARG, "bus_reverb_design: variant must be 0 .. 3");
    aidax_bus_reverb_rec r{};
    for (uint32_t i = 0; i < AIDAX_BUS_REVERB_LINES; ++i) {
        const double f = std::floor(base[v.variant][i] * static_cast<double>(v.size) * samplerate / 48000.0 + 0.5);
        // (compared as fp64 ahead of the conversion: a delay of any size is refused, never wrapped)
        if (!(f <= AIDAX_BUS_REVERB_MAX_DELAY)) return fail(AIDAX_ERR_ARG, "bus_reverb_design: a delay exceeds 32768 frames at this size and samplerate");
        uint32_t m = std::max<uint32_t>(AIDAX_BUS_REVERB_MIN_DELAY, static_cast<uint32_t>(f)) | 1u;
        for (uint32_t k = 0; k < i;)
            if (r.m[k] == m) { m += 2u; k = 0; } else ++k;
        if (m > AIDAX_BUS_REVERB_MAX_DELAY) return fail(AIDAX_ERR_ARG, "bus_reverb_design: a delay exceeds 32768 frames at this size and samplerate");
        r.m[i] = m;
        r.gq[i] = static_cast<float>(std::pow(10.0, -3.0 * static_cast<double>(m) / (static_cast<double>(v.rt60_s) * samplerate)) / std::sqrt(8.0));
    }
    r.a = static_cast<float>(static_cast<double>(v.damping) * 0.5);
    r.wet = v.wet;
    r.dry = v.dry;
    r.on = 1u;
    *out = r;
    return AIDAX_OK;
}

// The record of a stream delay (include/aidax.h, "Stream delays"), in fp64: the times as frames, the depth as Q16 frames, the rate as a
// step of the 32-bit phase, the damping as the FIR's coefficient.
AIDAX_API int aidax_delay_design(const aidax_delay_params* params, double samplerate, aidax_delay_rec* out)
{
    using aidax::fail;
    if (!params || !out) return fail(AIDAX_ERR_ARG, "delay_design: null argument");
    const aidax_delay_params& v = *params;
    if (!(samplerate > 0.0) || !std::isfinite(samplerate)) return fail(AIDAX_ERR_ARG, "delay_design: samplerate must be positive");
    // (compared as fp64 ahead of the rounding: a time of any size is refused, never wrapped)
    const double m = static_cast<double>(v.time_ms) * samplerate / 1000.0;
    if (!(m < AIDAX_DELAY_MAX + 1.0) || !(m >= 0.0) || std::llround(m) < AIDAX_DELAY_MIN || std::llround(m) > AIDAX_DELAY_MAX)
        return fail(AIDAX_ERR_ARG, "delay_design: the delay must be 64 .. 262144 frames");
    if (!(std::fabs(v.feedback) <= 0.98f)) return fail(AIDAX_ERR_ARG, "delay_design: feedback must be in [-0.98, 0.98]");
    if (!(v.damping >= 0.f && v.damping <= 1.f)) return fail(AIDAX_ERR_ARG, "delay_design: damping must be in [0, 1]");
    if (!(std::fabs(v.wet) <= 4.f) || !(std::fabs(v.dry) <= 4.f)) return fail(AIDAX_ERR_ARG, "delay_design: wet and dry must be finite and at most 4 in magnitude");
    const double depth = static_cast<double>(v.mod_depth_ms) * samplerate / 1000.0 * 65536.0;
    if (!(depth >= 0.0) || !(depth < AIDAX_DELAY_MAX_DEPTH * 65536.0 + 1.0) || std::llround(depth) > AIDAX_DELAY_MAX_DEPTH * 65536ll)
        return fail(AIDAX_ERR_ARG, "delay_design: the modulation depth must be 0 .. 4096 frames");
    if (!(v.mod_rate_hz >= 0.f && v.mod_rate_hz <= 1000.f) || !(static_cast<double>(v.mod_rate_hz) <= samplerate / 2.0))
        return fail(AIDAX_ERR_ARG, "delay_design: mod_rate_hz must be in [0, 1000] and at most half the samplerate");
    const double fade = static_cast<double>(v.fade_ms) * samplerate / 1000.0;
    if (!(fade >= 0.0) || !(fade < AIDAX_DELAY_MAX_FADE + 1.0) || std::llround(fade) > AIDAX_DELAY_MAX_FADE)
        return fail(AIDAX_ERR_ARG, "delay_design: the fade must be 0 .. 1048576 frames");
    aidax_delay_rec r{};
    r.m = static_cast<uint32_t>(std::llround(m));
    r.depth_q16 = static_cast<uint32_t>(std::llround(depth));
    r.lfo_step = static_cast<uint32_t>(std::llround(static_cast<double>(v.mod_rate_hz) / samplerate * 4294967296.0));
    r.fade = static_cast<uint32_t>(std::llround(fade));
    r.fb = v.feedback;
    r.damp = static_cast<float>(static_cast<double>(v.damping) * 0.5);
    r.wet = v.wet;
    r.dry = v.dry;
    r.on = 1u;
    *out = r;
    return AIDAX_OK;
}

// The stream tuners' design (include/aidax.h, "Stream tuners"): the lag range of [f_min, f_max] at the sample rate, in fp64, the
// shortest lag rounded down and the longest rounded up so that the range holds both frequencies.
AIDAX_API void aidax_tuner_params_default(aidax_tuner_params* params)
{
    if (!params) return;
    *params = aidax_tuner_params{ 2048u, 1024u, 70.f, 1400.f, 0.93f, 0.5f, -60.f };
}

AIDAX_API int aidax_tuner_design(double samplerate, const aidax_tuner_params* params, aidax_tuner_rec* out)
{
    using aidax::fail;
    if (!params || !out) return fail(AIDAX_ERR_ARG, "tuner_design: null argument");
    const aidax_tuner_params& t = *params;
    if (!(samplerate > 0.0) || !std::isfinite(samplerate)) return fail(AIDAX_ERR_ARG, "tuner_design: samplerate must be positive");
    if (t.window != 1024u && t.window != 2048u && t.window != 4096u) return fail(AIDAX_ERR_ARG, "tuner_design: window must be 1024, 2048 or 4096");
    if (t.hop < 64u || t.hop > 65536u || t.hop % 16u != 0u) return fail(AIDAX_ERR_ARG, "tuner_design: hop must be a multiple of 16 from 64 to 65536");
    if (!std::isfinite(t.f_min) || !std::isfinite(t.f_max) || !std::isfinite(t.threshold) || !std::isfinite(t.clarity_min) || !std::isfinite(t.level_min_db))
        return fail(AIDAX_ERR_ARG, "tuner_design: every parameter must be finite");
    if (!(t.f_min > 0.f) || !(t.f_max > 0.f) || t.f_min > t.f_max) return fail(AIDAX_ERR_ARG, "tuner_design: 0 < f_min <= f_max");
    if (!(t.threshold > 0.f && t.threshold <= 1.f)) return fail(AIDAX_ERR_ARG, "tuner_design: threshold must be in (0, 1]");
    if (!(t.clarity_min >= 0.f && t.clarity_min <= 1.f)) return fail(AIDAX_ERR_ARG, "tuner_design: clarity_min must be in [0, 1]");
    if (t.level_min_db > 0.f) return fail(AIDAX_ERR_ARG, "tuner_design: level_min_db must not exceed 0");
    const double lo = std::floor(samplerate / static_cast<double>(t.f_max)), hi = std::ceil(samplerate / static_cast<double>(t.f_min));
    if (!(lo >= 2.0)) return fail(AIDAX_ERR_ARG, "tuner_design: f_max is above half the samplerate (tmin < 2)");
    if (!(hi <= static_cast<double>(t.window / 2u - 1u))) return fail(AIDAX_ERR_ARG, "tuner_design: f_min needs a longer window (tmax > window / 2 - 1)");
    aidax_tuner_rec r{};
    r.window = t.window;
    r.hop = t.hop;
    r.tmin = static_cast<uint32_t>(lo);
    r.tmax = static_cast<uint32_t>(hi);
    r.threshold = t.threshold;
    r.clarity_min = t.clarity_min;
    r.level_min = t.level_min_db <= -200.f ? 0.f : static_cast<float>(std::pow(10.0, static_cast<double>(t.level_min_db) / 20.0));
    r.samplerate = samplerate;
    *out = r;
    return AIDAX_OK;
}

AIDAX_API int aidax_tuner_note(double hz, double a4_hz, int32_t* midi_note, float* cents)
{
    using aidax::fail;
    if (!midi_note || !cents) return fail(AIDAX_ERR_ARG, "tuner_note: null argument");
    if (!(hz > 0.0) || !std::isfinite(hz) || !(a4_hz > 0.0) || !std::isfinite(a4_hz)) return fail(AIDAX_ERR_ARG, "tuner_note: frequencies must be positive and finite");
    const double n = 69.0 + 12.0 * std::log2(hz / a4_hz);
    const double nearest = std::floor(n + 0.5);
    if (!(nearest >= -1000.0 && nearest <= 1000.0)) return fail(AIDAX_ERR_ARG, "tuner_note: the frequency is out of any note range");
    *midi_note = static_cast<int32_t>(nearest);
    *cents = static_cast<float>(100.0 * (n - nearest));
    return AIDAX_OK;
}

}  // extern "C"
