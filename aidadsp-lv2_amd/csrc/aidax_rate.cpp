// aidax_rate.cpp — host half of the rate conversion beside a pool (include/aidax.h, "Rate conversion"): the streaming resampler's
// arithmetic (RsFilter: ratio, row length, weight rows from the Kaiser sinc that aidax_ir_resample uses), aidax_resampler (the device
// state around k_resample: weight table, per-stream history ring, the counters of frames received and outputs produced) and aidax_rate,
// the adapter that runs a pool at its model's rate inside a host at another one: resampler A, the pool's pass, resampler B, all on one
// stream, with the frame counts worked out in exact integers.
#include <algorithm>
#include <cstdio>
#include <memory>
#include <string>
#include <vector>

#include "aidax_rate.h"
#include "aidax_sinc.h"
#include "aidax_hip_host.h"

namespace aidax {

int RsFilter::init(double rate_in, double rate_out)
{
    if (!integer_rate(rate_in) || !integer_rate(rate_out))
        return fail(AIDAX_ERR_ARG, "rate conversion: sample rates must be positive integers up to 16777216 (got " + std::to_string(rate_in) + " and " + std::to_string(rate_out) + ")");
    const uint64_t ri = static_cast<uint64_t>(rate_in), ro = static_cast<uint64_t>(rate_out), g = gcd_u64(ri, ro);
    L = static_cast<int64_t>(ro / g);
    M = static_cast<int64_t>(ri / g);
    D = L > M ? L : M;
    if (D > kRsMaxRatioTerm)
        return fail(AIDAX_ERR_ARG, "rate conversion: " + std::to_string(ro) + " / " + std::to_string(ri) + " is " + std::to_string(L) + " / " + std::to_string(M) +
                                   " in lowest terms, and max(L, M) must not exceed 640");
    H = (kRsZeros * D + L - 1) / L;
    T = 2 * H + 1;
    c = L < M ? static_cast<double>(L) / static_cast<double>(M) : 1.0;
    return AIDAX_OK;
}

void RsFilter::row(uint32_t phase, float* w) const
{
    const double inv_i0 = 1.0 / bessel_i0(kRsBeta);
    const int64_t reach = kRsZeros * D;
    for (int64_t i = -H; i <= H; ++i) {
        const int64_t n = static_cast<int64_t>(phase) + i * L;
        w[i + H] = n > -reach && n < reach ? static_cast<float>(c * kaiser_sinc(n, D, inv_i0)) : 0.f;
    }
}

}  // namespace aidax

using namespace aidax;

// One conversion rate_in -> rate_out for n_streams streams. Frames and outputs are counted since creation, the same for every stream:
// `received` input frames appended so far, `produced` outputs written so far. One caller at a time.
struct aidax_resampler {
    Stream q;                            // the stream of calls that name none (declared first, destroyed last: behind the blocks and the event)
    int device = 0;
    uint32_t n_streams = 0, max_in = 0, out_cap = 0;
    RsFilter f;
    int64_t d_in = 0, d_out = 0;
    uint32_t R = 0;                      // ring slots per stream, a power of two >= T + 2 max_in + 2 ceil(M / L) + 2
    DevBuf<float> d_ring;
    DevBuf<float> d_wt;                  // [T][L]
    uint64_t received = 0, produced = 0;
    hipStream_t last_stream = nullptr;
    Event ev_x;                          // edge between two streams that carry calls one after the other
    // aidax_resampler_process: pinned host and device staging of max_in resp. out_cap frames per stream (public creation only)
    PinnedBuf<float> h_in, h_out;
    DevBuf<float> d_sin, d_sout;

    int64_t numer(uint64_t j) const { return (static_cast<int64_t>(j) - d_out) * f.M - d_in * f.L; }
    // outputs j < ready_end(n) have their whole row inside the first n input frames: q(j) + H < n, i.e. (j - d_out) M < (n - H + d_in) L
    int64_t ready_end(uint64_t n) const { return d_out + ceil_div((static_cast<int64_t>(n) - f.H + d_in) * f.L, f.M); }
    uint32_t ready(uint64_t n) const
    {
        const int64_t r = ready_end(n) - static_cast<int64_t>(produced);
        return r <= 0 ? 0u : static_cast<uint32_t>(std::min<int64_t>(r, kRsMaxOut));
    }
    void enter_stream(hipStream_t s)
    {
        if (last_stream && last_stream != s) {
            HIP_TRY(hipEventRecord(ev_x.get(), last_stream));
            HIP_TRY(hipStreamWaitEvent(s, ev_x.get(), 0));
        }
        last_stream = s;
    }
};

namespace {

int resampler_create(uint32_t n_streams, double rate_in, double rate_out, uint32_t d_in, uint32_t d_out, uint32_t max_in, int device, bool host_staging,
                     aidax_resampler** out)
{
    if (!out) return fail(AIDAX_ERR_ARG, "null argument");
    *out = nullptr;
    if (n_streams == 0 || n_streams > 65535u || max_in == 0 || max_in > kRsMaxOut) return fail(AIDAX_ERR_ARG, "resampler: n_streams (1 .. 65535) or max_in_frames (1 .. 2^20) out of range");
    if (d_in > kRsMaxDelay || d_out > kRsMaxDelay) return fail(AIDAX_ERR_ARG, "resampler: a delay must be 0 .. 65536 frames");
    RsFilter f;
    if (const int rc = f.init(rate_in, rate_out)) return rc;
    return guarded([&]() -> int {
        int n_dev = 0;
        if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev <= 0) return fail(AIDAX_ERR_DEVICE, "no HIP device: the MI355X path has no CPU fallback");
        if (device < 0 || device >= n_dev) return fail(AIDAX_ERR_ARG, "device_id out of range");
        auto rs = std::make_unique<aidax_resampler>();
        rs->device = device; rs->n_streams = n_streams; rs->max_in = max_in; rs->f = f; rs->d_in = d_in; rs->d_out = d_out;
        // A caller that takes every ready output needs the latest 2 H frames and the new block; the ring holds a second block on top,
        // so that a call may also leave its outputs to the next one.
        // (and the up to ceil(M / L) frames by which the next output's row may trail the latest one's)
        uint32_t R = 64;
        while (R < static_cast<uint64_t>(f.T) + 2u * static_cast<uint64_t>(max_in) + 2u * static_cast<uint64_t>(ceil_div(f.M, f.L)) + 2u) R *= 2;
        rs->R = R;
        rs->out_cap = static_cast<uint32_t>(std::min<int64_t>(ceil_div((static_cast<int64_t>(max_in) + f.T) * f.L, f.M) + 2, kRsMaxOut));
        // (a failure from here on: the owning members give back what was made, the stream last)
        HIP_TRY(hipSetDevice(device));
        rs->q.create();
        rs->ev_x.create();
        const size_t ring_floats = n_streams * static_cast<size_t>(R);
        rs->d_ring.alloc(ring_floats);
        HIP_TRY(hipMemsetAsync(rs->d_ring.get(), 0, sizeof(float) * ring_floats, rs->q));
        std::vector<float> row(static_cast<size_t>(f.T)), wt(static_cast<size_t>(f.T * f.L));
        for (int64_t phi = 0; phi < f.L; ++phi) {
            f.row(static_cast<uint32_t>(phi), row.data());
            for (int64_t i = 0; i < f.T; ++i) wt[static_cast<size_t>(i * f.L + phi)] = row[static_cast<size_t>(i)];
        }
        rs->d_wt.alloc(wt.size());
        HIP_TRY(hipMemcpyAsync(rs->d_wt.get(), wt.data(), wt.size() * sizeof(float), hipMemcpyHostToDevice, rs->q));
        if (host_staging) {
            const size_t in_floats = n_streams * static_cast<size_t>(max_in), out_floats = n_streams * static_cast<size_t>(rs->out_cap);
            rs->h_in.alloc(in_floats);
            rs->h_out.alloc(out_floats);
            rs->d_sin.alloc(in_floats);
            rs->d_sout.alloc(out_floats);
        }
        HIP_TRY(hipStreamSynchronize(rs->q));                          // (the table's host copy ends with this scope)
        rs->last_stream = rs->q;
        *out = rs.release();
        return AIDAX_OK;
    });
}

void resampler_destroy(aidax_resampler* rs)
{
    if (!rs) return;
    (void)hipSetDevice(rs->device);
    if (rs->last_stream && rs->last_stream != rs->q) (void)hipStreamSynchronize(rs->last_stream);
    if (rs->q) (void)hipStreamSynchronize(rs->q);
    delete rs;
}

// the checks, the counters and the one launch of a call; HIP failures leave as HipFail
int resampler_issue(aidax_resampler* rs, const float* d_in, uint32_t n_in, float* d_out, uint32_t n_out, hipStream_t s)
{
    if (n_in > rs->max_in) return fail(AIDAX_ERR_ARG, "resampler: n_in exceeds max_in_frames");
    if ((n_in != 0 && !d_in) || (n_out != 0 && !d_out)) return fail(AIDAX_ERR_ARG, "null buffer");
    const uint64_t received = rs->received + n_in;
    if (n_out > rs->ready(received))
        return fail(AIDAX_ERR_STATE, "resampler: " + std::to_string(n_out) + " outputs asked for, " + std::to_string(rs->ready(received)) +
                                     " have their inputs (an output's row must end inside the frames received)");
    if (n_in == 0 && n_out == 0) return AIDAX_OK;
    const RsFilter& f = rs->f;
    const int64_t a0 = rs->numer(rs->produced), q0 = floor_div(a0, f.L);
    // the oldest frame the next output reads (this call's or a later one's) must outlive the append
    const int64_t oldest = std::max<int64_t>(q0 - f.H, 0);
    if (static_cast<int64_t>(received) - oldest > static_cast<int64_t>(rs->R))
        return fail(AIDAX_ERR_STATE, "resampler: the outputs of earlier calls were not taken (the new frames would overwrite history they need)");
    ResampleArgs a{};
    a.wt = rs->d_wt.get(); a.ring = rs->d_ring.get(); a.in = d_in; a.out = d_out;
    a.L = static_cast<uint32_t>(f.L); a.M = static_cast<uint32_t>(f.M); a.H = static_cast<uint32_t>(f.H);
    a.mask = rs->R - 1u; a.pos = static_cast<uint32_t>(rs->received & (rs->R - 1u));
    a.n_streams = rs->n_streams; a.n_in = n_in; a.n_out = n_out;
    a.n_hist = static_cast<uint32_t>(std::min<uint64_t>(rs->received, rs->R));
    a.phi0 = static_cast<uint32_t>(a0 - q0 * f.L);
    a.q0 = static_cast<int32_t>(q0 - static_cast<int64_t>(rs->received));
    a.copy = f.equal() ? 1u : 0u;
    HIP_TRY(hipSetDevice(rs->device));
    rs->enter_stream(s);
    HIP_TRY(launch_resample(a, s));
    rs->received = received;
    rs->produced += n_out;
    return AIDAX_OK;
}

int resampler_reset_stream(aidax_resampler* rs, uint32_t stream)
{
    if (stream >= rs->n_streams) return fail(AIDAX_ERR_ARG, "stream out of range");
    return guarded([&]() -> int {
        HIP_TRY(hipSetDevice(rs->device));
        HIP_TRY(hipMemsetAsync(rs->d_ring.get() + static_cast<size_t>(stream) * rs->R, 0, sizeof(float) * rs->R, rs->last_stream));
        return AIDAX_OK;
    });
}

}  // namespace

// A pool at its model's rate inside a host at another: host block -> A -> the pool's pass -> B -> host block, on one stream.
struct ResamplerDelete { void operator()(aidax_resampler* rs) const { resampler_destroy(rs); } };

struct aidax_rate {
    Stream q;                            // the stream of calls that name none (declared first, destroyed last)
    aidax_pool* pool = nullptr;
    int device = 0;
    uint32_t n_streams = 0, max_frames = 0, pool_cap = 0, latency = 0;
    uint64_t La = 1, Ma = 1;             // pool_rate / host_rate in lowest terms
    bool equal = false;
    DevBuf<float> d_a;                   // [n_streams][m]: the pool's input block
    DevBuf<float> d_b;                   // ... and its output block
    PinnedBuf<float> h_in, h_out;        // aidax_rate_process: pinned staging of the host block, and its place on the device
    DevBuf<float> d_hin, d_hout;
    std::unique_ptr<aidax_resampler, ResamplerDelete> A;      // host -> pool (the two resamplers go first, as they did)
    std::unique_ptr<aidax_resampler, ResamplerDelete> B;      // pool -> host
    hipStream_t last = nullptr;          // the stream last handed to the pool through the adapter
    uint64_t N = 0;                      // host frames received
};

namespace {

// H_A + d_B, d_B = ceil((H_B + 1) Ma / La): A is host -> pool (L / M = La / Ma), B pool -> host (Ma / La)
int rate_delays(double host_rate, double pool_rate, RsFilter* fa, RsFilter* fb, uint32_t* d_b)
{
    if (const int rc = fa->init(host_rate, pool_rate)) return rc;
    if (const int rc = fb->init(pool_rate, host_rate)) return rc;
    *d_b = static_cast<uint32_t>(ceil_div((fb->H + 1) * fb->L, fb->M));
    return AIDAX_OK;
}

}  // namespace

extern "C" {

AIDAX_API int aidax_resampler_create(uint32_t n_streams, double rate_in, double rate_out, uint32_t d_in, uint32_t d_out, uint32_t max_in_frames,
                                     int device_id, aidax_resampler** out)
{
    return resampler_create(n_streams, rate_in, rate_out, d_in, d_out, max_in_frames, device_id, true, out);
}

AIDAX_API void aidax_resampler_destroy(aidax_resampler* rs) { resampler_destroy(rs); }

AIDAX_API int aidax_resampler_row(double rate_in, double rate_out, uint32_t phase, float* w, uint32_t cap, uint32_t* n_taps)
{
    if (n_taps) *n_taps = 0;
    if (!n_taps || (cap != 0 && !w)) return fail(AIDAX_ERR_ARG, "null argument");
    RsFilter f;
    if (const int rc = f.init(rate_in, rate_out)) return rc;
    if (phase >= static_cast<uint64_t>(f.L)) return fail(AIDAX_ERR_ARG, "resampler row: phase must be below L = " + std::to_string(f.L));
    *n_taps = static_cast<uint32_t>(f.T);
    if (cap == 0) return AIDAX_OK;
    std::vector<float> row(static_cast<size_t>(f.T));
    f.row(phase, row.data());
    std::copy(row.begin(), row.begin() + std::min<size_t>(cap, row.size()), w);
    return AIDAX_OK;
}

AIDAX_API int aidax_resampler_process_device(aidax_resampler* rs, const float* d_in, uint32_t n_in, float* d_out, uint32_t n_out, void* hip_stream)
{
    if (!rs) return fail(AIDAX_ERR_ARG, "null resampler");
    return guarded([&]() -> int { return resampler_issue(rs, d_in, n_in, d_out, n_out, hip_stream ? static_cast<hipStream_t>(hip_stream) : rs->q); });
}

AIDAX_API int aidax_resampler_process(aidax_resampler* rs, const float* in, uint32_t n_in, float* out, uint32_t n_out)
{
    if (!rs) return fail(AIDAX_ERR_ARG, "null resampler");
    if (!rs->h_in) return fail(AIDAX_ERR_STATE, "resampler: no host staging");
    if (n_in > rs->max_in) return fail(AIDAX_ERR_ARG, "resampler: n_in exceeds max_in_frames");
    if (n_out > rs->out_cap) return fail(AIDAX_ERR_ARG, "resampler: the blocking call takes at most " + std::to_string(rs->out_cap) + " outputs a call");
    if ((n_in != 0 && !in) || (n_out != 0 && !out)) return fail(AIDAX_ERR_ARG, "null buffer");
    return guarded([&]() -> int {
        HIP_TRY(hipSetDevice(rs->device));
        const size_t in_bytes = sizeof(float) * rs->n_streams * static_cast<size_t>(n_in), out_bytes = sizeof(float) * rs->n_streams * static_cast<size_t>(n_out);
        if (in_bytes) {
            std::memcpy(rs->h_in.get(), in, in_bytes);
            rs->enter_stream(rs->q);
            HIP_TRY(hipMemcpyAsync(rs->d_sin.get(), rs->h_in.get(), in_bytes, hipMemcpyHostToDevice, rs->q));
        }
        if (const int rc = resampler_issue(rs, rs->d_sin.get(), n_in, rs->d_sout.get(), n_out, rs->q)) return rc;
        if (out_bytes) HIP_TRY(hipMemcpyAsync(rs->h_out.get(), rs->d_sout.get(), out_bytes, hipMemcpyDeviceToHost, rs->q));
        HIP_TRY(hipStreamSynchronize(rs->q));
        if (out_bytes) std::memcpy(out, rs->h_out.get(), out_bytes);
        return AIDAX_OK;
    });
}

AIDAX_API uint32_t aidax_resampler_ready(const aidax_resampler* rs) { return rs ? rs->ready(rs->received) : 0; }

AIDAX_API int aidax_resampler_reset_stream(aidax_resampler* rs, uint32_t stream)
{
    if (!rs) return fail(AIDAX_ERR_ARG, "null resampler");
    return resampler_reset_stream(rs, stream);
}

AIDAX_API int aidax_rate_latency(double host_rate, double pool_rate, uint32_t* frames)
{
    if (frames) *frames = 0;
    if (!frames) return fail(AIDAX_ERR_ARG, "null argument");
    RsFilter fa, fb;
    uint32_t d_b = 0;
    if (const int rc = rate_delays(host_rate, pool_rate, &fa, &fb, &d_b)) return rc;
    *frames = fa.equal() ? 0u : static_cast<uint32_t>(fa.H) + d_b;
    return AIDAX_OK;
}

AIDAX_API int aidax_rate_create(aidax_pool* pool, double host_rate, uint32_t max_frames, aidax_rate** out)
{
    if (out) *out = nullptr;
    if (!pool || !out) return fail(AIDAX_ERR_ARG, "null argument");
    if (max_frames == 0) return fail(AIDAX_ERR_ARG, "rate adapter: max_frames must be at least 1");
    RsFilter fa, fb;
    uint32_t d_b = 0;
    if (const int rc = rate_delays(host_rate, aidax_pool_samplerate(pool), &fa, &fb, &d_b)) return rc;
    const uint64_t m_cap = static_cast<uint64_t>(ceil_div(static_cast<int64_t>(max_frames) * fa.L, fa.M));
    if (m_cap > pool_max_frames(pool))
        return fail(AIDAX_ERR_ARG, "rate adapter: " + std::to_string(max_frames) + " host frames are up to " + std::to_string(m_cap) +
                                   " frames at the pool's rate, more than the pool's max_frames (" + std::to_string(pool_max_frames(pool)) + ")");
    return guarded([&]() -> int {
        auto r = std::make_unique<aidax_rate>();
        r->pool = pool; r->device = pool_device(pool); r->n_streams = aidax_pool_streams(pool); r->max_frames = max_frames;
        r->pool_cap = static_cast<uint32_t>(m_cap);
        r->La = static_cast<uint64_t>(fa.L); r->Ma = static_cast<uint64_t>(fa.M);
        r->equal = fa.equal();
        r->latency = r->equal ? 0u : static_cast<uint32_t>(fa.H) + d_b;
        if (r->equal) { *out = r.release(); return AIDAX_OK; }           // forwards to the pool: nothing of its own
        // (a failure from here on: the owning members give back what was made, the stream last)
        HIP_TRY(hipSetDevice(r->device));
        r->q.create();
        aidax_resampler* made = nullptr;
        if (const int rc = resampler_create(r->n_streams, host_rate, aidax_pool_samplerate(pool), static_cast<uint32_t>(fa.H), 0, max_frames, r->device, false, &made)) return rc;
        r->A.reset(made);
        if (const int rc = resampler_create(r->n_streams, aidax_pool_samplerate(pool), host_rate, 0, d_b, r->pool_cap, r->device, false, &made)) return rc;
        r->B.reset(made);
        const size_t pool_floats = r->n_streams * static_cast<size_t>(r->pool_cap), host_floats = r->n_streams * static_cast<size_t>(max_frames);
        r->d_a.alloc(pool_floats);
        r->d_b.alloc(pool_floats);
        r->h_in.alloc(host_floats);
        r->h_out.alloc(host_floats);
        r->d_hin.alloc(host_floats);
        r->d_hout.alloc(host_floats);
        *out = r.release();
        return AIDAX_OK;
    });
}

AIDAX_API void aidax_rate_destroy(aidax_rate* r)
{
    if (!r) return;
    (void)hipSetDevice(r->device);
    // the adapter's passes end, then the pool goes back to its own stream by the event edge alone (a zero-frame pass would latch targets)
    if (r->last) (void)hipStreamSynchronize(r->last);
    if (r->q) (void)hipStreamSynchronize(r->q);
    if (r->last) (void)pool_enter_own_stream(r->pool);
    delete r;
}

AIDAX_API uint32_t aidax_rate_latency_frames(const aidax_rate* r) { return r ? r->latency : 0; }

AIDAX_API int aidax_rate_process_device(aidax_rate* r, const float* d_in, float* d_out, uint32_t n_frames, void* hip_stream)
{
    if (!r) return fail(AIDAX_ERR_ARG, "null rate adapter");
    if (n_frames > r->max_frames) return fail(AIDAX_ERR_ARG, "n_frames exceeds the adapter's max_frames");
    if (n_frames != 0 && (!d_in || !d_out)) return fail(AIDAX_ERR_ARG, "null buffer");
    if (r->equal) {
        r->last = hip_stream ? static_cast<hipStream_t>(hip_stream) : r->last;
        return aidax_pool_process_device(r->pool, d_in, d_out, n_frames, hip_stream);
    }
    hipStream_t s = hip_stream ? static_cast<hipStream_t>(hip_stream) : r->q;
    r->last = s;
    if (n_frames == 0) return aidax_pool_process_device(r->pool, nullptr, nullptr, 0, s);      // the pre-run: targets latched, nothing else moves
    // pool frames of this call: floor(N' La / Ma) - floor(N La / Ma), N' = N + n
    const uint32_t m = static_cast<uint32_t>((r->N + n_frames) * r->La / r->Ma - r->N * r->La / r->Ma);
    return guarded([&]() -> int {
        if (const int rc = resampler_issue(r->A.get(), d_in, n_frames, r->d_a.get(), m, s)) return rc;
        if (const int rc = aidax_pool_process_device(r->pool, r->d_a.get(), r->d_b.get(), m, s)) return rc;
        if (const int rc = resampler_issue(r->B.get(), r->d_b.get(), m, d_out, n_frames, s)) return rc;
        r->N += n_frames;
        return AIDAX_OK;
    });
}

AIDAX_API int aidax_rate_process(aidax_rate* r, const float* in, float* out, uint32_t n_frames)
{
    if (!r) return fail(AIDAX_ERR_ARG, "null rate adapter");
    if (r->equal) return aidax_pool_process(r->pool, in, out, n_frames);
    if (n_frames > r->max_frames) return fail(AIDAX_ERR_ARG, "n_frames exceeds the adapter's max_frames");
    if (n_frames != 0 && (!in || !out)) return fail(AIDAX_ERR_ARG, "null buffer");
    return guarded([&]() -> int {
        HIP_TRY(hipSetDevice(r->device));
        const size_t bytes = sizeof(float) * r->n_streams * static_cast<size_t>(n_frames);
        if (bytes) {
            std::memcpy(r->h_in.get(), in, bytes);
            HIP_TRY(hipMemcpyAsync(r->d_hin.get(), r->h_in.get(), bytes, hipMemcpyHostToDevice, r->q));
        }
        if (const int rc = aidax_rate_process_device(r, r->d_hin.get(), r->d_hout.get(), n_frames, r->q)) return rc;
        if (bytes) HIP_TRY(hipMemcpyAsync(r->h_out.get(), r->d_hout.get(), bytes, hipMemcpyDeviceToHost, r->q));
        HIP_TRY(hipStreamSynchronize(r->q));
        if (pool_take_lp_fault(r->pool)) {                    // the pool's pass is wrong: silence, as aidax_pool_process reports it
            if (bytes) std::memset(out, 0, bytes);
            return fail(AIDAX_ERR_DEVICE, "k_mfma_lp: a layer hand-over timed out (this block is silence; the pool falls back to k_mfma)");
        }
        if (bytes) std::memcpy(out, r->h_out.get(), bytes);
        return AIDAX_OK;
    });
}

AIDAX_API int aidax_rate_reset_stream(aidax_rate* r, uint32_t stream)
{
    if (!r) return fail(AIDAX_ERR_ARG, "null rate adapter");
    if (stream >= r->n_streams) return fail(AIDAX_ERR_ARG, "stream out of range");
    if (r->equal) return AIDAX_OK;
    if (const int rc = resampler_reset_stream(r->A.get(), stream)) return rc;
    return resampler_reset_stream(r->B.get(), stream);
}

}  // extern "C"
