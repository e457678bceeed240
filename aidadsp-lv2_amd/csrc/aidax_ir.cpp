// aidax_ir.cpp — host side of the cabinet IR stage: the WAV reader (aidax_ir_load_wav) and the packer that turns an IR into the
// A fragments k_ir_conv multiplies (aidax_ir_mfma.hip), and IrPlan, the stage's plan builder. Host only, no HIP call; the device half is
// IrStage (aidax_ir_stage.cpp).
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "aidax_ir_stage.h"
#include "aidax_sinc.h"

namespace aidax {

// Every diagonal q (d = 16 q frames between an output tile and an input window) of the IR as the A operand of
// v_mfma_f32_16x16x32_bf16: lane l holds row i = l % 16, columns k = 8 (l / 16) .. + 7, A[i][k] = h[16 q + i - k] (0 outside the IR),
// each value split into three bf16 terms; [q][term][lane][4 words], two bf16 per word, the lower k in the low half.
std::vector<uint32_t> pack_ir_fragments(const float* h, uint32_t n_taps, uint32_t* n_diag)
{
    const uint32_t Q = ir_diagonals(n_taps);
    std::vector<uint32_t> out(static_cast<size_t>(Q) * 3 * 64 * 4, 0u);
    for (uint32_t q = 0; q < Q; ++q)
        for (int l = 0; l < 64; ++l)
            for (int e = 0; e < 8; ++e) {
                const int tap = 16 * static_cast<int>(q) + (l & 15) - (8 * (l >> 4) + e);
                const float v = tap >= 0 && tap < static_cast<int>(n_taps) ? h[tap] : 0.f;
                uint16_t t[3];
                split_bf16x3(v, t);
                for (int term = 0; term < 3; ++term)
                    out[((static_cast<size_t>(q) * 3 + term) * 64 + l) * 4 + e / 2] |= static_cast<uint32_t>(t[term]) << (16 * (e & 1));
            }
    *n_diag = Q;
    return out;
}

void IrPlan::init(uint32_t n)
{
    const size_t runs = (n + kIrItemStreams - 1) / kIrItemStreams;
    n_streams = n;
    assign.assign(n, AIDAX_IR_POOL);
    played_key.assign(n, -1);
    played_gen.assign(n, 0);
    main.items.resize(runs + kKeys);
    main.streams.resize(n);
    fade_out.items.resize(runs + 2 * kKeys);
    fade_out.streams.resize(n);
    mix.resize(n);
    src.resize(n);
    assign_b.assign(n, AIDAX_IR_NONE);
    ramp.assign(n, Ramp{});
    was_blended.assign(n, 0);
    blend.items.resize(runs + kKeys);
    blend.streams.resize(n);
    blend_list.resize(n);
}

// A section from src[]: the streams with src[s] >= 0 grouped by source, the sources in index order, each one's streams in stream order,
// cut into items of up to kIrItemStreams. Returns the largest number of streams one source holds.
uint32_t IrPlan::group(IrSection& sec, int n_sources)
{
    uint32_t count[2 * kKeys] = {}, at[2 * kKeys];
    for (uint32_t s = 0; s < n_streams; ++s)
        if (src[s] >= 0) ++count[src[s]];
    uint32_t first = 0, most = 0;
    for (int k = 0; k < n_sources; ++k) { at[k] = first; first += count[k]; }
    sec.n_listed = first;
    for (uint32_t s = 0; s < n_streams; ++s)
        if (src[s] >= 0) sec.streams[at[src[s]]++] = s;
    sec.n_items = sec.max_diag = 0;
    first = 0;
    for (int k = 0; k < n_sources; ++k) {
        if (count[k] == 0) continue;
        const IrSlot& sl = source(k);
        for (uint32_t c = 0; c < count[k]; c += kIrItemStreams)
            sec.items[sec.n_items++] = IrItem{ sl.d_frag, sl.n_diag, std::min(kIrItemStreams, count[k] - c), first + c, 0u };
        sec.max_diag = std::max(sec.max_diag, sl.n_diag);
        most = std::max(most, count[k]);
        first += count[k];
    }
    return most;
}

// `any_pass`: the pool has issued a pass (its first one has nothing to fade from). Without a fade length the streams switch as they
// always did; a stream whose old IR is held nowhere any more (neither live nor parked: it was retired under a fade length of 0)
// switches without a fade too.
void IrPlan::rebuild(bool any_pass)
{
    for (uint32_t s = 0; s < n_streams; ++s) src[s] = static_cast<int16_t>(eff_key(s));
    identity = group(main, kKeys) == n_streams;
    const bool fading = any_pass && fade != 0;
    spend_fade();
    for (uint32_t s = 0; s < n_streams; ++s) {
        const int nk = src[s], ok = played_key[s];
        const uint64_t ng = nk >= 0 ? live[nk].gen : 0, og = played_gen[s];
        const bool blended = rest(s) < 0, hand_over = blended || was_blended[s];      // coming to rest and leaving it is no IR change
        src[s] = -2;                                               // no fade
        played_key[s] = static_cast<int8_t>(nk);
        played_gen[s] = ng;
        was_blended[s] = blended;
        if (!fading || hand_over || (nk == ok && ng == og)) continue;
        if (ok < 0) src[s] = -1;                                   // from the dry block
        else if (live[ok].d_frag && live[ok].gen == og) src[s] = static_cast<int16_t>(ok);
        else if (parked[ok].d_frag && parked[ok].gen == og) src[s] = static_cast<int16_t>(kKeys + ok);
        if (src[s] >= -1) mix[n_mix++] = s | (src[s] < 0 ? kIrFadeDry : 0u);
    }
    if (n_mix) group(fade_out, 2 * kKeys);
    // the blended streams: their B sides, and each one's ramp as it stands
    blend.clear();
    n_blend = since_build = rest_in = blend_hi = 0;
    for (uint32_t s = 0; s < n_streams; ++s) {
        src[s] = -1;
        if (!was_blended[s]) continue;
        const Ramp& r = ramp[s];
        src[s] = static_cast<int16_t>(key_b(s));
        blend_list[n_blend++] = IrBlendEntry{ s | (src[s] < 0 ? kIrBlendDry : 0u), r.m0, r.m1, r.len, r.k };
        blend_hi = s;
        if (r.m1 == 0.f || r.m1 == 1.f) {                          // (blended: at least two frames left)
            const uint32_t in = frames_left(s) - 1u;
            rest_in = rest_in ? std::min(rest_in, in) : in;
        }
    }
    if (n_blend) group(blend, kKeys);
    dirty = false;
}

void IrPlan::set_mix(uint32_t s, float mix, uint32_t len)
{
    Ramp& r = ramp[s];
    const int before = rest(s);
    if (frames_left(s) != 0) --n_moving;
    r.m0 = r.now;
    r.m1 = mix + 0.f;                                              // (-0 is 0)
    r.len = len;
    r.k = 0;
    if (r.m0 == r.m1) r.len = 0, r.k = 1;
    else ++n_moving;
    if (before < 0 || rest(s) != before) dirty = true;
}

void IrPlan::advance(uint32_t n_active, uint32_t n_frames)
{
    if (n_frames == 0) return;
    if (n_blend) {
        since_build = std::min(since_build + n_frames, kIrMaxRampOffset);
        if (blend_hi >= n_active) dirty = true;                    // a prefix pass: the streams it left out are where they were
    }
    if (n_moving == 0) return;
    for (uint32_t s = 0; s < n_active; ++s) {
        if (frames_left(s) == 0) continue;
        Ramp& r = ramp[s];
        r.k += std::min(n_frames, frames_left(s));
        r.now = weight(r, r.k - 1u);
        if (frames_left(s) == 0) --n_moving;
    }
}

void IrPlan::commit(int key, IrSlot& staged)
{
    staged.gen = staged.d_frag ? gen_next++ : 0;
    std::swap(live[key], staged);
    // With a fade length set, content that has been played (a pass was issued since its commit) is parked for the streams that will
    // fade from it in the next pass, and `staged` gets what was parked before: an IR retired one commit earlier, whose last possible
    // use, a fade pass, precedes the commit's fence. Content that was never played has no stream to fade from it: it goes to `staged`
    // as ever, and what is parked (which streams may still have played) stays.
    if (fade != 0 && commit_seq[key] != pass_seq) std::swap(parked[key], staged);
    commit_seq[key] = pass_seq;
    dirty = true;                                                  // every stream of that IR switches at this block boundary
}

size_t IrPlan::serialise(uint8_t* snapshot) const
{
    std::memcpy(snapshot, main.items.data(), main.n_items * sizeof(IrItem));
    std::memcpy(snapshot + plan_items_bytes(), main.streams.data(), main.n_listed * sizeof(uint32_t));
    if (n_mix == 0 && n_blend == 0) return plan_items_bytes() + main.n_listed * sizeof(uint32_t);
    if (n_blend != 0) {
        // (one copy up to the end of the blend list, over the fade-out section's place whether that holds a section or not)
        std::memcpy(snapshot + blend_items_off(), blend.items.data(), blend.n_items * sizeof(IrItem));
        std::memcpy(snapshot + blend_streams_off(), blend.streams.data(), blend.n_listed * sizeof(uint32_t));
        std::memcpy(snapshot + blend_list_off(), blend_list.data(), n_blend * sizeof(IrBlendEntry));
        if (n_mix == 0) return blend_list_off() + n_blend * sizeof(IrBlendEntry);
    }
    // the fade-out section rides in the same upload: one copy up to the end of the mix list. It also carries the snapshot's gaps
    // (stream-list entries past n_listed, items past n_items), which no kernel reads: the counts travel as arguments
    std::memcpy(snapshot + fade_items_off(), fade_out.items.data(), fade_out.n_items * sizeof(IrItem));
    std::memcpy(snapshot + fade_streams_off(), fade_out.streams.data(), fade_out.n_listed * sizeof(uint32_t));
    std::memcpy(snapshot + fade_mix_off(), mix.data(), n_mix * sizeof(uint32_t));
    if (n_blend != 0) return blend_list_off() + n_blend * sizeof(IrBlendEntry);
    return fade_mix_off() + n_mix * sizeof(uint32_t);
}

namespace {

uint16_t rd16(const uint8_t* p) { return static_cast<uint16_t>(p[0] | (p[1] << 8)); }
uint32_t rd32(const uint8_t* p) { return static_cast<uint32_t>(p[0]) | (static_cast<uint32_t>(p[1]) << 8) | (static_cast<uint32_t>(p[2]) << 16) | (static_cast<uint32_t>(p[3]) << 24); }

constexpr uint16_t kTagPcm = 1, kTagFloat = 3, kTagExtensible = 0xfffe;
constexpr size_t kMaxWavBytes = size_t(256) << 20;
// the KSDATAFORMAT_SUBTYPE GUID of WAVE_FORMAT_EXTENSIBLE after its leading format tag: {xxxxxxxx-0000-0010-8000-00aa00389b71}
const uint8_t kSubtypeTail[12] = { 0x00, 0x00, 0x10, 0x00, 0x80, 0x00, 0x00, 0xaa, 0x00, 0x38, 0x9b, 0x71 };

int wav_error(const std::string& path, const std::string& what) { return fail(AIDAX_ERR_ARG, path + ": " + what); }

// aidax_ir_resample's filter (aidax_sinc.h: kRsZeros, kRsBeta, kaiser_sinc, shared with the streaming resampler)
constexpr uint32_t kRsMaxLead = 1024;

}  // namespace

}  // namespace aidax

using namespace aidax;

extern "C" {

AIDAX_API int aidax_ir_load_wav(const char* path, float* taps, uint32_t cap, uint32_t* n_frames, double* samplerate)
{
    if (!path || !n_frames || !samplerate || (cap != 0 && !taps)) return fail(AIDAX_ERR_ARG, "null argument");
    *n_frames = 0;
    *samplerate = 0.0;
    FILE* f = std::fopen(path, "rb");
    if (!f) return fail(AIDAX_ERR_IO, std::string(path) + ": cannot open");
    std::vector<uint8_t> buf;
    uint8_t chunk[65536];
    size_t got;
    while ((got = std::fread(chunk, 1, sizeof chunk, f)) > 0) {
        buf.insert(buf.end(), chunk, chunk + got);
        if (buf.size() > kMaxWavBytes) { std::fclose(f); return wav_error(path, "file larger than 256 MiB"); }
    }
    const bool read_error = std::ferror(f) != 0;
    std::fclose(f);
    if (read_error) return fail(AIDAX_ERR_IO, std::string(path) + ": read error");
    const size_t size = buf.size();
    const uint8_t* b = buf.data();
    if (size < 12 || std::memcmp(b, "RIFF", 4) != 0 || std::memcmp(b + 8, "WAVE", 4) != 0) return wav_error(path, "not a RIFF/WAVE file");

    bool have_fmt = false, have_data = false;
    uint16_t tag = 0, channels = 0, block_align = 0, bits = 0;
    uint32_t rate = 0;
    size_t data_off = 0, data_size = 0;
    size_t off = 12;
    while (off < size) {
        if (size - off < 8) return wav_error(path, "truncated chunk header");
        const uint8_t* id = b + off;
        const size_t csize = rd32(b + off + 4);
        const size_t body = off + 8;
        if (csize > size - body) return wav_error(path, std::string(std::memcmp(id, "data", 4) == 0 ? "data" : "a") + " chunk runs past the end of the file");
        if (std::memcmp(id, "fmt ", 4) == 0) {
            if (csize < 16) return wav_error(path, "fmt chunk shorter than 16 bytes");
            const uint8_t* p = b + body;
            tag = rd16(p); channels = rd16(p + 2); rate = rd32(p + 4); block_align = rd16(p + 12); bits = rd16(p + 14);
            if (tag == kTagExtensible) {
                if (csize < 40 || rd16(p + 16) < 22) return wav_error(path, "WAVE_FORMAT_EXTENSIBLE fmt chunk shorter than 40 bytes");
                const uint32_t sub = rd32(p + 24);
                if (std::memcmp(p + 28, kSubtypeTail, sizeof kSubtypeTail) != 0 || sub > 0xffffu) return wav_error(path, "unsupported WAVE_FORMAT_EXTENSIBLE subformat");
                tag = static_cast<uint16_t>(sub);
            }
            have_fmt = true;
        } else if (std::memcmp(id, "data", 4) == 0) {
            data_off = body;
            data_size = csize;
            have_data = true;
        }
        off = body + csize + (csize & 1);                   // chunks are padded to an even size
    }
    if (!have_fmt) return wav_error(path, "no fmt chunk");
    if (!have_data) return wav_error(path, "no data chunk");
    const bool pcm = tag == kTagPcm && (bits == 16 || bits == 24 || bits == 32);
    const bool flt = tag == kTagFloat && bits == 32;
    if (!pcm && !flt) return wav_error(path, "unsupported sample format (tag " + std::to_string(tag) + ", " + std::to_string(bits) + " bits): PCM 16 / 24 / 32-bit and IEEE float 32-bit are read");
    if (channels == 0) return wav_error(path, "zero channels");
    if (block_align != static_cast<uint32_t>(channels) * (bits / 8)) return wav_error(path, "block align does not match channels x sample size");
    if (rate == 0) return wav_error(path, "zero sample rate");
    const size_t frames = data_size / block_align;
    if (frames == 0) return wav_error(path, "no sample frames");
    if (frames > 0xffffffffu) return wav_error(path, "too many sample frames");
    const size_t n = frames < cap ? frames : cap;
    const uint8_t* d = b + data_off;
    for (size_t i = 0; i < n; ++i) {
        const uint8_t* s = d + i * block_align;            // channel 0 of frame i
        float v;
        if (flt) {
            const uint32_t u = rd32(s);
            std::memcpy(&v, &u, sizeof v);
        } else if (bits == 16) {
            v = static_cast<float>(static_cast<int16_t>(rd16(s))) / 32768.f;
        } else if (bits == 24) {
            const int32_t x = static_cast<int32_t>((static_cast<uint32_t>(s[0]) << 8) | (static_cast<uint32_t>(s[1]) << 16) | (static_cast<uint32_t>(s[2]) << 24)) >> 8;
            v = static_cast<float>(x) / 8388608.f;
        } else {
            v = static_cast<float>(static_cast<double>(static_cast<int32_t>(rd32(s))) / 2147483648.0);
        }
        taps[i] = v;
    }
    *n_frames = static_cast<uint32_t>(frames);
    *samplerate = static_cast<double>(rate);
    return AIDAX_OK;
}

// Band-limited rate conversion of an IR (include/aidax.h). With L / M the reduced ratio rate_out / rate_in, D = max(L, M) and
// n = (i - lead) M - k L (exact, 64-bit), input tap k reaches output frame i through c sinc(n / D) K(n / (D Z)), c = min(1, L / M):
// the sinc's sine from n mod 2 D, every sum in fp64 in tap order, one rounding to fp32. No table: any ratio costs the same per tap.
AIDAX_API int aidax_ir_resample(const float* in, uint32_t n_in, double rate_in, double rate_out, uint32_t lead, float* out, uint32_t cap,
                                uint32_t* n_full)
{
    if (n_full) *n_full = 0;
    if (!in || !n_full || (cap != 0 && !out)) return fail(AIDAX_ERR_ARG, "null argument");
    if (n_in == 0) return fail(AIDAX_ERR_ARG, "IR resample: no input taps");
    if (!integer_rate(rate_in) || !integer_rate(rate_out))
        return fail(AIDAX_ERR_ARG, "IR resample: sample rates must be positive integers up to 16777216 (got " + std::to_string(rate_in) + " and " + std::to_string(rate_out) + ")");
    if (lead > kRsMaxLead) return fail(AIDAX_ERR_ARG, "IR resample: lead must be 0 .. 1024 frames");
    for (uint32_t k = 0; k < n_in; ++k)
        if (!std::isfinite(in[k])) return fail(AIDAX_ERR_ARG, "IR resample: tap " + std::to_string(k) + " is not finite");
    const uint64_t ri = static_cast<uint64_t>(rate_in), ro = static_cast<uint64_t>(rate_out), g = gcd_u64(ri, ro);
    const int64_t L = static_cast<int64_t>(ro / g), M = static_cast<int64_t>(ri / g), D = L > M ? L : M;
    const int64_t reach = kRsZeros * D;                                      // |n| < reach: the kernel's support
    // lead + floor((n_in - 1 + Z / c) L / M) + 1, in integers (at most 2^32 2^24 + 2^29)
    const uint64_t full = static_cast<uint64_t>(lead) + static_cast<uint64_t>((static_cast<int64_t>(n_in - 1) * L + reach) / M) + 1u;
    if (full >= (uint64_t(1) << 31)) return fail(AIDAX_ERR_ARG, "IR resample: the result would have 2^31 frames or more");
    *n_full = static_cast<uint32_t>(full);
    const uint32_t n_out = cap < *n_full ? cap : *n_full;
    if (L == M) {                                                            // the same rate: the taps as they are, behind the lead
        for (uint32_t i = 0; i < n_out; ++i) out[i] = i >= lead && i - lead < n_in ? in[i - lead] : 0.f;
        return AIDAX_OK;
    }
    const double scale = L > M ? static_cast<double>(M) / static_cast<double>(L) : 1.0;       // (M / L) c
    const double inv_i0 = 1.0 / bessel_i0(kRsBeta);
    auto weight = [&](int64_t n) { return kaiser_sinc(n, D, inv_i0); };
    // The weight is a function of n alone, and for the usual ratios (D = 160 between 48 and 44.1 kHz) there are far fewer values of n
    // than (frame, tap) pairs: a table of all 2 Z D - 1 of them, the same doubles the direct evaluation gives.
    std::vector<double> table;
    if (D <= 4096 && static_cast<int64_t>(n_out) > D) {
        table.resize(static_cast<size_t>(2 * reach - 1));
        for (int64_t n = 1 - reach; n < reach; ++n) table[static_cast<size_t>(n + reach - 1)] = weight(n);
    }
    for (uint32_t i = 0; i < n_out; ++i) {
        const int64_t a = (static_cast<int64_t>(i) - static_cast<int64_t>(lead)) * M;
        // the taps k with |a - k L| < reach, floor / ceiling divisions of possibly negative numerators
        int64_t lo = a - reach, hi = a + reach;
        int64_t k_lo = (lo >= 0 ? lo / L : -((-lo + L - 1) / L)) + 1;        // floor(lo / L) + 1
        int64_t k_hi = (hi >= 0 ? (hi + L - 1) / L : -(-hi / L)) - 1;        // ceil(hi / L) - 1
        if (k_lo < 0) k_lo = 0;
        if (k_hi > static_cast<int64_t>(n_in) - 1) k_hi = static_cast<int64_t>(n_in) - 1;
        double acc = 0.0;
        for (int64_t k = k_lo; k <= k_hi; ++k) {
            const int64_t n = a - k * L;
            acc += static_cast<double>(in[k]) * (table.empty() ? weight(n) : table[static_cast<size_t>(n + reach - 1)]);
        }
        out[i] = static_cast<float>(scale * acc);
    }
    return AIDAX_OK;
}

}  // extern "C"
