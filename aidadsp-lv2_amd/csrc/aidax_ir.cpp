// aidax_ir.cpp — host side of the cabinet IR stage: the WAV reader (aidax_ir_load_wav) and the packer that turns an IR into the
// A fragments k_ir_conv multiplies (aidax_ir_mfma.hip). Host only; the pool's half (prepare / commit) is in aidax_pool.cpp.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "aidax_internal.h"
#include "aidax_kernels.h"

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

namespace {

uint16_t rd16(const uint8_t* p) { return static_cast<uint16_t>(p[0] | (p[1] << 8)); }
uint32_t rd32(const uint8_t* p) { return static_cast<uint32_t>(p[0]) | (static_cast<uint32_t>(p[1]) << 8) | (static_cast<uint32_t>(p[2]) << 16) | (static_cast<uint32_t>(p[3]) << 24); }

constexpr uint16_t kTagPcm = 1, kTagFloat = 3, kTagExtensible = 0xfffe;
constexpr size_t kMaxWavBytes = size_t(256) << 20;
// the KSDATAFORMAT_SUBTYPE GUID of WAVE_FORMAT_EXTENSIBLE after its leading format tag: {xxxxxxxx-0000-0010-8000-00aa00389b71}
const uint8_t kSubtypeTail[12] = { 0x00, 0x00, 0x10, 0x00, 0x80, 0x00, 0x00, 0xaa, 0x00, 0x38, 0x9b, 0x71 };

int wav_error(const std::string& path, const std::string& what) { return fail(AIDAX_ERR_ARG, path + ": " + what); }

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

}  // extern "C"
