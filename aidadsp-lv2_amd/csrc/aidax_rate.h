// aidax_rate.h — rate conversion beside a pool (include/aidax.h, "Rate conversion"): RsFilter, the host-only arithmetic of the streaming
// resampler (the ratio, the row length, one weight row from the Kaiser sinc of aidax_sinc.h), and the two types built on it in
// aidax_rate.cpp: aidax_resampler (the history ring, the weight table and the counters around k_resample) and aidax_rate (two of
// them around a borrowed pool).
#pragma once

#include <cstdint>

#include "aidax_internal.h"

namespace aidax {

constexpr int64_t kRsMaxRatioTerm = 640;       // max(L, M): every pair of 44.1 / 48 / 88.2 / 96 / 176.4 / 192 kHz
constexpr int64_t kRsMaxDelay = 65536;         // d_in, d_out
constexpr uint32_t kRsMaxOut = 1u << 20;       // outputs of one call (t M stays far below 2^32)

struct RsFilter {
    int64_t L = 1, M = 1, D = 1, H = 0, T = 1;  // L / M = rate_out / rate_in in lowest terms, D = max(L, M), H = ceil(Z D / L), T = 2 H + 1
    double c = 1.0;                             // min(1, L / M)
    bool equal() const { return L == M; }
    // fails with AIDAX_ERR_ARG and the reason: rates that are no positive integers <= 2^24, max(L, M) > 640
    int init(double rate_in, double rate_out);
    // w[i + H] = c sinc(c (phase + i L) / L) K(c (phase + i L) / (L Z)), i = -H .. H: fp64, rounded once to fp32
    void row(uint32_t phase, float* w) const;
};

inline int64_t floor_div(int64_t a, int64_t b) { const int64_t q = a / b; return (a % b != 0 && ((a < 0) != (b < 0))) ? q - 1 : q; }
inline int64_t ceil_div(int64_t a, int64_t b) { return -floor_div(-a, b); }

}  // namespace aidax
