// aidax_sinc.h — the Kaiser-windowed sinc that aidax_ir_resample (aidax_ir.cpp) and the streaming resampler's weight rows
// (aidax_rate.cpp) share: a sinc of kRsZeros zero crossings a side under a Kaiser window of shape kRsBeta (include/aidax.h), evaluated in
// fp64 from an exact integer numerator. Host only.
#pragma once

#include <cmath>
#include <cstdint>

namespace aidax {

constexpr int64_t kRsZeros = 32;
constexpr double kRsBeta = 12.0;
constexpr double kRsPi = 3.14159265358979323846;

// I0 by its power series, sum ((x / 2)^k / k!)^2: every term positive, 40 of them at x = 12
inline double bessel_i0(double x)
{
    const double q = 0.25 * x * x;
    double term = 1.0, sum = 1.0;
    for (int k = 1; k < 200; ++k) {
        term *= q / (static_cast<double>(k) * static_cast<double>(k));
        sum += term;
        if (term < 1e-20 * sum) break;
    }
    return sum;
}

inline uint64_t gcd_u64(uint64_t a, uint64_t b)
{
    while (b) { const uint64_t t = a % b; a = b; b = t; }
    return a;
}

// sin(pi n / D) from the residue of n mod 2 D folded into [0, D / 2]: exactly 0 where n / D is an integer
inline double sin_pi_ratio(int64_t n, int64_t D)
{
    int64_t r = n % (2 * D);
    if (r < 0) r += 2 * D;
    double sign = 1.0;
    if (r >= D) { r -= D; sign = -1.0; }
    if (2 * r > D) r = D - r;
    return r == 0 ? 0.0 : sign * std::sin(kRsPi * static_cast<double>(r) / static_cast<double>(D));
}

inline bool integer_rate(double r) { return r >= 1.0 && r <= 16777216.0 && r == std::floor(r); }

// sinc(n / D) K(n / (D Z)) for |n| < Z D (the caller keeps to the support), inv_i0 = 1 / I0(beta): 1 at n = 0, 0 at every other multiple of D
inline double kaiser_sinc(int64_t n, int64_t D, double inv_i0)
{
    if (n == 0) return 1.0;
    const double x = static_cast<double>(n) / static_cast<double>(D);
    const double v = x / static_cast<double>(kRsZeros);
    return sin_pi_ratio(n, D) / (kRsPi * x) * bessel_i0(kRsBeta * std::sqrt(1.0 - v * v)) * inv_i0;
}

}  // namespace aidax
