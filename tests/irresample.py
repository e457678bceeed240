"""aidax_ir_resample's formula (include/aidax.h) stated once more, independently, in numpy fp64: what tests/test_ir_resample_host.py and
tests/test_gpu_ir_rates.py hold the library against. It never calls the library.

    out[i] = (M / L) sum_k in[k] c sinc(c u) K(c u / Z),   u = ((i - lead) M - k L) / L,   c = min(1, L / M),   Z = 32,   beta = 12
    K(v) = I0(beta sqrt(1 - v^2)) / I0(beta) for |v| < 1, else 0

The numerator of u is formed from Python integers (exact), and with D = max(L, M) the argument of the sinc is c u = num / D: its sine is
taken from num mod 2 D, so a whole number of periods weighs exactly 0. Everything else is the formula as written, np.i0 for I0."""
from math import gcd

import numpy as np

Z = 32
BETA = 12.0


def ratio(rate_in, rate_out):
    ri, ro = int(rate_in), int(rate_out)
    assert ri == rate_in and ro == rate_out and ri > 0 and ro > 0
    g = gcd(ri, ro)
    return ro // g, ri // g                                             # L, M


def n_full(n_in, rate_in, rate_out, lead=0):
    """lead + floor((n_in - 1 + Z / c) L / M) + 1, in integers"""
    L, M = ratio(rate_in, rate_out)
    return lead + ((n_in - 1) * L + Z * max(L, M)) // M + 1


def full_lead(rate_in, rate_out):
    """the whole pre-ringing: ceil(Z max(1, L / M)) frames"""
    L, M = ratio(rate_in, rate_out)
    return -(-Z * max(L, M) // M)


def weights(num, D):
    """c-free part of the kernel, sinc(num / D) K(num / (D Z)), for an int64 array of numerators"""
    x = num.astype(np.float64) / D
    r = np.mod(num, 2 * D)                                                # 0 .. 2 D - 1, exact
    s = np.sin(np.pi * (np.where(r >= D, r - 2 * D, r).astype(np.float64) / D))
    s = np.where(np.mod(num, D) == 0, 0.0, s)
    with np.errstate(divide="ignore", invalid="ignore"):
        sinc = np.where(num == 0, 1.0, s / (np.pi * x))
    v = x / Z
    inside = np.abs(num) < D * Z
    k = np.i0(BETA * np.sqrt(np.where(inside, 1.0 - v * v, 0.0))) / np.i0(BETA)
    return np.where(inside, sinc * k, 0.0)


def resample64(h, rate_in, rate_out, lead=0, cap=None):
    """the fp64 result, before the one rounding to fp32"""
    h = np.asarray(h, np.float64)
    L, M = ratio(rate_in, rate_out)
    D = max(L, M)
    n = n_full(h.size, rate_in, rate_out, lead)
    if cap is not None:
        n = min(n, cap)
    c = min(1.0, L / M)
    out = np.zeros(n, np.float64)
    hp = np.concatenate([h, [0.0]])                                       # index h.size: a tap outside the IR
    width = 2 * Z * D // L + 3
    for i0 in range(0, n, 4096):                                          # (in slices: bounded temporaries)
        a = [(i - lead) * M for i in range(i0, min(n, i0 + 4096))]        # Python integers
        k_lo = np.array([(v - Z * D) // L for v in a], np.int64)
        kk = k_lo[:, None] + np.arange(width, dtype=np.int64)[None, :]    # covers every k with |a - k L| < Z D
        num = np.array(a, np.int64)[:, None] - kk * L
        taps = hp[np.where((kk >= 0) & (kk < h.size), kk, h.size)]
        out[i0:i0 + len(a)] = (M / L) * c * np.sum(taps * weights(num, D), axis=1)
    return out


def resample(h, rate_in, rate_out, lead=0, cap=None):
    return resample64(h, rate_in, rate_out, lead, cap).astype(np.float32)


def dtft(h, rate, freqs, delay=0):
    """H(f) = sum_k h[k] exp(-2 pi j f (k - delay) / rate), fp64"""
    k = np.arange(len(h), dtype=np.float64) - delay
    return np.exp(-2j * np.pi * np.outer(np.asarray(freqs, np.float64), k) / rate) @ np.asarray(h, np.float64)


def noise_ir(n=8192):
    """the spectral checks' IR: decaying noise with a unit first tap"""
    h = np.random.default_rng(3).standard_normal(n) * np.exp(-np.arange(n) / 600.0)
    h[0] = 1.0
    return h.astype(np.float32)
