"""Inputs on which the cabinet IR stage (k_ir_conv, aidax_ir_mfma.hip) must be exact to the last bit, and their exact convolutions.

The kernel splits both operands into three bf16 terms (h = h0 + h1 + h2, x = x0 + x1 + x2) and accumulates six of the nine term products
in fp32: (h0 h1 h2) x0, (h0 h1) x1, h0 x2. On the families below the three products it drops (h1 x2, h2 x1, h2 x2) are zero, and every
partial sum of the kept term products that any output can form fits fp32's 24 bits, whatever the order of the additions, the rounding
inside one MFMA, the K split or the reduce. The correct output is then the true convolution bit for bit, and a missing, extra or
misplaced term product changes bits (tests/test_ir_arith.py checks both claims in numpy).

    family  h                                                x                                             term products exercised
    A       dense, L taps of 22 significant bits,            sparse impulses +-2^k, k in [-6, 0], spaced   h0 x0, h1 x0, h2 x0
            magnitudes in [2^-7, 1)                          more than L apart, a random phase per stream
    B       2 - 4 taps of +-1 or +-1/2 at random delays,     dense, k 2^-20 with odd integer |k| < 2^20     h0 x0, h0 x1, h0 x2
            one of them at L - 1
    C       dense, L taps of 11 significant bits             sparse impulses of 11 significant bits,       h0 x0, h1 x0, h0 x1, h1 x1
                                                             spaced more than L apart
    D       L <= 12 taps m 2^-10, 2^9 <= |m| < 2^10          dense, of the same form                       h0 x0, h1 x0, h0 x1, h1 x1

A and C: one input sample reaches each output, so an output is one product (<= 22 + 0 or 11 + 11 significant bits). B: at most four
shifted copies of x scaled by 2^0 or 2^-1, multiples of 2^-21 below 4. D: at most 12 products, multiples of 2^-20 below 1 each.
Every generator returns (h [L], x [S][T], truth [S][T]), all float32; the truths are computed by superposition (exact_conv), no FFT."""
import numpy as np

from tests.test_split_arith import bf16_rne, split3          # noqa: F401  (re-exported: the split the kernel and the packer use)

# the kernel's six term products as (term of h, term of x), in the order it issues them per window
KEPT = ((0, 0), (1, 0), (2, 0), (0, 1), (1, 1), (0, 2))
DROPPED = ((1, 2), (2, 1), (2, 2))
# what each family exercises (tests/test_ir_arith.py holds the families to these claims)
EXERCISES = {"A": ((0, 0), (1, 0), (2, 0)),
             "B": ((0, 0), (0, 1), (0, 2)),
             "C": ((0, 0), (1, 0), (0, 1), (1, 1)),
             "D": ((0, 0), (1, 0), (0, 1), (1, 1))}


def _mantissa(rng, n, bits):
    """n signed odd integers of exactly `bits` significant bits: the last bit set, so that every term of the split carries bits (an odd
    22-bit value has a non-zero third bf16 term, an odd 10- or 11-bit value a non-zero second one)"""
    m = 2 * rng.integers(1 << (bits - 2), 1 << (bits - 1), size=n) + 1
    return np.where(rng.random(n) < 0.5, -m, m)


def _taps(rng, L, bits):
    """L taps of `bits` significant bits, magnitudes in [2^(e-1), 2^e) for e in [-6, 0]"""
    e = rng.integers(-6, 1, size=L)
    return (_mantissa(rng, L, bits) * np.exp2(e - bits).astype(np.float64)).astype(np.float32)


def _impulses(rng, L, S, T, amp):
    """per stream, impulses spaced more than L apart from a random phase; amp(n) draws their values"""
    x = np.zeros((S, T), np.float32)
    n = T // (L + 1) + 1
    for s in range(S):
        p = int(rng.integers(0, L + 1)) + np.concatenate([[0], np.cumsum(L + 1 + rng.integers(0, max(L // 8, 2), size=n - 1))])
        p = p[p < T]
        x[s, p] = amp(p.size)
    return x


def family_a(L, S, T, seed):
    rng = np.random.default_rng([0xA, L, S, T, seed])
    h = _taps(rng, L, 22)
    x = _impulses(rng, L, S, T, lambda n: (np.where(rng.random(n) < 0.5, -1.0, 1.0) * np.exp2(rng.integers(-6, 1, size=n))).astype(np.float32))
    return h, x, exact_conv(h, x)


def family_b(L, S, T, seed):
    rng = np.random.default_rng([0xB, L, S, T, seed])
    n = min(L, int(rng.integers(2, 5)))
    delays = np.concatenate([[L - 1], rng.choice(L - 1, size=n - 1, replace=False)]) if L > 1 else np.array([0])
    h = np.zeros(L, np.float32)
    h[delays] = rng.choice(np.array([1.0, -1.0, 0.5, -0.5], np.float32), size=delays.size)
    k = 2 * rng.integers(-(1 << 19), 1 << 19, size=(S, T)) + 1          # odd: x2 != 0 wherever |k| >= 2^17
    x = (k * 2.0 ** -20).astype(np.float32)
    return h, x, exact_conv(h, x)


def family_c(L, S, T, seed):
    rng = np.random.default_rng([0xC, L, S, T, seed])
    h = _taps(rng, L, 11)
    x = _impulses(rng, L, S, T, lambda n: (_mantissa(rng, n, 11) * np.exp2(rng.integers(-6, 1, size=n) - 11.0)).astype(np.float32))
    return h, x, exact_conv(h, x)


def family_d(L, S, T, seed):
    assert L <= 12, L
    rng = np.random.default_rng([0xD, L, S, T, seed])
    h = (_mantissa(rng, L, 10) * 2.0 ** -10).astype(np.float32)
    x = (_mantissa(rng, S * T, 10) * 2.0 ** -10).astype(np.float32).reshape(S, T)
    return h, x, exact_conv(h, x)


FAMILIES = {"A": family_a, "B": family_b, "C": family_c, "D": family_d}


def exact_conv(h, x):
    """y[s][t] = sum_k h[k] x[s][t - k] (causal, truncated to T), exact on these families: an IR of at most 16 non-zero taps as a sum of
    shifted copies of x in fp64; otherwise x must be impulses spaced at least L apart (one product per output). Asserts the result is
    exact in float32."""
    h64 = h.astype(np.float64)
    S, T = x.shape
    L = h.size
    nz = np.flatnonzero(h64)
    if nz.size <= 16:
        y = np.zeros((S, T), np.float64)
        for k in nz:
            y[:, k:] += h64[k] * x[:, :T - k].astype(np.float64)
    else:
        y32 = np.zeros((S, T), np.float32)
        for s0 in range(0, S, 64):                                    # (in slices of 64 streams: bounded temporaries at S = 1024)
            rows, cols = np.nonzero(x[s0:s0 + 64])
            assert np.all(np.diff(cols)[np.diff(rows) == 0] >= L), "impulses closer than the IR's length"
            # one impulse reaches each output: y[r][c + k] = x[r][c] h[k], k < L
            n = np.minimum(L, T - cols)
            k = np.arange(n.sum()) - np.repeat(np.cumsum(n) - n, n)
            v = np.repeat(x[s0 + rows, cols].astype(np.float64), n) * h64[k]
            y32[s0 + np.repeat(rows, n), np.repeat(cols, n) + k] = v
            assert np.array_equal(y32[s0 + np.repeat(rows, n), np.repeat(cols, n) + k], v), "the truth is not exact in float32"
        return y32
    y32 = y.astype(np.float32)
    assert np.array_equal(y32.astype(np.float64), y), "the truth is not exact in float32"
    return y32
