"""The streaming resampler and the rate adapter (include/aidax.h, "Rate conversion") stated once more, independently, in numpy fp64 on
top of tests/irresample.weights: what tests/test_rate_host.py and tests/test_gpu_rate.py hold the library against. It never calls the
library.

    L / M = rate_out / rate_in in lowest terms, D = max(L, M), c = min(1, L / M), H = ceil(Z D / L), T = 2 H + 1
    a = (j - d_out) M - d_in L,  q = floor(a / L),  phi = a - q L
    out[s][j] = sum_{i = -H .. H} w_phi[i + H] x[s][q - i],   w_phi[i + H] = fp32(c weights(phi + i L, D)),   x[k] = 0 for k < 0

The weights are part of the definition AFTER their one rounding to fp32; the sums here are fp64 (`stage64`). The same function with
absolute weights and samples gives sum |w| |x| per output, the scale of the fp32 dot-product bound."""
import numpy as np

from tests import irresample as rs

Z = rs.Z


def params(rate_in, rate_out):
    """L, M, D, c, H, T"""
    L, M = rs.ratio(rate_in, rate_out)
    D = max(L, M)
    H = -(-Z * D // L)
    return L, M, D, min(1.0, L / M), H, 2 * H + 1


def rows64(rate_in, rate_out):
    """[L][T] in fp64, before the rounding"""
    L, M, D, c, H, T = params(rate_in, rate_out)
    num = np.arange(L, dtype=np.int64)[:, None] + np.arange(-H, H + 1, dtype=np.int64)[None, :] * L
    return c * rs.weights(num, D)


def rows(rate_in, rate_out):
    return rows64(rate_in, rate_out).astype(np.float32)


def ready(n_received, rate_in, rate_out, d_in=0, d_out=0):
    """outputs j with q(j) + H < n_received: j < d_out + ceil((n_received - H + d_in) L / M)"""
    L, M, D, c, H, T = params(rate_in, rate_out)
    return max(0, d_out - (-(n_received - H + d_in) * L // M))


def q_phi(rate_in, rate_out, d_in, d_out, j0, j1):
    """(q, phi) of the outputs j0 .. j1 - 1, int64 arrays: a = (j - d_out) M - d_in L = q L + phi, 0 <= phi < L"""
    L, M = rs.ratio(rate_in, rate_out)
    a = [(j - d_out) * M - d_in * L for j in range(j0, j1)]               # Python integers
    return np.array([v // L for v in a], np.int64), np.array([v % L for v in a], np.int64)


def gamma(T):
    """T u / (1 - T u), u = 2^-24: the bound on the relative error of an fp32 sum of T rounded terms in ANY order (valid while T u < 1;
    the (T + 2) u of the audio-rate tests is this number only for small T)"""
    u = 2.0 ** -24
    return T * u / (1.0 - T * u)


def stage64(x, rate_in, rate_out, d_in, d_out, n_out, absolute=False, first=0):
    """outputs first .. n_out - 1 (first = 0: all of them) of every row of x, fp64 sums over the fp32 weights (absolute: sum |w| |x|
    instead). A long row is evaluated in chunks of outputs through `first`; the values do not depend on the chunking."""
    x = np.atleast_2d(np.asarray(x, np.float64))
    L, M, D, c, H, T = params(rate_in, rate_out)
    assert n_out <= ready(x.shape[1], rate_in, rate_out, d_in, d_out), "a row would reach past the input"
    W = rows(rate_in, rate_out).astype(np.float64)
    if absolute:
        W, x = np.abs(W), np.abs(x)
    q, phi = q_phi(rate_in, rate_out, d_in, d_out, first, n_out)
    k = q[:, None] - np.arange(-H, H + 1, dtype=np.int64)[None, :]        # [n_out][T]: the frame under weight i + H
    xp = np.concatenate([x, np.zeros((x.shape[0], 1))], axis=1)           # last column: a frame before the stream's start
    k = np.where(k >= 0, k, x.shape[1])
    assert k.max(initial=0) <= x.shape[1]
    return np.einsum("jt,sjt->sj", W[phi], xp[:, k])


def delays(host_rate, pool_rate):
    """(H_A, d_B): stage A host -> pool has d_in = H_A, stage B pool -> host d_out = d_B = ceil((H_B + 1) Ma / La)"""
    if host_rate == pool_rate:
        return 0, 0
    H_A = params(host_rate, pool_rate)[4]
    Lb, Mb, _, _, H_B, _ = params(pool_rate, host_rate)                   # Lb / Mb = Ma / La
    return H_A, -(-(H_B + 1) * Lb // Mb)


def latency(host_rate, pool_rate):
    return sum(delays(host_rate, pool_rate))


def pool_frames(blocks, host_rate, pool_rate):
    """m_k = floor(N_k r) - floor(N_{k-1} r) for the host blocks n_k, r = pool_rate / host_rate, in integers"""
    La, Ma = rs.ratio(host_rate, pool_rate)
    out, N = [], 0
    for n in blocks:
        out.append((N + n) * La // Ma - N * La // Ma)
        N += n
    return out


def adapter64(x, host_rate, pool_rate, rel=None):
    """B64(A64(x)) around a transparent pool for the whole of x, and the per-sample bound on an fp32 implementation's distance from it:
    (T_B + 2) 2^-24 (|w_B| o |y|) + |w_B| o ((T_A + 2) 2^-24 (|w_A| o |x|)),   y = A64(x),   o: the stage with absolute weights
    (rel: the relative bound of a T-term sum in place of (T + 2) 2^-24, e.g. `gamma`)"""
    if rel is None:
        rel = lambda T: (T + 2) * 2.0 ** -24
    x = np.atleast_2d(np.asarray(x, np.float64))
    N = x.shape[1]
    H_A, d_B = delays(host_rate, pool_rate)
    La, Ma = rs.ratio(host_rate, pool_rate)
    P = N * La // Ma
    T_A, T_B = params(host_rate, pool_rate)[5], params(pool_rate, host_rate)[5]
    y = stage64(x, host_rate, pool_rate, H_A, 0, P)
    bound_a = rel(T_A) * stage64(x, host_rate, pool_rate, H_A, 0, P, absolute=True)
    out = stage64(y, pool_rate, host_rate, 0, d_B, N)
    bound = rel(T_B) * stage64(y, pool_rate, host_rate, 0, d_B, N, absolute=True) \
        + stage64(bound_a, pool_rate, host_rate, 0, d_B, N, absolute=True)
    return out, bound
