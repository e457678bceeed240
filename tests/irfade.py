"""The IR fade's truth in fp64 (include/aidax.h, "IR fade"): the block a stream must return in the one pass behind a change of its
effective IR, and the envelope its error is held against.

    y[t] = (1 - w[t]) (h_old * x)[t] + w[t] (h_new * x)[t],   w[t] = min(1, (t + 1) / Lf),   Lf = min(F, n)
    E[t] = (1 - w[t]) (|h_old| * |x|)[t] + w[t] (|h_new| * |x|)[t]

x is the stream's dry history including the block (its last n frames are the block); an IR of None is the unit impulse: that side is the
dry block. Host only: numpy, no device."""
import numpy as np


def weights(F, n):
    """w[0 .. n-1] of a pass of n frames under a fade length F >= 1"""
    assert F >= 1 and n >= 1
    lf = min(F, n)
    return np.minimum(1.0, (np.arange(n, dtype=np.float64) + 1.0) / lf)


def conv64(x, h):
    """causal convolution of every row of x ([S][T]) with h in fp64, truncated to T frames; h None: x itself. Short IRs tap by tap
    (exact to fp64 rounding), long ones through the FFT"""
    x = np.asarray(x, np.float64)
    if h is None:
        return x.copy()
    h = np.asarray(h, np.float64)
    T, L = x.shape[1], h.size
    if L <= 64:
        y = np.zeros_like(x)
        for k in range(min(L, T)):
            y[:, k:] += h[k] * x[:, :T - k]
        return y
    nfft = 1 << int(np.ceil(np.log2(T + L)))
    return np.fft.irfft(np.fft.rfft(x, nfft, axis=1) * np.fft.rfft(h, nfft)[None, :], nfft, axis=1)[:, :T]


def expected(x, h_old, h_new, F, n):
    """(y, E), [S][n] each: the fade pass's block and its error envelope for streams of dry history x ([S][T], T >= n)"""
    x = np.asarray(x, np.float64)
    assert x.ndim == 2 and x.shape[1] >= n >= 1
    w = weights(F, n)[None, :]
    ax = np.abs(x)
    old, new = conv64(x, h_old)[:, -n:], conv64(x, h_new)[:, -n:]
    e_old = conv64(ax, None if h_old is None else np.abs(h_old))[:, -n:]
    e_new = conv64(ax, None if h_new is None else np.abs(h_new))[:, -n:]
    return (1.0 - w) * old + w * new, (1.0 - w) * e_old + w * e_new
