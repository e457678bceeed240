"""The IR blend's truth (include/aidax.h, "IR blend"): the fp32 weights of a ramp, the one defined output of a frame from exact
rationals, and the fp64 truth and error envelope for data on which the convolutions themselves round.

    ramp frame k of m0 -> m1 over R frames:   k + 1 <  R:  wd = m0 + (m1 - m0) * (k + 1) / R in fp64,  w = (float)wd,  u = (float)(1 - wd)
                                              k + 1 >= R:  w = m1,  u = (float)(1 - (double)m1)
    y = yA where w == 0,  yB where w == 1,  else fmaf(w, yB, (float)(u * yA))

Host only: numpy and integers, no device."""
from fractions import Fraction

import numpy as np

from tests import irfade


def weights(m0, m1, R, k0, n):
    """(w, u), float32 [n] each: ramp frames k0 .. k0 + n - 1 of a ramp from m0 to m1 (rounded to float32 first) over R frames; numpy
    float64 operations in the stated order: one subtraction, one multiplication, one division, one addition"""
    d0, d1 = np.float64(np.float32(m0)), np.float64(np.float32(m1))
    k = np.arange(k0, k0 + n, dtype=np.int64)
    wd = np.full(n, d1, np.float64)
    on = k + 1 < R
    if on.any():
        step = d1 - d0
        run = step * (k[on] + 1).astype(np.float64)
        part = run / np.float64(R)
        wd[on] = d0 + part
    return wd.astype(np.float32), (np.float64(1.0) - wd).astype(np.float32)


class Ramp:
    """one stream's mix by the rules of include/aidax.h, on weights(): set() starts a ramp from the weight of the last frame issued, take(n)
    issues n frames and returns their (w, u); a stream starts at rest on 0"""

    def __init__(self):
        self.m0 = self.m1 = self.now = np.float32(0)
        self.R, self.k = 0, 1

    def set(self, mix, R):
        self.m0, self.m1, self.R, self.k = self.now, np.float32(mix), R, 0
        if self.m0 == self.m1:                                          # a ramp between equal weights has ended when it is set
            self.R, self.k = 0, 1

    def take(self, n):
        w, u = weights(self.m0, self.m1, self.R, self.k, n)
        if n and self.left:
            self.now = w[-1]
        self.k += n
        return w, u

    @property
    def left(self):
        """frames still to be issued until the weight is m1 (a jump, R <= 1, takes one)"""
        return max(max(self.R, 1) - self.k, 0)


def _exact(v):
    """a finite float32 as an exact rational, from its bits"""
    b = int(np.asarray(v, np.float32).view(np.uint32))
    sign, e, m = b >> 31, (b >> 23) & 0xff, b & 0x7fffff
    assert e != 0xff, "not finite"
    q = Fraction(m, 1 << 149) if e == 0 else Fraction((1 << 23) | m, 1) * Fraction(2) ** (e - 150)
    return -q if sign else q


def round32(q):
    """the float32 nearest to the rational q, ties to even, subnormals included, in integer arithmetic; returns its bits as np.uint32.
    An exact zero is +0 (what an IEEE sum of unlike-signed or +0 terms gives under round-to-nearest)"""
    q = Fraction(q)
    if q == 0:
        return np.uint32(0)
    sign = 1 if q < 0 else 0
    a = -q if sign else q
    e = a.numerator.bit_length() - a.denominator.bit_length()           # 2^(e-1) < a < 2^(e+1)
    if a < Fraction(2) ** e:
        e -= 1                                                          # 2^e <= a < 2^(e+1)
    qe = max(e, -126) - 23                                              # the exponent of the last place
    scaled = a / Fraction(2) ** qe
    m, rem = divmod(scaled.numerator, scaled.denominator)
    twice = 2 * rem
    if twice > scaled.denominator or (twice == scaled.denominator and (m & 1)):
        m += 1
    E = qe + 150                                                        # biased exponent of a normal m in [2^23, 2^24)
    assert E <= 254, "overflow"
    # (m < 2^23: a subnormal, E == 1 and the bits are m itself; m == 2^24 carries into the exponent field)
    return np.uint32((sign << 31) | (((E - 1) << 23) + m))


def mix32(w, u, ya, yb):
    """the defined output, float32 of the broadcast shape: yA's bits where w == 0, yB's where w == 1, elsewhere the product u * yA rounded
    to float32, then w * yB + that product rounded ONCE (the fmaf), both from exact rationals"""
    full = np.broadcast_arrays(*(np.asarray(v, np.float32) for v in (w, u, ya, yb)))
    shape = full[0].shape
    w, u, ya, yb = (np.ascontiguousarray(v).ravel() for v in full)
    ba, bb = ya.view(np.uint32), yb.view(np.uint32)
    out = np.where(w == 0, ba, np.where(w == 1, bb, np.uint32(0)))
    cache = {}
    for i in np.flatnonzero((w != 0) & (w != 1) & ((ya != 0) | (yb != 0))):
        key = (float(w[i]), float(u[i]), int(ba[i]), int(bb[i]))
        if key not in cache:
            p = _exact(round32(_exact(u[i]) * _exact(ya[i])).view(np.float32))
            cache[key] = round32(_exact(w[i]) * _exact(yb[i]) + p)
        out[i] = cache[key]
    return out.astype(np.uint32).view(np.float32).reshape(shape)


def expected(x, hA, hB, w, u):
    """(y, E), [S][n] each: the fp64 truth u convA + w convB over the last n frames of the dry histories x ([S][T]) and the envelope
    E = u (|hA| * |x|) + w (|hB| * |x|); w, u: [n] or [S][n]; an IR of None is the unit impulse (tests/irfade.py: conv64)"""
    x = np.asarray(x, np.float64)
    w, u = np.asarray(w, np.float64), np.asarray(u, np.float64)
    n = w.shape[-1]
    assert x.ndim == 2 and x.shape[1] >= n >= 1
    ax = np.abs(x)
    a, b = irfade.conv64(x, hA)[:, -n:], irfade.conv64(x, hB)[:, -n:]
    ea = irfade.conv64(ax, None if hA is None else np.abs(hA))[:, -n:]
    eb = irfade.conv64(ax, None if hB is None else np.abs(hB))[:, -n:]
    return u * a + w * b, u * ea + w * eb
