"""The mix buses' reference (include/aidax.h, "Mix buses"): the rule restated in numpy, independently of the library. Gains of ramp
frames in fp64, every operation rounded on its own (numpy's float64 array operations are), then one rounding to float32; float32
products and sums in exactly the normative order: the entries of a bus in ascending (stream, send) order, cut into groups of 32 by
position; a group sum from +0.0f, its terms added in order; the bus sample from +0.0f, the group sums added in group order; a term whose
gain is exactly 0 left out. Plain Python loops over entries: fine at the sizes of the tests.

Reference carries the sends of a pool (bus, ramp, the state behind the last pass) by the rules of aidax_pool_set_send, and mix(y) returns
the bus block of a pass that returned the stream block y and moves the ramps on."""
import numpy as np

SENDS = 4
BUS_NONE = -1
ALL_STREAMS = -1
GROUP = 32
f32 = np.float32


def gain(g0, g1, ramp, k):
    """the gain of ramp frame k, a scalar or an array of frames: fp64 operation by operation, rounded once to float32"""
    g0, g1 = float(f32(g0)), float(f32(g1))
    k = np.asarray(k, np.int64)
    if ramp == 0:
        return np.full(k.shape, f32(g1), f32)
    moving = g0 + (g1 - g0) * (k + 1).astype(np.float64) / float(ramp)
    return np.where(k + 1 >= ramp, f32(g1), moving.astype(f32)).astype(f32)


def sum_entries(rows, gains, n):
    """the bus row of n frames whose entries are (rows[i], gains[i]), in that order: float32 arrays of n frames each"""
    bus = np.zeros(n, f32)
    with np.errstate(all="ignore"):
        for at in range(0, len(rows), GROUP):
            acc = np.zeros(n, f32)
            for y, g in zip(rows[at:at + GROUP], gains[at:at + GROUP]):
                assert y.dtype == f32 and g.dtype == f32
                acc = np.where(g != 0, acc + g * y, acc)
            bus = bus + acc
    assert bus.dtype == f32
    return bus


class Send:
    def __init__(self):
        self.bus = self.played_bus = BUS_NONE
        self.g0 = self.g1 = self.now = f32(0)
        self.len, self.k = 0, 1

    def frames_left(self):
        return max(self.len, 1) - self.k

    def gain_now(self):
        return self.now if self.bus != BUS_NONE and self.bus == self.played_bus else f32(0)


class Reference:
    def __init__(self, n_streams, n_buses):
        self.S, self.B = n_streams, n_buses
        self.sends = [[Send() for _ in range(SENDS)] for _ in range(n_streams)]

    def set_send(self, stream, send, bus, gain=1.0, ramp=0):
        """as aidax_pool_set_send: judged against the state behind the last pass; the same bus ramps from g_now, another one from 0"""
        assert bus == BUS_NONE or 0 <= bus < self.B
        for s in (range(self.S) if stream == ALL_STREAMS else [stream]):
            x = self.sends[s][send]
            x.bus = bus
            x.g0 = x.gain_now()
            x.g1 = f32(0) if bus == BUS_NONE else f32(gain) + f32(0)
            x.len, x.k = ramp, 0
            if x.g0 == x.g1:
                x.len, x.k = 0, 1

    def stream_send(self, stream, send):
        """(bus, gain_now, gain_target, frames_left), as aidax_pool_stream_send"""
        x = self.sends[stream][send]
        return x.bus, float(x.gain_now()), float(x.g1), x.frames_left()

    def entries(self, bus, n_active=None):
        """the (stream, send) pairs on `bus` in the order of the sum"""
        n_active = self.S if n_active is None else n_active
        return [(s, j) for s in range(n_active) for j in range(SENDS) if self.sends[s][j].bus == bus]

    def gains(self, stream, send, n):
        """the float32 gains of the send's next n frames"""
        x = self.sends[stream][send]
        return gain(x.g0, x.g1, x.len, x.k + np.arange(n))

    def mix(self, y, n_active=None, order=None):
        """the bus block [B][n] of a pass that returned y, [S][n]; the sends of the first n_active streams move on. order: {bus: entries},
        another order of a bus's entries (to show that the order matters), which does not move anything"""
        y = np.ascontiguousarray(y, f32)
        n_active = self.S if n_active is None else n_active
        n = y.shape[1]
        out = np.zeros((self.B, n), f32)
        for b in range(self.B):
            es = self.entries(b, n_active) if order is None or b not in order else order[b]
            out[b] = sum_entries([y[s] for s, _ in es], [self.gains(s, j, n) for s, j in es], n)
        if order is None and n:
            for s in range(n_active):
                for x in self.sends[s]:
                    x.played_bus = x.bus
                    x.k += min(n, x.frames_left())
                    x.now = f32(0) if x.bus == BUS_NONE else gain(x.g0, x.g1, x.len, x.k - 1)[()]
        return out
