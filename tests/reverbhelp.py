"""The bus reverbs' reference (include/aidax.h, "Bus reverbs"): the rule restated in numpy, independently of the library and not by the
kernel's algorithm. The kernel evaluates a pass in chunks of up to 256 frames, a lane per frame; here every frame is evaluated on its
own, one after the other (chunks of 1), with whole-array float32 operations over [buses][8 lines]: two gathers for the taps, the damping
FIR, the three butterfly stages written out with index lists, the write, the wet sum, the output. numpy rounds every float32 operation
once and fuses nothing.

reverb(x, rec) is the rule over a whole signal from frame 0 on (epoch 0). Reference carries the memories of a pool's buses across
passes: process(raw) returns the block of a reverberated pass whose k_mix produced `raw`. A new epoch is restated as memories that are
zero: set() with other delays or from off, and reset(), clear them.

signal(), CASES and plan_of() are the inputs of tests/test_gpu_bus_reverb.py, kept here so that tests/test_bus_reverb_host.py can hold
them to the conditions that make the GPU comparison mean something."""
import math

import numpy as np

LINES, MIN_DELAY, MAX_DELAY = 8, 64, 32768
ALL_BUSES = -1
f32 = np.float32
CLAMP = f32(2.0 ** 64)
BASE = ((1423, 1637, 1871, 2087, 2311, 2539, 2767, 2999),
        (1493, 1693, 1913, 2129, 2357, 2591, 2803, 2971),
        (1447, 1663, 1889, 2113, 2339, 2557, 2789, 2963),
        (1481, 1709, 1931, 2141, 2371, 2579, 2819, 2953))


class Rec:
    """a bus's record: eight delays, eight gains, damping, wet, dry"""

    def __init__(self, m, gq, a, wet, dry):
        self.m = tuple(int(k) for k in m)
        self.gq = np.asarray(gq, f32)
        self.a, self.wet, self.dry = f32(a), f32(wet), f32(dry)
        assert len(self.m) == LINES and self.gq.shape == (LINES,)

    def valid(self, capacity=MAX_DELAY):
        return (all(MIN_DELAY <= k <= capacity for k in self.m) and bool(((self.gq >= 0) & (self.gq.astype(np.float64) < 1.0 / math.sqrt(8.0))).all())
                and 0 <= self.a <= 0.5 and abs(self.wet) <= 4 and abs(self.dry) <= 4)


def design(rt60_s, size, damping, wet, dry, variant, rate):
    """the record by the formulas of aidax_bus_reverb_design, in Python floats (IEEE doubles); the parameters are float32 as in aidax_bus_reverb_params"""
    rt60, size, damping = float(f32(rt60_s)), float(f32(size)), float(f32(damping))
    m = []
    for base in BASE[variant]:
        k = max(MIN_DELAY, int(math.floor(base * size * rate / 48000.0 + 0.5))) | 1
        while k in m:
            k += 2
        m.append(k)
    gq = [f32(10.0 ** (-3.0 * k / (rt60 * rate)) / math.sqrt(8.0)) for k in m]
    return Rec(m, gq, f32(damping * 0.5), wet, dry)


def sanitise(x):
    x = np.asarray(x, f32)
    return np.clip(np.where(np.isfinite(x), x, f32(0.0)).astype(f32), -CLAMP, CLAMP).astype(f32)


_STAGES = [([i for i in range(LINES) if not i & st], [i + st for i in range(LINES) if not i & st]) for st in (1, 2, 4)]


class Reference:
    """the buses of a pool with the stage on: a record or None per bus, and of every line the last `capacity + 1` frames of its memory"""

    def __init__(self, n_buses, capacity):
        self.B, self.keep = n_buses, capacity + 1
        self.rec = [None] * n_buses
        self.hist = np.zeros((n_buses, LINES, self.keep), f32)
        self.since = [0] * n_buses                               # reverberated frames since the bus's epoch

    def _cut(self, b):
        self.hist[b] = 0
        self.since[b] = 0

    def set(self, bus, rec):
        for b in (range(self.B) if bus == ALL_BUSES else [bus]):
            if rec is not None:
                assert rec.valid(self.keep - 1)
                if self.rec[b] is None or self.rec[b].m != rec.m:
                    self._cut(b)
            self.rec[b] = rec

    def reset(self, bus):
        for b in (range(self.B) if bus == ALL_BUSES else [bus]):
            self._cut(b)

    def process(self, raw):
        """the block [B][n] of a reverberated pass whose raw bus block is `raw`; a pass of no frames moves nothing"""
        raw = np.ascontiguousarray(raw, f32)
        n = raw.shape[1]
        out = raw.copy()                                         # (a bus whose reverb is off keeps its bits)
        on = [b for b in range(self.B) if self.rec[b] is not None]
        if n == 0 or not on:
            return out
        keep = self.keep
        x = sanitise(raw[on])
        m = np.array([self.rec[b].m for b in on], np.int64)
        gq = np.array([self.rec[b].gq for b in on], f32)
        a = np.array([[self.rec[b].a] for b in on], f32)
        wet, dry = np.array([self.rec[b].wet for b in on], f32), np.array([self.rec[b].dry for b in on], f32)
        d = np.concatenate([self.hist[on], np.zeros((len(on), LINES, n), f32)], axis=2)
        res = np.zeros((len(on), n), f32)
        rows, lines = np.arange(len(on))[:, None], np.arange(LINES)[None, :]
        for t in range(n):                                       # frame by frame
            at = keep + t
            s, u = d[rows, lines, at - m], d[rows, lines, at - m - 1]
            f = s + a * (u - s)
            for lo_i, hi_i in _STAGES:
                lo, hi = f[:, lo_i], f[:, hi_i]                  # (copies: an index list gathers)
                f[:, lo_i], f[:, hi_i] = lo + hi, lo - hi
            xt = x[:, t]
            d[:, :, at] = xt[:, None] + gq * f
            w = ((s[:, 0] - s[:, 1]) + (s[:, 2] - s[:, 3])) + ((s[:, 4] - s[:, 5]) + (s[:, 6] - s[:, 7]))
            res[:, t] = dry * xt + wet * w
            assert f.dtype == f32 and w.dtype == f32
        self.hist[on] = d[:, :, -keep:]
        for b in on:
            self.since[b] += n
        out[on] = res
        return out


def reverb(x, rec):
    """the whole signal x from frame 0 on in one piece, evaluated frame by frame"""
    ref = Reference(1, max(rec.m))
    ref.set(0, rec)
    return ref.process(np.asarray(x, f32)[None, :])[0]


# ---- the inputs of the GPU tests -------------------------------------------------------------------------------------------------------
PLAN1 = [1, 3, 0, 63, 64, 65, 257, 4]                            # every tail around the chunks of 64 .. 256 frames, a pass of no frames
MAXF = 257


def ring_row(capacity, max_frames=MAXF):
    row = 1
    while row < capacity + 1 + max_frames:
        row <<= 1
    return row


def signal(seed, n, kind="plain"):
    """one bus's raw samples: noise of +-0.5 and, for "wild", NaN, +Inf and -Inf sprinkled in, 1e6 at frame 200 and 3e38 (clamped to
    2^64 by the rule) at three fifths of the signal"""
    rng = np.random.default_rng(seed)
    x = rng.uniform(-0.5, 0.5, n).astype(f32)
    if kind == "wild":
        x[7:n:97] = np.nan
        x[11:n:131] = np.inf
        x[13:n:151] = -np.inf
        if n > 200:
            x[200] = f32(1e6)
        x[(3 * n) // 5] = f32(3e38)
    return x


def _rec(m, g, a, wet, dry):
    """a record of the tests' own: gains spread around g / sqrt(8)"""
    gq = [f32(g * (1.0 - 0.01 * i) / math.sqrt(8.0)) for i in range(LINES)]
    return Rec(m, gq, a, wet, dry)


def spread(m_min, order=1):
    """eight distinct delays from m_min on, the shortest on the first (order 1) or the last line"""
    m = [m_min + k for k in (0, 1, 3, 5, 7, 9, 13, 15)]
    return m[::order]


# (name, [record per bus], delay capacity): the bit-for-bit cases; bus b is fed by the disabled stream b alone, at unity gain, with
# signal(SEED + b, T, KINDS[b])
CASES = [
    ("smallest", [_rec(spread(64), 0.93, 0.0, 0.5, 1.0), _rec(spread(64, -1), 0.97, 0.25, -0.7, 0.5), _rec([64] * 4 + [70, 79, 64, 66], 0.90, 0.5, 4.0, -4.0)], 128),
    ("edges", [_rec(spread(65), 0.95, 0.1, 0.5, 1.0), _rec(spread(255, -1), 0.96, 0.3, 0.6, 0.8), _rec(spread(256), 0.97, 0.5, -0.5, 1.0), _rec(spread(257, -1), 0.98, 0.0, 1.0, 0.0)], 512),
    ("long", [design(1.0, 1.0, 0.3, 0.4, 1.0, v, 48000.0) for v in (0, 1, 2)], 4096),
]
SEED = 200
KINDS = ("plain", "wild", "plain", "plain")


def plan_of(recs, capacity):
    """PLAN1 repeated until every line's ring row has wrapped twice (frames >= 2 ring rows) and the feedback has gone round eight times
    (frames >= 8 m_max)"""
    need = max(2 * ring_row(capacity), 8 * max(max(r.m) for r in recs if r is not None))
    return PLAN1 * -(-need // sum(PLAN1))


def case(name):
    """(records, capacity, plan, the buses' raw signals [B][T])"""
    _, recs, capacity = next(c for c in CASES if c[0] == name)
    plan = plan_of(recs, capacity)
    T = sum(plan)
    return recs, capacity, plan, np.stack([signal(SEED + b, T, KINDS[b]) for b in range(len(recs))])


# The mixed case: 70 buses on one launch, fed by 12 disabled streams. Bus b < 48 carries send b // 12 of stream b % 12 at unity gain, the
# buses from 48 on are empty; every fifth bus's reverb is off; the others take their shortest delay from the list below.
MIXED_B, MIXED_S, MIXED_CAPACITY = 70, 12, 512
MIXED_MMIN = (64, 65, 100, 127, 128, 129, 191, 192, 193, 255, 256, 257, 300, 497)
MIXED_PLAN = [257, 257, 1, 63, 0, 257, 79] * 3


def mixed_layout():
    """(bus, stream or None, send, record or None) per bus"""
    for b in range(MIXED_B):
        stream, send = (b % MIXED_S, b // MIXED_S) if b < 4 * MIXED_S else (None, None)
        rec = None if b % 5 == 4 else _rec(spread(MIXED_MMIN[b % len(MIXED_MMIN)], 1 if b % 2 else -1), 0.9 + 0.001 * b, 0.05 * (b % 11), 0.5, 1.0 if b % 3 else 0.0)
        yield b, stream, send, rec


def mixed_signal(stream):
    return signal(700 + stream, sum(MIXED_PLAN), "wild" if stream % 4 == 1 else "plain")
