"""The bus limiters' reference (include/aidax.h, "Bus limiters"): the rule restated in numpy, independently of the library and not by the
kernel's algorithm. Every window is explicit: q per frame, h[m] as the minimum over the W entries q[m - W + 1 .. m], s[n] as the sum over
the L entries h[n - L + 1 .. n] (views of every window side by side, reduced along the window), then one fp64 division rounded to
float32 and one float32 product.

limit(x, C, L, H) is the rule over a whole signal from frame 0 on (x[j] = 0 for j < 0). Reference carries the sample history and the
meter records of a pool's buses across passes: process(raw) returns the bus block of a pass whose k_mix produced `raw`.

signal() and CASES are the inputs of tests/test_gpu_bus_limit.py, kept here so that tests/test_bus_limit_host.py can hold them to the
condition that makes the GPU comparison mean something (every limited bus is limited somewhere, not everywhere, and reaches its
ceiling)."""
import numpy as np
from numpy.lib.stride_tricks import sliding_window_view

U = 1 << 22
ALL_BUSES = -1
LOOKAHEAD_MAX, HOLD_MAX = 512, 4096
f32 = np.float32
METER_DTYPE = np.dtype([("frames", "<u8"), ("passes", "<u8"), ("in_nonfinite", "<u8"), ("limited", "<u8"),
                        ("in_peak", "<f4"), ("out_peak", "<f4"), ("min_gain", "<f4"), ("reserved", "<f4")])


def design(ceiling_db, lookahead_ms, hold_ms, rate):
    """(C, L, H) by the formula of aidax_bus_limit_design, in Python floats (IEEE doubles)"""
    def frames(ms):
        return int(np.floor(float(f32(ms)) * rate / 1000.0 + 0.5))
    return f32(10.0 ** (float(f32(ceiling_db)) / 20.0)), frames(lookahead_ms), frames(hold_ms)


def sanitise(x):
    x = np.asarray(x, f32)
    return np.where(np.isfinite(x), x, f32(0.0)).astype(f32)


def gain_positions(xs, C):
    """q per frame: U where |x| <= C, else floor(((double)C / (double)|x|) * 2^22)"""
    assert xs.dtype == f32
    a = np.abs(xs)
    q = np.full(xs.shape, U, np.int64)
    over = a > f32(C)
    q[over] = np.floor((float(f32(C)) / a[over].astype(np.float64)) * 4194304.0).astype(np.int64)
    return q


def evaluate(xs, C, L, H, n):
    """the rule for the last n frames of the sanitised samples xs (float32), whose frames before xs[0] are zeros: (out, g, s)"""
    assert xs.dtype == f32 and 1 <= L and 0 <= H and n <= len(xs)
    W = L + 1 + H
    pad = 2 * L + H                                              # frames ahead of xs[0] that a window or the delay can reach
    q = np.concatenate([np.full(pad, U, np.int64), gain_positions(xs, C)])
    x = np.concatenate([np.zeros(pad, f32), xs])
    end = len(q)
    h = sliding_window_view(q[end - n - (L - 1) - (W - 1):], W).min(axis=1)        # h[m] for m = first - L + 1 .. last
    s = sliding_window_view(h, L).sum(axis=1)                                        # s[n] for the n frames
    assert len(h) == n + L - 1 and len(s) == n and s.max(initial=0) <= L * U
    g = (s.astype(np.float64) / float(L * U)).astype(f32)
    delayed = x[end - n - L:end - L]
    out = delayed * g
    assert out.dtype == f32
    return out, g, s


def limit(x, C, L, H):
    """the whole signal x from frame 0 on in one piece: (out, g, s)"""
    xs = sanitise(x)
    return evaluate(xs, C, L, H, len(xs))


class Reference:
    """the buses of a pool with the stage on: records (C, L, H) or None per bus, the sanitised history, the meter records"""

    def __init__(self, n_buses, keep=2 * LOOKAHEAD_MAX + HOLD_MAX):
        self.B, self.keep = n_buses, keep
        self.rec = [None] * n_buses
        self.hist = [np.zeros(0, f32) for _ in range(n_buses)]
        self.meters = np.zeros(n_buses, METER_DTYPE)
        self.meters["min_gain"] = 1.0

    def set(self, bus, rec):
        for b in (range(self.B) if bus == ALL_BUSES else [bus]):
            self.rec[b] = None if rec is None else (f32(rec[0]), int(rec[1]), int(rec[2]))

    def latency(self, bus):
        return 0 if self.rec[bus] is None else self.rec[bus][1]

    def read_meters(self, clear=False):
        got = self.meters.copy()
        if clear:
            self.meters[:] = np.zeros(self.B, METER_DTYPE)
            self.meters["min_gain"] = 1.0
        return got

    def process(self, raw):
        """the bus block [B][n] of a limited pass whose raw bus block is `raw`; a pass of no frames moves nothing"""
        raw = np.ascontiguousarray(raw, f32)
        n = raw.shape[1]
        out = np.zeros((self.B, n), f32)
        if n == 0:
            return out
        for b in range(self.B):
            xs = sanitise(raw[b])
            m = self.meters[b]
            m["frames"] += n
            m["passes"] += 1
            m["in_nonfinite"] += int((~np.isfinite(raw[b])).sum())
            peak = np.abs(xs).max()
            m["in_peak"] = max(m["in_peak"], peak)
            self.hist[b] = np.concatenate([self.hist[b], xs])[-(self.keep + n):]
            if self.rec[b] is None:
                out[b] = raw[b]
                m["out_peak"] = max(m["out_peak"], peak)
                continue
            C, L, H = self.rec[b]
            out[b], g, s = evaluate(self.hist[b], C, L, H, n)
            m["out_peak"] = max(m["out_peak"], np.abs(out[b]).max())
            m["limited"] += int((s < L * U).sum())
            m["min_gain"] = min(m["min_gain"], g.min())
        return out


# ---- the inputs of the GPU tests -------------------------------------------------------------------------------------------------------
PLAN = [1, 3, 0, 63, 64, 65, 257, 4] * 2
MAXF = 257
T = sum(PLAN)                                                    # 914 frames


def signal(C, seed, n=T, kind="peaks"):
    """one bus's raw samples, chosen frame by frame: noise below the ceiling and, by kind,
    "peaks": a sample exactly at C (frame 5, ahead of everything else by more than any look-ahead), one ulp above C (530), peaks at
             4 C of both signs (600, 601, 640), 1e6 C (760) and 3e38 (800);
    "quiet": nothing beyond 0.9 C, with C itself at frame 5;
    "wild":  "peaks" with NaN, +Inf and -Inf sprinkled in"""
    C = f32(C)
    rng = np.random.default_rng(seed)
    x = (rng.uniform(-0.4, 0.4, n) * float(C)).astype(f32)
    if n > 5:
        x[5] = C
    if kind == "quiet":
        if n > 300:
            x[300] = f32(-0.9) * C
        return x
    for at, v in ((530, -np.nextafter(C, f32(np.inf))), (600, f32(4) * C), (601, f32(4) * C), (640, f32(-4) * C), (760, f32(1e6) * C), (800, f32(3e38))):
        if at < n:
            x[at] = v
    if kind == "wild":
        x[7:n:97] = np.nan
        x[11:n:131] = np.inf
        x[13:n:151] = -np.inf
    assert x.dtype == f32
    return x


def ms(frames, rate=48000.0):
    """the time, as the float32 of aidax_bus_limit_params, that designs to `frames` at `rate`"""
    return float(f32(frames * 1000.0 / rate))


# (name, ceiling_db, [(L, H) per bus], (look-ahead capacity, hold capacity)): the bit-for-bit cases of three buses, bus b fed by the
# disabled stream b alone, at unity gain, with signal(C, SEEDS[b], kind=KINDS[b])
CASES = [
    ("smallest", -6.0, [(1, 0), (2, 0), (64, 0)], (64, 0)),
    ("crossing", -3.0, [(63, 1), (65, 100), (512, 4096)], (512, 4096)),
]
SEEDS, KINDS = (101, 102, 103), ("peaks", "wild", "peaks")


# The mixed case: 70 buses on one launch, fed by 12 disabled streams. Bus b < 48 carries send b // 12 of stream b % 12 at unity gain, the
# buses from 48 on are empty; every fifth bus's limiter is off; the others take their look-ahead and hold from the lists below and their
# ceiling from their stream (a stream's signal is built around one ceiling).
MIXED_B, MIXED_S = 70, 12
MIXED_LS, MIXED_HS, MIXED_DBS = (1, 2, 3, 7, 63, 64, 65, 200, 512), (0, 1, 5, 100, 1000, 4096), (-60.0, -20.0, -6.0, 0.0, 12.0)


def mixed_layout():
    """(bus, stream or None, send, (ceiling_db, L, H) or None) per bus"""
    for b in range(MIXED_B):
        stream, send = (b % MIXED_S, b // MIXED_S) if b < 4 * MIXED_S else (None, None)
        db = MIXED_DBS[(b % MIXED_S) % len(MIXED_DBS)]
        yield b, stream, send, (None if b % 5 == 4 else (db, MIXED_LS[b % len(MIXED_LS)], MIXED_HS[b % len(MIXED_HS)]))


def mixed_signal(stream, ceiling_of_db):
    return signal(ceiling_of_db(MIXED_DBS[stream % len(MIXED_DBS)]), 500 + stream, kind="wild" if stream % 2 else "peaks")


def mixed_buses(ceiling_of_db):
    """(bus, its raw signal or None for an empty bus, (C, L, H) or None for a limiter that is off) per bus"""
    for b, stream, _, rec in mixed_layout():
        yield b, (None if stream is None else mixed_signal(stream, ceiling_of_db)), (None if rec is None else (ceiling_of_db(rec[0]), rec[1], rec[2]))
