"""The stream delays' reference (include/aidax.h, "Stream delays"): the rule restated in numpy, independently of the library and not by
the kernel's algorithm. The kernel evaluates a pass in chunks of up to 256 frames, a lane per frame; Reference.process evaluates every
frame on its own, one after the other, with whole-array operations over the playing streams only: the LFO and the read positions in
integers, three gathers per tap, the two interpolations, the damping, the crossfade, the write, the output. numpy rounds every float32
operation once and fuses nothing. (The core takes the frames to evaluate as an index list; process() hands it one frame at a time.
tests/test_delay_host.py also hands it chunks of K frames to show that the kernel's shape is allowed by the rule.)

A line's memory is kept as its last cap + 3 frames; "0 before the line's frame 0" is restated as a memory that is zero after a restart.

signal(), CASES, PLAN1, case() and walk() are the inputs of tests/test_gpu_delay.py, kept here so that tests/test_delay_host.py can hold them
to the conditions that make the GPU comparison mean something."""
import math

import numpy as np

MIN_DELAY, MAX_DELAY, MAX_DEPTH, MAX_FADE = 64, 1 << 18, 4096, 1 << 20
ALL_STREAMS = -1
f32 = np.float32
CLAMP = f32(2.0 ** 64)
STATE_DTYPE = np.dtype([("pos", "<u8"), ("m_cur", "<u4"), ("m_old", "<u4"), ("fade_len", "<u4"), ("fade_left", "<u4"), ("phase", "<u4"), ("replaced", "<u4")])


class Rec:
    """a stream's record: the delay, the modulation depth (Q16 frames) and phase step, the fade length, feedback, damping, wet, dry"""

    def __init__(self, m, depth_q16=0, lfo_step=0, fade=0, fb=0.0, damp=0.0, wet=1.0, dry=1.0):
        self.m, self.depth_q16, self.lfo_step, self.fade = int(m), int(depth_q16), int(lfo_step), int(fade)
        self.fb, self.damp, self.wet, self.dry = f32(fb), f32(damp), f32(wet), f32(dry)

    def but(self, **kw):
        d = dict(m=self.m, depth_q16=self.depth_q16, lfo_step=self.lfo_step, fade=self.fade, fb=self.fb, damp=self.damp, wet=self.wet, dry=self.dry)
        d.update(kw)
        return Rec(**d)

    def reach(self):
        return self.m + ((self.depth_q16 + 0xffff) >> 16)

    def valid(self, cap=MAX_DELAY):
        return (MIN_DELAY <= self.m <= MAX_DELAY and 0 <= self.depth_q16 <= MAX_DEPTH << 16 and 0 <= self.lfo_step < 1 << 32 and 0 <= self.fade <= MAX_FADE
                and abs(self.fb) <= f32(0.98) and 0 <= self.damp <= 0.5 and abs(self.wet) <= 4 and abs(self.dry) <= 4 and self.reach() <= cap)


def _round(v):
    """llround of a non-negative double"""
    return int(math.floor(v + 0.5))


def design(time_ms, feedback, damping, wet, dry, mod_rate_hz, mod_depth_ms, fade_ms, rate):
    """the record by the formulas of aidax_delay_design, in Python floats (IEEE doubles); the parameters are float32 as in aidax_delay_params"""
    time_ms, damping, mod_rate_hz, mod_depth_ms, fade_ms = (float(f32(v)) for v in (time_ms, damping, mod_rate_hz, mod_depth_ms, fade_ms))
    return Rec(_round(time_ms * rate / 1000.0), _round(mod_depth_ms * rate / 1000.0 * 65536.0), _round(mod_rate_hz / rate * 4294967296.0),
               _round(fade_ms * rate / 1000.0), f32(feedback), f32(damping * 0.5), f32(wet), f32(dry))


def sanitise(x):
    x = np.asarray(x, f32)
    return np.clip(np.where(np.isfinite(x), x, f32(0.0)).astype(f32), -CLAMP, CLAMP).astype(f32)


class Reference:
    """the streams of a pool with the stage on: a record or None per stream, whether its control record is enabled, its state, and the
    last cap + 3 frames of its line's memory"""

    def __init__(self, n_streams, cap):
        self.S, self.cap, self.keep = n_streams, cap, cap + 3
        self.rec = [None] * n_streams
        self.enabled = [True] * n_streams
        self.state = np.zeros(n_streams, STATE_DTYPE)
        self.hist = np.zeros((n_streams, self.keep), f32)
        self.fr_nonzero = np.zeros(n_streams, np.int64)          # frames evaluated with fr != 0 (for the host test's conditions)

    def _which(self, stream):
        return range(self.S) if stream == ALL_STREAMS else [stream]

    def reset(self, stream=ALL_STREAMS):
        for s in self._which(stream):
            self.state[s] = 0
            self.hist[s] = 0

    def set(self, stream, rec):
        for s in self._which(stream):
            if rec is not None:
                assert rec.valid(self.cap)
                if self.rec[s] is None:
                    self.reset(s)
            self.rec[s] = rec

    def playing(self, n_active=None):
        return [s for s in range(self.S if n_active is None else n_active) if self.rec[s] is not None and self.enabled[s]]

    # ---- the rule ---------------------------------------------------------------------------------------------------------------------
    def begin(self, on):
        """the first frame of a pass for the streams `on`: the delay in force, a fade from the one before it"""
        for s in on:
            st, r = self.state[s], self.rec[s]
            if st["m_cur"] == 0:
                st["m_cur"] = r.m
            elif r.m != st["m_cur"]:
                st["m_old"], st["m_cur"], st["fade_len"], st["fade_left"] = st["m_cur"], r.m, r.fade, r.fade
            self.state[s] = st

    def frames(self, on, d, x, x_raw, out, ts):
        """frames `ts` (offsets into the pass, an int64 array) of the streams `on`, all read from d as it stands, then written; d is
        [len(on)][keep + n], x the sanitised block"""
        st = self.state[on]
        col = lambda v, dt: np.array(v, dt)[:, None]
        m_cur, m_old = col(st["m_cur"], np.int64), col(st["m_old"], np.int64)
        fade_len, fade_left, phase0 = col(st["fade_len"], np.int64), col(st["fade_left"], np.int64), col(st["phase"], np.int64)
        depth, step = col([self.rec[s].depth_q16 for s in on], np.int64), col([self.rec[s].lfo_step for s in on], np.int64)
        fb, damp = col([self.rec[s].fb for s in on], f32), col([self.rec[s].damp for s in on], f32)
        wet, dry = col([self.rec[s].wet for s in on], f32), col([self.rec[s].dry for s in on], f32)
        t = np.asarray(ts, np.int64)[None, :]
        rows = np.arange(len(on))[:, None]
        phase = (phase0 + t * step) & 0xffffffff
        u = (phase >> 8) & 0xffffff
        tri = np.where(u < 1 << 23, u, (1 << 24) - u)
        off = (depth * tri) >> 23                                # (< 2^51: exact in int64)
        whole, fr = off >> 16, (off & 0xffff).astype(f32) * f32(2.0 ** -16)
        left = np.maximum(fade_left - t, 0)
        at = self.keep + t

        def tap(m):
            i = np.minimum(m + whole, self.cap)
            a, b, c = d[rows, at - i], d[rows, at - i - 1], d[rows, at - i - 2]
            p0 = a + fr * (b - a)
            p1 = b + fr * (c - b)
            return p0 + damp * (p1 - p0)

        f = tap(m_cur)
        fading = left > 0
        if fading.any():
            fo = tap(np.where(fade_left > 0, m_old, m_cur))
            w = ((fade_len - left).astype(np.float64) / np.maximum(fade_len, 1).astype(np.float64)).astype(f32)
            f = np.where(fading, fo + w * (f - fo), f)
        xt = x[:, ts]
        d[rows, at] = xt + fb * f
        out[:, ts] = dry * xt + wet * f
        assert f.dtype == f32 and d.dtype == f32 and out.dtype == f32
        self.fr_nonzero[on] += (fr != 0).sum(axis=1)

    def end(self, on, n, x_raw):
        """behind the pass's last frame"""
        for k, s in enumerate(on):
            st = self.state[s]
            st["pos"] += n
            st["phase"] = (int(st["phase"]) + n * self.rec[s].lfo_step) & 0xffffffff
            st["fade_left"] = max(int(st["fade_left"]) - n, 0)
            st["replaced"] = (int(st["replaced"]) + int((~np.isfinite(x_raw[k])).sum())) & 0xffffffff
            self.state[s] = st

    def process(self, block, n_active=None, chunk=1):
        """the block [S][n] a delayed pass returns where the pass without the stage returns `block`; a pass of no frames moves nothing.
        chunk: frames evaluated from one reading of the memory (1: the restatement; tests/test_delay_host.py also asks for 64 .. 256,
        each held to what the shortest delay in force allows, and None: the kernel's own choice per stream and pass)"""
        block = np.ascontiguousarray(block, f32)
        n = block.shape[1]
        res = block.copy()                                       # (a stream that does not play keeps its bits)
        on = self.playing(n_active)
        if n == 0 or not on:
            return res
        self.begin(on)
        groups = {}
        for s in on:
            st = self.state[s]
            allowed = (min(256, min(int(st["m_cur"]), int(st["m_old"])) if st["fade_left"] else int(st["m_cur"])) // 64) * 64      # the kernel's K
            groups.setdefault(allowed if chunk is None else min(chunk, allowed), []).append(s)
        for k, grp in groups.items():
            x_raw = block[grp]
            x = sanitise(x_raw)
            d = np.concatenate([self.hist[grp], np.zeros((len(grp), n), f32)], axis=1)
            out = np.zeros((len(grp), n), f32)
            for c0 in range(0, n, k):
                self.frames(grp, d, x, x_raw, out, np.arange(c0, min(c0 + k, n)))
            self.hist[grp] = d[:, -self.keep:]
            self.end(grp, n, x_raw)
            res[grp] = out
        return res


def delay(x, rec, cap=None):
    """the whole signal x through a fresh line in one piece, evaluated frame by frame"""
    ref = Reference(1, rec.reach() if cap is None else cap)
    ref.set(0, rec)
    return ref.process(np.asarray(x, f32)[None, :])[0]


# ---- the inputs of the GPU tests -------------------------------------------------------------------------------------------------------
PLAN1 = [1, 3, 0, 63, 64, 65, 257, 4]                            # every tail around the chunks of 64 .. 256 frames, a pass of no frames
MAXF = 257
RATE = 48000.0


def ring_row(cap, max_frames=MAXF):
    row = 1
    while row < cap + 3 + max_frames:
        row <<= 1
    return row


def signal(seed, n, kind="plain"):
    """one stream's samples: noise of +-0.5 and, for "wild", NaN, +Inf and -Inf sprinkled in and 3e38 (clamped to 2^64 by the rule) at
    three fifths of the signal"""
    rng = np.random.default_rng(seed)
    x = rng.uniform(-0.5, 0.5, n).astype(f32)
    if kind == "wild":
        x[7:n:97] = np.nan
        x[11:n:131] = np.inf
        x[13:n:151] = -np.inf
        x[(3 * n) // 5] = f32(3e38)
    return x


def _q16(frames):
    return _round(frames * 65536.0)


def _step(hz):
    return _round(hz / RATE * 4294967296.0)


# (name, capacity, frames, [(from this frame on, the record)]): the bit-for-bit cases. A change is made ahead of the first pass that starts
# at or behind its frame. Stream 0 plays the records as they are, stream 1 with the feedback and the wet level negated.
_STEPS = Rec(64, fade=100, fb=0.6, damp=0.2, wet=0.7, dry=1.0)
_CHORUS = Rec(64, depth_q16=_q16(37.3), lfo_step=_step(40.0), fade=300, fb=0.5, damp=0.1, wet=0.8, dry=0.9)
_LONG = Rec(1000, depth_q16=_q16(90.7), lfo_step=_step(25.0), fade=0, fb=-0.98, damp=0.5, wet=1.0, dry=0.5)
CASES = [
    ("steps", 300, 12000, [(1500 * k, _STEPS.but(m=m)) for k, m in enumerate((64, 300, 65, 255, 256, 257, 128, 191))]),
    ("chorus", 300, 6000, [(2000 * k, _CHORUS.but(m=m)) for k, m in enumerate((64, 200, 64))]),
    ("long", 1100, 9000, [(0, _LONG)]),
]
CASE_STREAMS = 2
SEED = 300


def of_stream(rec, s):
    return rec if s == 0 else rec.but(fb=-rec.fb, wet=-rec.wet)


def case(name):
    """(capacity, the plan, the changes [(frame, record)])"""
    _, cap, T, changes = next(c for c in CASES if c[0] == name)
    plan = PLAN1 * -(-T // sum(PLAN1))
    return cap, plan, changes


def walk(plan, changes):
    """(the pass's first frame, its length, the records that change ahead of it) per pass"""
    at, todo = 0, list(changes)
    for n in plan:
        now = []
        while todo and todo[0][0] <= at:
            now.append(todo.pop(0)[1])
        yield at, n, now
        at += n
    assert not todo


# The mixed case: 70 streams on one launch. Every fifth delay is off, streams 3, 17 and 46 are disabled plugins, the others take their
# delay from the list below (both sides of every chunk switch); every third of them changes to MIXED_M2 ahead of pass MIXED_CHANGE_AT
# with fades of 150 to 470 frames, so that launches find streams in the middle of a fade, and every fourth is modulated.
MIXED_S, MIXED_CAP = 70, 512
MIXED_M = (64, 65, 100, 127, 128, 129, 191, 192, 193, 255, 256, 257, 300, 449)
MIXED_M2 = (257, 64, 128, 300, 65, 192)
MIXED_PLAN = [257, 257, 1, 63, 0, 257, 79] * 3
MIXED_CHANGE_AT = 9
MIXED_DISABLED = (3, 17, 46)


def mixed_rec(s, changed=False):
    if s % 5 == 4:
        return None
    m = MIXED_M2[s % len(MIXED_M2)] if changed and s % 3 == 0 else MIXED_M[s % len(MIXED_M)]
    depth = _q16(1.0 + 3.7 * (s % 7)) if s % 4 == 1 else 0
    return Rec(m, depth, _step(3.0 + s), 150 + 40 * (s % 9), 0.9 - 0.02 * (s % 11) if s % 2 else -0.7, 0.05 * (s % 11), 0.5, 1.0 if s % 3 else 0.0)
