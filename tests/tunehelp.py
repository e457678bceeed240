"""The stream tuners' rule (include/aidax.h, "Stream tuners") restated in numpy, step by step and sequentially: what k_tune's parallel
evaluation is held to. Nothing here is shared with the library: the design, the boundary rule, the NSDF, the walk over the lobes, the
choice and the fp64 interpolation are written out again, and a Tracker follows a stream's frame count and history through any cut of
blocks. Also the synthetic plucked strings of the CPU and the GPU tests."""
import math

import numpy as np

F32 = np.float32
FUNDAMENTALS = [82.41, 110.0, 146.83, 196.0, 246.94, 329.63, 440.0, 659.26, 987.77, 1318.5]      # E2 .. E6
# five partials each; the second one has its fundamental at 0.05 of the second partial
MIXES = [
    [1.0, 0.5, 0.33, 0.25, 0.2],
    [0.05, 1.0, 0.6, 0.4, 0.3],
    [1.0, 0.1, 0.7, 0.05, 0.4],
    [0.6, 1.0, 0.8, 0.5, 0.3],
]


def design(samplerate, window=2048, hop=1024, f_min=70.0, f_max=1400.0, threshold=0.93, clarity_min=0.5, level_min_db=-60.0):
    """aidax_tuner_design, restated: a dict with the record's fields, or None where the header refuses the parameters"""
    if window not in (1024, 2048, 4096) or hop < 64 or hop > 65536 or hop % 16:
        return None
    f_min, f_max, threshold, clarity_min, level_min_db = (F32(v) for v in (f_min, f_max, threshold, clarity_min, level_min_db))
    if not (samplerate > 0 and f_min > 0 and f_max > 0 and f_min <= f_max and 0 < threshold <= 1 and 0 <= clarity_min <= 1 and level_min_db <= 0):
        return None
    tmin, tmax = math.floor(samplerate / float(f_max)), math.ceil(samplerate / float(f_min))
    if tmin < 2 or tmax > window // 2 - 1:
        return None
    level_min = F32(0.0) if level_min_db <= -200 else F32(10.0 ** (float(level_min_db) / 20.0))
    return dict(window=window, hop=hop, tmin=tmin, tmax=tmax, threshold=threshold, clarity_min=clarity_min, level_min=level_min,
                samplerate=float(samplerate))


def crosses(p0, p1, window, hop):
    """rule 1: (does the pass analyse, the boundary b)"""
    b = (p1 // hop) * hop
    return b > p0 and b >= window, b


def autocorr(x, tmax):
    """rule 2 in fp64: r[0 .. tmax + 1]"""
    x = np.asarray(x, np.float64)
    W = len(x)
    return np.array([np.dot(x[:W - t], x[t:]) for t in range(tmax + 2)])


def autocorr_exact(x, tmax, scale=8):
    """rule 2 for rows of integers / scale: the exact sums, as fp32 numbers"""
    xi = np.rint(np.asarray(x, np.float64) * scale).astype(np.int64)
    assert np.array_equal(xi / scale, np.asarray(x, np.float64))
    W = len(xi)
    r = np.array([int(np.dot(xi[:W - t], xi[t:])) for t in range(tmax + 2)], np.int64)
    assert np.abs(r).max() < 1 << 24
    return (r / float(scale * scale)).astype(F32)


def nsdf(x, r, tmax):
    """rules 3 and 4: the fp32 NSDF row from the window and an autocorrelation row (fp64 or fp32), and c[W]"""
    x = np.asarray(x, np.float32).astype(np.float64)
    W = len(x)
    c = np.concatenate([[0.0], np.cumsum(x * x)])
    t = np.arange(tmax + 2)
    m = c[W - t] + (c[W] - c[t])
    with np.errstate(divide="ignore", invalid="ignore"):
        n = ((2.0 * np.asarray(r, np.float64)) / m).astype(F32)
    n[m <= 0] = F32(0.0)
    return n, c[W]


def pick(n, tmin, tmax, k):
    """rules 5 and 6, one lag after the other: (the chosen lag or 0, the key maxima)"""
    last = tmax + 1
    t = 1
    while t <= last and n[t] > 0:
        t += 1
    keys = []
    while t <= last:
        if not n[t] > 0:
            t += 1
            continue
        best = None
        while t <= last and n[t] > 0:
            if tmin <= t <= tmax and n[t] >= n[t - 1] and n[t] > n[t + 1] and (best is None or n[t] > n[best]):
                best = t
            t += 1
        if best is not None:
            keys.append(best)
    if not keys:
        return 0, keys
    nmax = max(n[q] for q in keys)
    bar = F32(k) * F32(nmax)
    for q in keys:
        if n[q] >= bar:
            return q, keys
    raise AssertionError("the largest key maximum passes its own bar")


def reading(n, cW, rec):
    """rules 5 to 8 on an fp32 NSDF row: a dict with lag, hz, period, clarity, level"""
    W = rec["window"]
    q, _ = pick(n, rec["tmin"], rec["tmax"], rec["threshold"])
    with np.errstate(invalid="ignore"):
        level = F32(math.sqrt(cW / W)) if cW == cW else F32(np.nan)
    hz = period = clarity = F32(0.0)
    if q:
        a, b, c = float(n[q - 1]), float(n[q]), float(n[q + 1])
        den = (a - 2.0 * b) + c
        d = (0.5 * (a - c)) / den if den < 0 else 0.0
        pd = q + d
        cl = b - (0.25 * (a - c)) * d
        period, clarity, hz = F32(pd), F32(cl), F32(rec["samplerate"] / pd)
    voiced = q != 0 and not clarity < rec["clarity_min"] and not level < rec["level_min"]
    return dict(lag=q if voiced else 0, hz=hz if voiced else F32(0.0), period=period if voiced else F32(0.0), clarity=clarity, level=level)


def analyse(x, rec, exact=False):
    """the whole analysis of one window: (the reading, the NSDF row)"""
    r = autocorr_exact(x, rec["tmax"]) if exact else autocorr(x, rec["tmax"])
    n, cW = nsdf(x, r, rec["tmax"])
    return reading(n, cW, rec), n


class Tracker:
    """one stream's tuner through its blocks: the frame count, the history, and the window of the last analysis"""

    def __init__(self, rec):
        self.rec = rec
        self.restart()

    def restart(self):
        self.pos, self.hist = 0, np.zeros(0, np.float32)
        self.frame, self.analyses, self.window = 0, 0, None

    def feed(self, row):
        """a pass hands the stream `row`; True when it analyses (self.window is then the window, self.frame its boundary)"""
        row = np.asarray(row, np.float32)
        if len(row) == 0:
            return False
        p0, p1 = self.pos, self.pos + len(row)
        self.hist = np.concatenate([self.hist, row])
        self.pos = p1
        yes, b = crosses(p0, p1, self.rec["window"], self.rec["hop"])
        if yes:
            self.frame, self.analyses = b, self.analyses + 1
            self.window = self.hist[b - self.rec["window"]:b].copy()
        return yes


def string(f0, mix, n_frames, samplerate=48000.0, seed=0, level=0.25, decay_s=1.0, noise_db=-50.0):
    """a plucked string: five harmonic partials in the proportions of `mix`, a slow common decay, white noise noise_db below the
    partials' RMS; fp32"""
    rng = np.random.default_rng(seed)
    t = np.arange(n_frames) / samplerate
    x = np.zeros(n_frames)
    for h, a in enumerate(mix, start=1):
        x += a * np.sin(2.0 * np.pi * h * f0 * t + rng.uniform(0, 2 * np.pi))
    x *= level / math.sqrt(sum(a * a for a in mix) / 2.0)
    rms = math.sqrt(np.mean(x * x))
    x *= np.exp(-t / decay_s)
    x += rng.standard_normal(n_frames) * rms * 10.0 ** (noise_db / 20.0)
    return x.astype(np.float32)


def cents(hz, f0):
    return 1200.0 * math.log2(float(hz) / f0)
