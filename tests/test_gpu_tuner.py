"""Stream tuners on the GPU (-m gpu): k_tune against the numpy restatement of the rule (tests/tunehelp.py).

Exact inputs (rows of integers in [-8, 8] / 8: every product and partial sum is an fp32 number) must give the restatement's NSDF row and
reading bit for bit; real signals must stay within TAU + 2^-23 of the fp64 NSDF, give a reading that is the restatement's rules 5 - 8
applied to the kernel's own row, bit for bit, and lie within 1 cent of the string's f0.

`analyses` counts the passes that analysed (rule 1: a pass that crosses several boundaries analyses the last one only), so at a hop
shorter than a block it depends on the cut: the block-cut test holds it to the rule's count for each cut, and to one value for every cut
only at the hop that no block can cross twice. Every other field and the curve are the same bits for every cut at both hops.

A prefix pass (n_active < n_streams) is reached by the hub alone, and the hub never enables the stage: without a test hook there is no
way to it, so it is covered on the host side only (tests/asan_tuner_harness.cpp: the counts of the streams behind the prefix stand)."""
import importlib

import numpy as np
import pytest

from tests import errlog, modelgen, tunehelp as th

pytestmark = pytest.mark.gpu
ax = importlib.import_module("aidadsp-lv2_amd")

SR = 48000.0
TAU = 4e-6                                      # tests/test_gpu_ir.py's bound on the same six-product arithmetic


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    p = str(tmp_path_factory.mktemp("tuner") / "lstm16.json")
    modelgen.write_model(modelgen.make_model(kind="lstm", hidden=16, input_size=1, seed=5), p)
    return ax.Model(p)


def _design(**kw):
    """(the library's TunerParams, the restatement's record) of the same parameters"""
    rec = th.design(SR, **kw)
    assert rec is not None
    got = ax.tuner_design(SR, ax.tuner_params(**kw))
    assert (got.window, got.hop, got.tmin, got.tmax) == (rec["window"], rec["hop"], rec["tmin"], rec["tmax"])
    return ax.tuner_params(**kw), rec


def _pool(model, S, max_frames, params, tuned=True, on=True):
    p = ax.Pool(S, max_frames)
    p.set_model(model)
    if tuned:
        p.set_tuning(params)
        if on:
            p.set_tuner(True)
    return p


def _plan(total, sizes):
    """blocks of `sizes` in turn, the last one cut so that they add up to `total`"""
    out, k = [], 0
    while sum(out) < total:
        out.append(min(sizes[k % len(sizes)], total - sum(out)))
        k += 1
    return out


def _feed(p, x, plan, trackers=None):
    at = 0
    for n in plan:
        blk = np.ascontiguousarray(x[:, at:at + n])
        p.process(blk)
        if trackers is not None:
            for s, tr in enumerate(trackers):
                if tr is not None:
                    tr.feed(blk[s])
        at += n
    assert at == x.shape[1]


def _bits(v):
    return np.asarray(v, np.float32).view(np.uint32)


def _same_reading(got, want, what, level=True):
    fields = ("hz", "period", "clarity") + (("level",) if level else ())
    assert int(got["lag"]) == int(want["lag"]), (what, got, want)
    for f in fields:
        assert _bits(got[f]) == _bits(want[f]), (what, f, got, want)


def _exact_rows(S, n, seed):
    """rows of integers in [-8, 8] / 8: periodic patterns of period 16, 255, 256 and 257 (a peak on both sides of a tile edge), and a
    row without a period; every stream its own"""
    rng = np.random.default_rng(seed)
    rows = []
    for s in range(S):
        period = (16, 255, 256, 257, n)[s % 5]
        pat = rng.integers(-8, 9, period)
        rows.append(np.tile(pat, n // period + 1)[:n])
    return (np.array(rows) / 8.0).astype(np.float32)


@pytest.mark.parametrize("S", [1, 3, 17])
@pytest.mark.parametrize("W", [1024, 2048])
def test_exact_inputs_bit_for_bit(model, W, S):
    tmax = W // 2 - 1
    params, rec = _design(window=W, hop=256, f_min=SR / (tmax - 0.5), f_max=12000.0)
    assert rec["tmax"] == tmax and rec["tmin"] == 4
    p = _pool(model, S, 256, params)
    x = _exact_rows(S, W + 512, seed=1000 + W + S)
    trackers = [th.Tracker(rec) for _ in range(S)]
    at = 0
    for k in range(x.shape[1] // 256):
        _feed(p, x[:, at:at + 256], [256], trackers)
        at += 256
        got = p.read_tuners()
        if at < W:
            assert not got.tobytes().strip(b"\0"), "no reading before the first full window"
            continue
        for s, tr in enumerate(trackers):
            want, n = th.analyse(tr.window, rec, exact=True)
            curve = p.read_tuner_curve(s)
            assert curve.shape == (tmax + 2,)
            bad = np.flatnonzero(_bits(curve) != _bits(n))
            assert bad.size == 0, (W, S, s, at, "first lags that differ", bad[:8], curve[bad[:8]], n[bad[:8]])
            assert (int(got["frame"][s]), int(got["analyses"][s])) == (tr.frame, tr.analyses) == (at, k - W // 256 + 2)
            _same_reading(got[s], want, (W, S, s, at))
    lags = p.read_tuners()["lag"]
    p.close()
    assert (lags > 0).any(), "the periodic rows are voiced"


def test_exact_inputs_at_the_longest_window(model):
    """W = 4096 with tmax = 2047: nine lag tiles, the last one for lag 2048 alone, and more than 64 KiB of LDS (the launch raises the
    kernel's limit). One analysis of two streams: a pattern of period 2047, whose peak is the last lag in range, and one of period 257"""
    W, tmax = 4096, 2047
    params, rec = _design(window=W, hop=4096, f_min=SR / (tmax - 0.5), f_max=12000.0)
    assert rec["tmax"] == tmax
    rng = np.random.default_rng(4096)
    x = (np.array([np.tile(rng.integers(-8, 9, period), W // period + 1)[:W] for period in (2047, 257)]) / 8.0).astype(np.float32)
    p = _pool(model, 2, 1024, params)
    trackers = [th.Tracker(rec) for _ in range(2)]
    _feed(p, x, [1024] * 4, trackers)
    got = p.read_tuners()
    for s, tr in enumerate(trackers):
        want, n = th.analyse(tr.window, rec, exact=True)
        curve = p.read_tuner_curve(s)
        bad = np.flatnonzero(_bits(curve) != _bits(n))
        assert curve.shape == (2049,) and bad.size == 0, (s, bad[:8], curve[bad[:8]], n[bad[:8]])
        assert (int(got["frame"][s]), int(got["analyses"][s])) == (4096, 1)
        _same_reading(got[s], want, s)
    p.close()
    assert int(got["lag"][0]) == 2047 and int(got["lag"][1]) in (257, 514)


@pytest.fixture(scope="module")
def strings():
    """the synthetic strings of the CPU test, one stream each: 10 fundamentals x 4 mixes, 2048 frames"""
    f0 = [f for f in th.FUNDAMENTALS for _ in th.MIXES]
    x = np.stack([th.string(f, th.MIXES[k % 4], 2048, SR, seed=100 * (k // 4) + k % 4) for k, f in enumerate(f0)])
    return f0, x


def test_real_signals(model, strings):
    f0, x = strings
    params, rec = _design()
    S = len(f0)
    p = _pool(model, S, 256, params)
    _feed(p, x, [256] * 8)
    got = p.read_tuners()
    worst_n, worst_c = 0.0, 0.0
    for s in range(S):
        curve = p.read_tuner_curve(s)
        n64 = th.autocorr(x[s], rec["tmax"])
        xs = x[s].astype(np.float64)
        c = np.concatenate([[0.0], np.cumsum(xs * xs)])
        t = np.arange(rec["tmax"] + 2)
        want_n = 2.0 * n64 / (c[2048 - t] + (c[2048] - c[t]))
        err = float(np.abs(curve.astype(np.float64) - want_n).max())
        worst_n = max(worst_n, err)
        want = th.reading(curve, c[2048], rec)
        _same_reading(got[s], want, (s, f0[s]), level=False)
        assert abs(float(got["level"][s]) - float(want["level"])) <= 2.0 ** -23 * float(want["level"])
        assert (int(got["frame"][s]), int(got["analyses"][s])) == (2048, 1)
        cents = abs(th.cents(got["hz"][s], f0[s])) if got["hz"][s] > 0 else float("inf")
        worst_c = max(worst_c, cents)
    p.close()
    print(f"worst |n_gpu - n_fp64| = {worst_n:.3e} (bound {TAU + 2.0 ** -23:.3e}), worst deviation = {worst_c:.3f} cents")
    errlog.bound(worst_n, TAU + 2.0 ** -23, "gpu_tuner_nsdf:strings_w2048")
    assert worst_c <= 1.0


@pytest.mark.parametrize("hop", [64, 272])
def test_block_cuts_do_not_show(model, strings, hop):
    """6000 frames (more than the ring's 2048: it wraps) in blocks of 1, 63, 64, 257 mixed, and in one size throughout"""
    params, rec = _design(window=1024, hop=hop, f_min=100.0)
    S, total = 3, 6000
    rng = np.random.default_rng(7)
    x = np.stack([np.tile(strings[1][5], 3)[:total], np.tile(strings[1][22], 3)[:total], (rng.standard_normal(total) * 0.1).astype(np.float32)])
    x[0] *= np.linspace(1.0, 0.3, total, dtype=np.float32)               # (not periodic in the window's position)
    seen = []
    for sizes in ([1, 63, 64, 257, 257, 1, 64], [257], [64], [63]):
        p = _pool(model, S, 257, params)
        trackers = [th.Tracker(rec) for _ in range(S)]
        marks = []
        for lo, hi in ((0, 3000), (3000, 6000)):
            _feed(p, x[:, lo:hi], _plan(hi - lo, sizes), trackers)
            rd = p.read_tuners()
            assert [int(v) for v in rd["frame"]] == [tr.frame for tr in trackers] == [hi // hop * hop] * S
            assert [int(v) for v in rd["analyses"]] == [tr.analyses for tr in trackers], sizes
            marks.append((rd, [p.read_tuner_curve(s) for s in range(S)]))
        p.close()
        seen.append(marks)
    for marks, sizes in zip(seen[1:], ([257], [64], [63])):
        for (rd, curves), (rd0, curves0) in zip(marks, seen[0]):
            names = [f for f in rd.dtype.names if hop > 257 or f != "analyses"]
            for f in names:
                assert rd[f].tobytes() == rd0[f].tobytes(), (sizes, f, rd, rd0)
            for a, b in zip(curves, curves0):
                assert a.tobytes() == b.tobytes(), sizes
    assert (seen[0][1][0]["hz"][:2] > 0).all()


def test_before_the_first_full_window_and_three_boundaries_in_one_pass(model, strings):
    params, rec = _design(window=1024, hop=64, f_min=100.0)
    p = _pool(model, 2, 256, params)
    x = np.ascontiguousarray(strings[1][[6, 14], :1160])
    trackers = [th.Tracker(rec) for _ in range(2)]
    _feed(p, x[:, :960], [256, 256, 256, 192], trackers)
    assert not p.read_tuners().tobytes().strip(b"\0") and not p.read_tuner_curve(0).any()
    _feed(p, x[:, 960:], [200], trackers)                                 # 960 -> 1160: over 1024, 1088 and 1152
    got = p.read_tuners()
    for s, tr in enumerate(trackers):
        assert (int(got["frame"][s]), int(got["analyses"][s])) == (tr.frame, tr.analyses) == (1152, 1)
        c = np.cumsum(tr.window.astype(np.float64) ** 2)[-1]
        _same_reading(got[s], th.reading(p.read_tuner_curve(s), c, rec), s, level=False)
        assert np.array_equal(tr.window, x[s, 128:1152]) and got["hz"][s] > 0
    p.close()


def test_per_stream_switches(model, strings):
    """off -> on and aidax_pool_reset_stream restart one stream; its neighbours' bits are those of a pool that saw no switch"""
    params, rec = _design(window=1024, hop=256, f_min=100.0)
    S = 5
    x = np.ascontiguousarray(strings[1][[6, 9, 17, 26, 33]])
    a, twin = _pool(model, S, 256, params, on=False), _pool(model, S, 256, params, on=False)
    for s in (0, 1, 2, 4):
        a.set_tuner(True, s)
        twin.set_tuner(True, s)
    assert [a.stream_tuner(s)[0] for s in range(S)] == [True, True, True, False, True]
    trackers = [th.Tracker(rec) if s != 3 else None for s in range(S)]
    _feed(a, x[:, :1280], [256] * 5, trackers)
    _feed(twin, x[:, :1280], [256] * 5)
    assert a.stream_tuner(1) == (True, 1280) and a.stream_tuner(3) == (False, 0)
    a.set_tuner(False, 1)
    a.set_tuner(True, 1)                                                  # restarts: pos = 0
    trackers[1].restart()
    a.reset_stream(2)
    trackers[2].restart()
    a.set_tuner(False, 4)                                                 # off: keeps the reading it has
    kept = a.read_tuners()[4].tobytes()
    trackers[4] = None
    rd = a.read_tuners()
    assert not rd[1].tobytes().strip(b"\0") and not rd[2].tobytes().strip(b"\0") and not a.read_tuner_curve(1).any()
    assert a.stream_tuner(1) == (True, 0) and a.stream_tuner(2) == (True, 0)
    _feed(a, x[:, 1280:1280 + 512], [256, 256], trackers)
    _feed(twin, x[:, 1280:1280 + 512], [256, 256])
    rd = a.read_tuners()
    assert [int(v) for v in rd["analyses"][:3]] == [4, 0, 0] and not rd[1].tobytes().strip(b"\0")
    _feed(a, x[:, 1792:2048], [256], trackers)
    _feed(a, np.ascontiguousarray(x[:, :256]), [256], trackers)           # 1024 frames since the restarts
    _feed(twin, x[:, 1792:2048], [256])
    _feed(twin, np.ascontiguousarray(x[:, :256]), [256])
    rd, rd_twin = a.read_tuners(), twin.read_tuners()
    assert rd[0].tobytes() == rd_twin[0].tobytes() and a.read_tuner_curve(0).tobytes() == twin.read_tuner_curve(0).tobytes()
    assert not rd[3].tobytes().strip(b"\0") and rd[4].tobytes() == kept
    for s in (0, 1, 2):
        tr = trackers[s]
        assert (int(rd["frame"][s]), int(rd["analyses"][s])) == (tr.frame, tr.analyses) == ((2304, 6) if s == 0 else (1024, 1))
        c = np.cumsum(tr.window.astype(np.float64) ** 2)[-1]
        _same_reading(rd[s], th.reading(a.read_tuner_curve(s), c, rec), s, level=False)
        n64, _ = th.nsdf(tr.window, th.autocorr(tr.window, rec["tmax"]), rec["tmax"])
        errlog.bound(np.abs(a.read_tuner_curve(s).astype(np.float64) - n64).max(), TAU + 2.0 ** -23, "gpu_tuner_nsdf:switches_w1024")
    # the stage off: the counts stand, and on again they go on where they were
    a.set_tuning(None)
    _feed(a, np.ascontiguousarray(x[:, :256]), [256])
    assert a.read_tuners().tobytes() == rd.tobytes() and a.stream_tuner(0) == (True, 2304) and not a.tuning()[1]
    a.set_tuning(params)
    assert a.tuning()[1] and a.tuning()[0].tmax == rec["tmax"]
    with pytest.raises(ax.AidaxError):
        a.set_tuning(ax.tuner_params(window=1024, hop=512, f_min=100.0))  # the design is fixed
    a.close()
    twin.close()


def test_one_interior_streams_word_changes_between_two_passes(model):
    """the `on` words reach the device as the range that changed: of 5 streams 3 alone goes on, then 1 alone, then 3 goes off, each
    between two passes of 64 frames (exact rows, window 1024, hop 64: every pass behind a stream's first 1024 frames analyses). After
    every pass each stream's reading and count are the restatement's, bit for bit, and so is the curve at every analysis; a stream that
    no call named reads zeros, and stream 3, once off, keeps the reading it had"""
    W, S, n = 1024, 5, 64
    tmax = W // 2 - 1
    params, rec = _design(window=W, hop=64, f_min=SR / (tmax - 0.5), f_max=12000.0)
    p = _pool(model, S, n, params, on=False)
    x = _exact_rows(S, 2 * W + 4 * n, seed=1300)
    trackers, kept, at = [None] * S, {}, 0

    def passes(count):
        nonlocal at
        for _ in range(count):
            blk = x[:, at:at + n]
            _feed(p, blk, [n], trackers)
            at += n
            got = p.read_tuners()
            for s, tr in enumerate(trackers):
                if tr is None or tr.window is None:
                    assert got[s].tobytes() == kept.get(s, bytes(got[s].nbytes)), (at, s, got[s])
                    continue
                assert (int(got["frame"][s]), int(got["analyses"][s])) == (tr.frame, tr.analyses), (at, s, got[s])
                if tr.frame == tr.pos:                           # (this pass analysed)
                    want, nsdf = th.analyse(tr.window, rec, exact=True)
                    assert np.array_equal(_bits(p.read_tuner_curve(s)), _bits(nsdf)), (at, s)
                    _same_reading(got[s], want, (at, s))
                assert p.stream_tuner(s) == (True, tr.pos)

    p.set_tuner(True, 3)
    trackers[3] = th.Tracker(rec)
    passes(W // n + 1)                                           # stream 3's first two analyses
    p.set_tuner(True, 1)
    trackers[1] = th.Tracker(rec)
    passes(W // n + 1)                                           # ... and stream 1's, 3 going on
    assert (trackers[1].analyses, trackers[3].analyses) == (2, W // n + 3)
    kept[3] = p.read_tuners()[3].tobytes()
    p.set_tuner(False, 3)
    trackers[3] = None
    passes(2)
    assert trackers[1].analyses == 4 and p.stream_tuner(3) == (False, 2 * W + 2 * n) and p.read_tuners()["lag"][1] > 0
    assert [p.stream_tuner(s)[0] for s in range(S)] == [False, True, False, False, False]
    p.close()


def _dressed_pool(model, S, tuned, params):
    """the gate (closing hard), the meters, an IR and the buses on beside the tuners"""
    p = _pool(model, S, 128, params, tuned=tuned)
    p.set_gate(ax.GateParams(-12.0, -14.0, -80.0, 0.5, 1.0, 5.0))
    p.set_metering(True)
    p.set_ir(np.array([0.5, 0.25, 0.0, -0.125], np.float32))
    p.set_buses(2)
    for s in range(S):
        p.set_send(s, 0, s % 2, 0.5)
    return p


def test_no_effect_on_audio_or_on_the_other_stages(model, strings):
    import torch
    params, rec = _design(window=1024, hop=128, f_min=100.0)
    S = 3
    x = np.ascontiguousarray(strings[1][[5, 18, 31], :1536]) * np.float32(0.5)
    a, b = _dressed_pool(model, S, True, params), _dressed_pool(model, S, False, params)
    trackers = [th.Tracker(rec) for _ in range(S)]
    blocks = [np.ascontiguousarray(x[:, k:k + 128]) for k in range(0, 1536, 128)]
    for blk in blocks[:4]:                                                # the blocking path
        assert a.process(blk).tobytes() == b.process(blk).tobytes()
    for blk in blocks[4:8]:                                               # on the device, in place
        d_a, d_b = torch.from_numpy(blk).cuda(), torch.from_numpy(blk).cuda()
        torch.cuda.synchronize()
        a.process_device(d_a.data_ptr(), d_a.data_ptr(), 128)
        b.process_device(d_b.data_ptr(), d_b.data_ptr(), 128)
        a.sync()
        b.sync()
        assert d_a.cpu().numpy().tobytes() == d_b.cpu().numpy().tobytes()
    for k in (8, 10):                                                     # two blocks in flight
        for p in (a, b):
            p.submit(blocks[k])
            p.submit(blocks[k + 1])
        for _ in range(2):
            assert a.collect(128).tobytes() == b.collect(128).tobytes()
    assert a.read_meters().tobytes() == b.read_meters().tobytes() and a.read_buses().tobytes() == b.read_buses().tobytes()
    assert a.read_gate().tobytes() == b.read_gate().tobytes() and a.read_gate()["atten"].max() > 0, "the gate did close"
    # the tuner heard the block the passes were handed: ungated
    for blk in blocks:
        for s, tr in enumerate(trackers):
            tr.feed(blk[s])
    rd = a.read_tuners()
    for s, tr in enumerate(trackers):
        assert (int(rd["frame"][s]), int(rd["analyses"][s])) == (tr.frame, tr.analyses) == (1536, 5)
        n64, _ = th.nsdf(tr.window, th.autocorr(tr.window, rec["tmax"]), rec["tmax"])
        errlog.bound(np.abs(a.read_tuner_curve(s).astype(np.float64) - n64).max(), TAU + 2.0 ** -23, "gpu_tuner_nsdf:dressed_w1024")
    with pytest.raises(ax.AidaxError):
        b.read_tuners()
    a.close()
    b.close()


def test_silence_and_non_finite_input(model, strings):
    params, rec = _design(window=1024, hop=1024, f_min=100.0)
    x = np.zeros((3, 1024), np.float32)
    x[1] = strings[1][8, :1024]
    x[1, 700] = np.nan
    x[2] = strings[1][8, :1024]
    a, twin = _pool(model, 3, 256, params), _pool(model, 3, 256, params)
    _feed(a, x, [256] * 4)
    clean = x.copy()
    clean[1] = 0.0
    _feed(twin, clean, [256] * 4)
    rd, rd_twin = a.read_tuners(), twin.read_tuners()
    assert [int(v) for v in rd["analyses"]] == [1, 1, 1] and [int(v) for v in rd["frame"]] == [1024] * 3
    for s in (0, 1):
        assert (int(rd["lag"][s]), float(rd["hz"][s]), float(rd["period"][s]), float(rd["clarity"][s])) == (0, 0.0, 0.0, 0.0), rd[s]
    assert rd["level"][0] == 0.0 and np.isnan(rd["level"][1]) and not a.read_tuner_curve(0).any() and np.isnan(a.read_tuner_curve(1)).all()
    assert rd[2].tobytes() == rd_twin[2].tobytes() and rd["hz"][2] > 0 and a.read_tuner_curve(2).tobytes() == twin.read_tuner_curve(2).tobytes()
    # the next window is clean again: the NaN left with its frames
    _feed(a, np.ascontiguousarray(strings[1][[8, 8, 8], 1024:2048]), [256] * 4)
    rd = a.read_tuners()
    a.close()
    twin.close()
    assert rd[1].tobytes() == rd[2].tobytes() == rd[0].tobytes() and rd["hz"][1] > 0
