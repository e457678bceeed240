"""The stream delays on the GPU (-m gpu): after every pass the block a pool with the stage returns is, bit for bit, what the numpy
restatement (tests/delayhelp.py: frame by frame, not the kernel's chunks) makes of the block its twin returns, a pool set up the same way
without the stage: the twin's stream block is the delay's input. tests/test_delay_host.py holds the cases to the conditions that every
ring row wraps twice, the feedback goes round eight times, the fades run out across pass boundaries and the LFO turns. No tolerance
anywhere.

Shapes: an LSTM-16 model, max_frames 257 and the ragged block plan 1, 3, 0, 63, 64, 65, 257, 4, repeated (every tail around the kernel's
chunks of 64, 128, 192 and 256 frames; delays of 64, 65, 255, 256 and 257 frames sit on the switches between them)."""
import ctypes as C
import importlib

import numpy as np
import pytest

from tests import conftest, delayhelp as dh, gatehelp as gh, limithelp as lh, mixhelp as mh, modelgen, pool_census, rateref as rr, reverbhelp as rh

pytestmark = pytest.mark.gpu
ax = importlib.import_module("aidadsp-lv2_amd")

ERR_ARG, ERR_STATE = -1, -6
MAXF = dh.MAXF
f32 = np.float32


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def same(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def to_c(rec):
    return ax.DelayRec(rec.m, rec.depth_q16, rec.lfo_step, rec.fade, float(rec.fb), float(rec.damp), float(rec.wet), float(rec.dry), 0)


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    p = str(tmp_path_factory.mktemp("delay") / "lstm16.json")
    modelgen.write_model(modelgen.make_model(kind="lstm", hidden=16, input_size=1, seed=5), p)
    return ax.Model(p)


@pytest.fixture(scope="module")
def skip_model(tmp_path_factory):
    """the same model with in_skip = 1: a non-finite input reaches the output through the skip path (without one the recurrent kernels'
    clamps absorb it, tests/test_gpu_meters.py)"""
    p = str(tmp_path_factory.mktemp("delay") / "lstm16_skip.json")
    modelgen.write_model(modelgen.make_model(kind="lstm", hidden=16, input_size=1, seed=5, in_skip=1), p)
    return ax.Model(p)


def _cuts(x, plan):
    at = 0
    for n in plan:
        yield np.ascontiguousarray(x[:, at:at + n])
        at += n


class Rig:
    """a pool with the delay stage, its twin without it, and the restatement; setup(pool) is applied to both"""

    def __init__(self, model, S, cap, max_frames=MAXF, setup=None):
        self.pool, self.twin = ax.Pool(S, max_frames), ax.Pool(S, max_frames)
        for p in self.both():
            p.set_model(model)
            if setup:
                setup(p)
        self.pool.set_delays(True, cap)
        self.ref, self.S = dh.Reference(S, cap), S
        assert self.pool.delays and not self.twin.delays

    def both(self):
        return self.pool, self.twin

    def delay(self, stream, rec):
        """rec: a delayhelp.Rec or None"""
        self.pool.set_delay_rec(None if rec is None else to_c(rec), stream)
        self.ref.set(stream, rec)

    def reset(self, stream=ax.ALL_STREAMS):
        self.pool.reset_delay(stream)
        self.ref.reset(stream)

    def enable(self, stream, on):
        for p in self.both():
            p.set_controls(ax.default_controls(enabled=1.0 if on else 0.0), stream)
        self.ref.enabled[stream] = on

    def process(self, blk, what=""):
        """one blocking pass through both pools: (the pool's block, the twin's)"""
        dry = self.twin.process(blk)
        want = self.ref.process(dry)
        got = self.pool.process(blk)
        assert same(got, want), f"{what}: a pass of {blk.shape[1]} frames, streams {np.flatnonzero((bits(got) != bits(want)).any(axis=1))}"
        return got, dry

    def check_states(self, what=""):
        got = self.pool.read_delays()
        assert got.tobytes() == self.ref.state.tobytes(), (what, got, self.ref.state)

    def close(self):
        self.pool.close()
        self.twin.close()


@pytest.mark.parametrize("case", [c[0] for c in dh.CASES])
def test_bit_for_bit(model, case):
    cap, plan, changes = dh.case(case)
    S, T = dh.CASE_STREAMS, sum(plan)
    r = Rig(model, S, cap)
    x = modelgen.signal(S, T, seed=dh.SEED)
    outs, dries = [], []
    for at, n, recs in dh.walk(plan, changes):
        for rec in recs:
            for s in range(S):
                r.delay(s, dh.of_stream(rec, s))
                assert r.pool.stream_delay(s)[2] and r.pool.stream_delay(s)[1].m == rec.m
        got, dry = r.process(np.ascontiguousarray(x[:, at:at + n]), f"{case} at frame {at}")
        outs.append(got)
        dries.append(dry)
    out, dry = np.concatenate(outs, axis=1), np.concatenate(dries, axis=1)
    assert out.shape == (S, T) and np.isfinite(out).all() and np.isfinite(dry).all() and np.abs(dry).max() > 1e-3
    for s in range(S):                                           # every delay sounded
        assert int((bits(out[s]) != bits(dh.of_stream(changes[0][1], s).dry * dry[s])).sum()) >= 0.8 * T
    r.check_states(case)
    st = r.pool.read_delays()
    assert (st["pos"] == T).all() and (st["m_cur"] == changes[-1][1].m).all() and (st["fade_left"] == 0).all() and (st["replaced"] == 0).all()
    r.close()


def test_mixed_records_on_one_launch(model):
    """70 streams: delays on both sides of every chunk switch, every fifth delay off, three disabled plugins, a third of the delays
    changed half way with fades of 150 .. 470 frames (launches find them mid-fade), every fourth modulated"""
    S = dh.MIXED_S
    r = Rig(model, S, dh.MIXED_CAP)
    for s in dh.MIXED_DISABLED:
        r.enable(s, False)
    for s in range(S):
        r.delay(s, dh.mixed_rec(s))
    x = modelgen.signal(S, sum(dh.MIXED_PLAN), seed=301)
    mid_fade = 0
    for k, blk in enumerate(_cuts(x, dh.MIXED_PLAN)):
        if k == dh.MIXED_CHANGE_AT:
            for s in range(S):
                r.delay(s, dh.mixed_rec(s, changed=True))
        got, dry = r.process(blk, f"pass {k}")
        if blk.shape[1]:
            off = [s for s in range(S) if dh.mixed_rec(s) is None or s in dh.MIXED_DISABLED]
            assert same(got[off], dry[off])
            mid_fade += int((r.ref.state["fade_left"] > 0).sum())
    assert mid_fade >= 10
    r.check_states("mixed")
    st = r.pool.read_delays()
    assert not st[list(dh.MIXED_DISABLED)]["pos"].any() and (st[[s for s in range(S) if s % 5 != 4 and s not in dh.MIXED_DISABLED]]["pos"] == sum(dh.MIXED_PLAN)).all()
    r.close()


def test_cuts_do_not_show(model):
    """one signal under three block plans, one of them a single block of 8192 frames on a pool sized for it"""
    T, S = 8192, 3
    recs = [dh.Rec(64, fade=0, fb=0.7, damp=0.3, wet=0.6, dry=1.0), dh.Rec(257, dh._q16(20.5), dh._step(11.0), 0, -0.8, 0.1, 1.0, 0.5), dh.Rec(191, fb=0.5, wet=1.0, dry=0.0)]
    x = modelgen.signal(S, T, seed=302)
    plans = [(T, [T]), (MAXF, dh.PLAN1 * 17 + [257, 166]), (200, [200, 57] * 31 + [200, 25])]
    outs = []
    for max_frames, plan in plans:
        assert sum(plan) == T and max(plan) <= max_frames
        r = Rig(model, S, 300, max_frames=max_frames)
        for s in range(S):
            r.delay(s, recs[s])
        outs.append(np.concatenate([r.process(blk, f"plan of {max_frames}")[0] for blk in _cuts(x, plan)], axis=1))
        r.check_states()
        r.close()
    assert same(outs[0], outs[1]) and same(outs[0], outs[2])


def test_an_off_or_disabled_stream_keeps_its_bits_and_its_state(model):
    S = 5
    r = Rig(model, S, 300)
    base = dh.Rec(100, dh._q16(3.3), dh._step(5.0), 50, 0.6, 0.2, 0.7, 1.0)
    r.delay(0, base)
    r.delay(1, base.but(wet=0.0, dry=1.0))                      # wet 0, dry 1: the twin's bits
    r.delay(2, base)                                             # on, and disabled from pass 10 on
    r.delay(3, base)                                             # off from pass 10 on
    # (stream 4: never on)
    plan = dh.PLAN1 * 3
    x = modelgen.signal(S, sum(plan), seed=303)
    frozen = None
    for k, blk in enumerate(_cuts(x, plan)):
        if k == 10:
            r.enable(2, False)
            r.delay(3, None)
            frozen = r.pool.read_delays()[2:4].copy()
            assert frozen["pos"].all()
        got, dry = r.process(blk, f"pass {k}")
        assert same(got[1], dry[1]) and same(got[4], dry[4])
        if k >= 10:
            assert same(got[2:4], dry[2:4]) and r.pool.read_delays()[2:4].tobytes() == frozen.tobytes()
        elif blk.shape[1] > 3 and k > 4:
            assert not same(got[2:4], dry[2:4]) and not same(got[0], dry[0])
    assert r.pool.stream_delay(3)[2] is False and r.pool.stream_delay(2)[2] is True and bytes(r.pool.stream_delay(3)[1]) == bytes(48)
    r.enable(2, True)                                            # enabled again: the line goes on from where it stood
    r.process(x[:, :200].copy(), "enabled again")
    r.check_states()
    assert r.pool.read_delays()[2]["pos"] == frozen[0]["pos"] + 200
    r.close()


def test_changes(model):
    """a change of m fades; a second one inside the fade snaps to the first one's target; gains and LFO keep the line; off -> on,
    reset_delay, reset_stream and the stage going off and on restart it; a fade from a long delay under a record whose depth grows in
    the same change reads the old delay held to the capacity — the restatement agrees throughout"""
    S = 2
    r = Rig(model, S, 600, max_frames=300)
    base = dh.Rec(200, dh._q16(2.5), dh._step(3.0), 500, 0.7, 0.2, 0.8, 1.0)
    other = dh.Rec(64, fb=-0.5, wet=0.5, dry=1.0)
    r.delay(0, base)
    r.delay(1, other)
    n = 300
    deep = base.but(m=100, depth_q16=dh._q16(60.0), lfo_step=dh._step(100.0), fade=400)

    def restarted(got, dry, rec):
        """the first rec.m frames of a fresh line: the memory reads as 0"""
        return same(got[0, :rec.m], (rec.dry * dh.sanitise(dry[0]) + rec.wet * f32(0))[:rec.m])

    steps = [(None, base, False),
             (lambda: r.delay(0, base.but(m=450)), None, False),                                     # a fade of 500 frames begins
             (lambda: r.delay(0, base.but(m=100)), None, False),                                     # 200 frames left: it snaps to 450, a new fade begins
             (None, None, False), (None, None, False),
             (lambda: r.delay(0, base.but(m=100, fb=-0.9, damp=0.5, wet=2.0, dry=0.5, depth_q16=dh._q16(40.0), lfo_step=dh._step(30.0), fade=7)), None, False),
             (lambda: (r.delay(0, None), r.delay(0, base)), base, True),
             (lambda: r.reset(0), base, True),
             (lambda: (r.pool.reset_stream(0), r.twin.reset_stream(0), r.ref.reset(0)), base, True),
             (lambda: (r.pool.set_delays(False), r.pool.set_delays(True, 600), r.ref.reset()), base, True),
             (lambda: r.delay(0, base), base, False),                                                # the same record again: nothing moves
             (lambda: r.delay(0, base.but(m=560, fade=0)), None, False),                             # no fade: the time snaps
             (lambda: r.delay(0, deep), None, False),                                                # 560 -> 100 over 400 frames, 60 frames deep: 560 + 60 > 600
             (None, None, False)]
    x = modelgen.signal(S, n * len(steps), seed=304)
    for k, (blk, (change, rec, restart)) in enumerate(zip(_cuts(x, [n] * len(steps)), steps)):
        if change:
            change()
        if k == 12:                                                                                  # the old delay's read position passes the capacity inside the fade
            ph = (int(r.ref.state[0]["phase"]) + np.arange(deep.fade, dtype=np.int64) * deep.lfo_step) & 0xffffffff
            u = (ph >> 8) & 0xffffff
            whole = (deep.depth_q16 * np.where(u < 1 << 23, u, (1 << 24) - u)) >> 39
            assert r.ref.state[0]["m_cur"] == 560 and int((560 + whole > 600).sum()) >= 50 and int((560 + whole < 600).sum()) >= 50
        got, dry = r.process(blk, f"block {k}")
        r.check_states(f"block {k}")
        st = r.pool.read_delays()[0]
        if k == 1:
            assert (st["m_cur"], st["m_old"], st["fade_len"], st["fade_left"]) == (450, 200, 500, 200)
        if k == 2:
            assert (st["m_cur"], st["m_old"], st["fade_len"], st["fade_left"]) == (100, 450, 500, 200)
        if k == 5:
            assert (st["m_cur"], st["fade_left"]) == (100, 0) and st["pos"] == 6 * n                 # gains, LFO and fade changed: the line went on
        if rec is not None:
            assert restarted(got, dry, rec) == (restart or k == 0), k
        if restart:
            assert st["pos"] == n
    st = r.pool.read_delays()
    assert (st[0]["m_cur"], st[0]["m_old"], st[0]["fade_len"], st[0]["fade_left"]) == (100, 560, 400, 0)
    assert st[1]["pos"] == 5 * n                                                                     # (the stage's restart took the neighbour along)
    r.close()


def test_non_finite(skip_model):
    """a NaN in an enabled stream's input sticks in its input filter and reaches the output through the model's skip path: the twin's
    row is non-finite behind it; a disabled plugin hands NaN and +-Inf through and its line does not play; the delayed rows are finite
    and the restatement's, and `replaced` counts what was replaced"""
    S = 4
    r = Rig(skip_model, S, 300)
    r.enable(1, False)
    for s in range(S):
        r.delay(s, dh.Rec(64 + 31 * s, dh._q16(1.5 * s), dh._step(9.0), 0, 0.9, 0.25, 0.5, 1.0))
    plan = dh.PLAN1 * 4
    T = sum(plan)
    x = modelgen.signal(S, T, seed=305)
    x[0, 700] = np.nan
    x[1] = dh.signal(306, T, "wild")
    x[3, 5:T:211] = np.inf                                       # (a disabled plugin hands these through; an enabled one's model decides)
    outs, dries = [], []
    for k, blk in enumerate(_cuts(x, plan)):
        got, dry = r.process(blk, f"pass {k}")
        outs.append(got)
        dries.append(dry)
    out, dry = np.concatenate(outs, axis=1), np.concatenate(dries, axis=1)
    bad = ~np.isfinite(dry)
    assert bad[0].sum() > 0 and bad[0, :700].sum() == 0 and bad[3].sum() > 0, "the twin's rows hold what the NaN and the Inf made of them"
    assert np.isfinite(out[[0, 2, 3]]).all() and np.isfinite(dry[2]).all()
    st = r.pool.read_delays()
    assert list(st["replaced"][[0, 2, 3]]) == [int(bad[s].sum()) for s in (0, 2, 3)] and st["replaced"][0] > 0 and st["replaced"][2] == 0
    assert same(out[1], dry[1]) and st["replaced"][1] == 0 and st["pos"][1] == 0      # the disabled plugin: a raw copy, the line does not move
    r.enable(1, True)                                            # enabled, the wild row goes through the model; then through the line
    r.process(np.ascontiguousarray(x[:, :257]), "enabled")
    r.check_states()
    r.close()


class _DeviceBlock:
    """a view of device memory for torch.as_tensor"""

    def __init__(self, ptr, shape):
        self.__cuda_array_interface__ = {"shape": shape, "typestr": "<f4", "data": (ptr, False), "version": 2}


def _chain(p):
    """a gate (on stream 4, or on the last one of a smaller pool), meters, an IR, three buses with a reverb and a limiter each"""
    p.set_ir(np.array([0.5, 0.25, -0.125], f32))
    p.set_metering(True)
    p.set_gate(gh.params(**gh.SETS[0]), min(4, p.n_streams - 1))
    p.set_buses(3)
    for s in range(p.n_streams):
        p.set_send(s, 0, s % 3, 1.0 if s < 3 else 0.25, 0)
    p.set_bus_reverbs(True, 128)
    p.set_bus_limiting(True, 64, 100)
    for b, rec in enumerate(rh.CASES[0][1]):
        p.set_bus_reverb_rec(ax.BusReverbRec((C.c_uint32 * 8)(*rec.m), (C.c_float * 8)(*[float(g) for g in rec.gq]), float(rec.a), float(rec.wet), float(rec.dry), 0, 0), b)
    p.set_bus_limiter(ax.BusLimitParams(-20.0, lh.ms(64), lh.ms(100)))


class _Buses:
    """what the bus stages make of the block they are handed: the numpy restatements of k_mix, k_bus_reverb and k_bus_limit in a row"""

    def __init__(self, S):
        self.mix, self.rev, self.lim = mh.Reference(S, 3), rh.Reference(3, 128), lh.Reference(3)
        for s in range(S):
            self.mix.set_send(s, 0, s % 3, 1.0 if s < 3 else 0.25, 0)
        d = ax.bus_limit_design(ax.BusLimitParams(-20.0, lh.ms(64), lh.ms(100)), 48000.0)
        for b, rec in enumerate(rh.CASES[0][1]):
            self.rev.set(b, rec)
            self.lim.set(b, (f32(d.ceiling), d.lookahead, d.hold))

    def process(self, y):
        return self.lim.process(self.rev.process(self.mix.mix(y)))


def test_every_path(model):
    """process, process_device in place and on a caller's stream, submit / collect with a record change between two blocks in flight,
    next to a gate, meters, an IR and the buses with a reverb and a limiter: the stream block is the restatement's over the twin's, and
    the buses and the out meter see the delayed block"""
    import torch
    n, S = 65, 6
    r = Rig(model, S, 300, max_frames=n, setup=_chain)
    buses = _Buses(S)
    recs = [dh.Rec(64 + 40 * s, dh._q16(2.0 * s), dh._step(6.0 + s), 90, 0.8 if s % 2 else -0.8, 0.1 * s, 0.6, 1.0) for s in range(S)]
    for s in range(S):
        r.delay(s, recs[s] if s != 5 else None)
    x = modelgen.signal(S, 16 * n, seed=307)
    blocks = iter(_cuts(x, [n, 64, n, 33, n, n, n, 1, n]))
    peak = np.zeros(S, f32)

    def seen(got):
        """the buses and the out meter behind a pass that returned `got`"""
        assert same(r.pool.read_buses(), buses.process(got))
        np.maximum(peak, np.abs(got).max(axis=1), out=peak)
        m, mt = r.pool.read_meters(), r.twin.read_meters()
        assert np.array_equal(m["out_peak"], peak) and np.array_equal(m["in_peak"], mt["in_peak"])

    for what in ("process", "process, 64 frames"):
        got, _ = r.process(next(blocks), what)
        seen(got)

    # process_device in place, on the pool's stream and on a caller's
    for stream in (None, torch.cuda.Stream()):
        blk = next(blocks)
        want = r.ref.process(r.twin.process(blk))
        d_x = torch.from_numpy(blk).cuda()
        torch.cuda.synchronize()
        if stream is None:
            r.pool.process_device(d_x.data_ptr(), d_x.data_ptr(), blk.shape[1])
            r.pool.sync()
        else:
            with torch.cuda.stream(stream):
                r.pool.process_device(d_x.data_ptr(), d_x.data_ptr(), blk.shape[1], stream.cuda_stream)
            stream.synchronize()
        got = d_x.cpu().numpy()
        assert same(got, want), "process_device"
        seen(got)

    # submit / collect with two blocks in flight, a record changed between them
    b1, b2 = next(blocks), next(blocks)
    r.pool.submit(b1)
    r.pool.set_delay_rec(to_c(recs[0].but(m=250, wet=1.0)), 0)
    r.pool.submit(b2)
    y1, y2 = r.pool.collect(b1.shape[1]), r.pool.collect(b2.shape[1])
    assert same(y1, r.ref.process(r.twin.process(b1)))
    buses.process(y1)                                            # (the restatements follow block by block)
    np.maximum(peak, np.abs(y1).max(axis=1), out=peak)
    r.ref.set(0, recs[0].but(m=250, wet=1.0))
    assert same(y2, r.ref.process(r.twin.process(b2)))
    seen(y2)
    assert r.pool.read_delays()[0]["fade_left"] == 90 - n

    # a pass of no frames, one frame, a whole block: the states agree at the end
    for blk in (next(blocks)[:, :0], next(blocks), next(blocks)):
        got, _ = r.process(blk, "the tail")
        if blk.shape[1]:
            seen(got)
    r.check_states()
    m, mt = r.pool.read_meters(), r.twin.read_meters()
    assert (m["out_peak"][:5] != mt["out_peak"][:5]).all() and m["out_peak"][5] == mt["out_peak"][5]      # (stream 5 has no delay)
    assert r.pool.read_gate().tobytes() == r.twin.read_gate().tobytes()
    r.close()


def test_a_one_stream_zero_copy_pool(model):
    """the blocking round trip of one stream, next to a gate, meters, an IR and the buses: the pass works in pinned host memory and the
    completion word is the queue's"""
    r = Rig(model, 1, 300, max_frames=64, setup=_chain)
    r.delay(0, dh.Rec(64, dh._q16(3.0), dh._step(8.0), 0, 0.8, 0.2, 0.7, 1.0))
    x = modelgen.signal(1, 64 * 12, seed=308)
    for k, blk in enumerate(_cuts(x, [64, 1, 63, 0, 64, 64, 17, 64])):
        r.process(blk, f"zero-copy pass {k}")
    r.delay(0, None)                                             # every delay off: the pass carries its own end markers again
    got, dry = r.process(x[:, :64].copy(), "off")
    assert same(got, dry)
    r.check_states()
    r.close()


def test_under_a_rate_adapter(model):
    """44.1 kHz around a 48 kHz pool, next to a gate, meters, an IR and the buses: the delay works on the pool-rate block between the
    adapter's two stages; against the two stages by hand around a twin pool, with the restatement between the twin and the second
    stage. A change of time falls between two blocks"""
    S, host, rate, cap = 3, 44100, 48000, 300
    blocks = (64, 1, 255, 17, 256, 256, 200)
    a, b, ref = ax.Pool(S, 288, float(rate)), ax.Pool(S, 288, float(rate)), dh.Reference(S, cap)
    for p in (a, b):
        p.set_model(model)
        _chain(p)
    a.set_delays(True, cap)
    recs = [dh.Rec(64 + 70 * s, dh._q16(2.5 * s), dh._step(7.0), 120, 0.8 if s else -0.8, 0.2, 0.7, 1.0) for s in range(S)]
    for s in range(S):
        a.set_delay_rec(to_c(recs[s]), s)
        ref.set(s, recs[s])
    ad = ax.RateAdapter(a, float(host), 256)
    H_A, d_B = rr.delays(host, rate)
    A = ax.Resampler(S, float(host), float(rate), H_A, 0, 256)
    B = ax.Resampler(S, float(rate), float(host), 0, d_B, 288)
    x = modelgen.signal(S, sum(blocks), seed=309)
    frames = rr.pool_frames(blocks, host, rate)
    for k, (blk, m) in enumerate(zip(_cuts(x, blocks), frames)):
        if k == 4:
            a.set_delay_rec(to_c(recs[0].but(m=250)), 0)
            ref.set(0, recs[0].but(m=250))
        got = ad.process(blk)
        dry = b.process(A.process(blk, m))
        want = ref.process(dry)
        assert same(got, B.process(want, blk.shape[1])), f"block {k}"
        assert a.read_delays().tobytes() == ref.state.tobytes(), f"block {k}"
        if k >= 4:
            assert not same(want, dry)
    st = a.read_delays()
    assert (st["pos"] == sum(frames)).all() and sum(frames) > 1100 and (st["m_cur"][0], st["m_old"][0], st["fade_left"][0]) == (250, 64, 0)
    ad.close()
    A.close()
    B.close()
    a.close()
    b.close()


def test_a_prefix_pass(model):
    """the hub's pass over the first n_active streams only, next to a gate, meters, an IR and the buses: the other streams' rows and
    lines do not move. No public call reaches a prefix pass on a pool with delays (hub seats are not covered), so this runs through the
    test build's aidax_test_process_prefix and only there: on the shipped library the path is not covered"""
    if conftest.SHIP_LEG:
        pytest.skip("aidax_test_process_prefix: a test hook — the shipped library has none")
    import torch
    n, S = 65, 6
    r = Rig(model, S, 300, max_frames=n, setup=_chain)
    for s in range(S):
        r.delay(s, dh.Rec(64 + 40 * s, fade=0, fb=0.7, damp=0.1, wet=0.8, dry=1.0))
    x = modelgen.signal(S, 4 * n, seed=310)
    blocks = list(_cuts(x, [n, n, 33, n]))
    hook = ax.lib().aidax_test_process_prefix
    hook.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32]
    r.process(blocks[0], "a whole pass")
    for k, n_active in ((1, 5), (2, 1)):
        blk, ys = blocks[k], []
        for p in r.both():
            d_x = torch.from_numpy(blk).cuda()
            d_y = torch.zeros_like(d_x)
            torch.cuda.synchronize()
            assert hook(p.h, d_x.data_ptr(), d_y.data_ptr(), blk.shape[1], None, n_active) == 0
            p.sync()
            ys.append(d_y.cpu().numpy())
        want = r.ref.process(ys[1], n_active=n_active)
        assert same(ys[0], want) and not ys[0][n_active:].any()
        r.check_states(f"a prefix pass of {n_active} streams")
    r.process(blocks[3], "a whole pass behind them")
    assert list(r.pool.read_delays()["pos"]) == [3 * n + 33] + [3 * n] * 4 + [2 * n]
    r.close()


def test_off_is_free(model):
    """a pool that never enables the stage, one with the stage off and one with every delay off return the twin's bits; by the test
    build's table of HIP calls (tests/pool_census.py reads it) they make exactly the twin's calls pass for pass, only the first
    enabling call allocates, and a delayed pass adds one launch of k_delay and, behind a changed record only, one upload"""
    S, n = 5, 64
    twin, never, off, none_on, on = (ax.Pool(S, n) for _ in range(5))
    pools = (twin, never, off, none_on, on)
    for p in pools:
        p.set_model(model)
    read = None if conftest.SHIP_LEG else pool_census._calls_reader(ax)
    calls = (lambda: {}) if read is None else read
    stable = lambda c: {name: v for name, v in c.items() if name not in pool_census.MAY_VARY}      # (what a poll that runs out of its 2 ms adds)
    calls()
    never.set_delays(False, 300)                                 # off before any on: nothing at all
    assert calls() == {} and not never.delays
    off.set_delays(True, 300)
    c = calls()
    if read:                                                     # the set-up side: ring, records, states; the read's staging and four snapshots
        assert c.get("hipMalloc") == 3 and c.get("hipHostMalloc") == 5 and c.get("hipEventCreateWithFlags") == 4, c
    rec = to_c(dh.Rec(64, fb=0.5, wet=1.0, dry=1.0))
    off.set_delay_rec(rec)
    off.set_delays(False, 0)
    for p in (none_on, on):
        p.set_delays(True, 300)
    none_on.set_delay_rec(rec, 2)
    none_on.set_delay_rec(None, 2)
    on.set_delay_rec(rec, 1)
    calls()
    x = modelgen.signal(S, 6 * n, seed=311)
    for k, blk in enumerate(_cuts(x, [n, n, 0, 17, n])):
        if k == 3:
            on.set_delay(ax.DelayParams(2.0, 0.5, 0.3, 0.5, 1.0, 1.0, 0.1, 5.0), 3)
            assert calls().get("hipMemsetAsync", 0) == (1 if read else 0)      # the restart of stream 3's line, and nothing else
        want = twin.process(blk)
        base = stable(calls())
        for p in (never, off, none_on):
            assert same(p.process(blk), want)
            assert stable(calls()) == base, (k, base)
        got = on.process(blk)
        c = stable(calls())
        if blk.shape[1]:
            assert not same(got[1], want[1]) or k == 0
            assert same(got[[0, 2, 4]], want[[0, 2, 4]])
        if read:
            extra = {name: c.get(name, 0) - base.get(name, 0) for name in set(c) | set(base) if c.get(name, 0) != base.get(name, 0)}
            delayed = {"launch_delay": 1} if blk.shape[1] else {}      # (the completion word of a pass over five streams is the queue's anyway)
            if k in (0, 3):
                delayed.update(hipMemcpyAsync=1, hipEventRecord=1)                                 # the changed records
            assert extra == delayed, (k, extra, base, c)
    for p in pools:
        p.close()


def test_errors(model):
    S = 3
    p = ax.Pool(S, 64)
    p.set_model(model)
    L = ax.lib()

    def code(fn, *a, **kw):
        with pytest.raises(ax.AidaxError) as e:
            fn(*a, **kw)
        return e.value.code

    good = dh.Rec(100, dh._q16(10.0), dh._step(2.0), 50, 0.5, 0.2, 0.5, 1.0)
    params = ax.DelayParams(2.0, 0.5, 0.3, 0.5, 1.0, 1.0, 0.1, 5.0)        # 96 frames at 48 kHz, 4.8 frames deep
    # before the stage's first enabling
    assert code(p.set_delay, params) == ERR_STATE and code(p.set_delay, None, 0) == ERR_STATE and code(p.set_delay_rec, to_c(good), 0) == ERR_STATE
    assert code(p.reset_delay) == ERR_STATE and code(p.read_delays) == ERR_STATE
    pr, rec, on = p.stream_delay(0)
    assert (pr.time_ms, on) == (0.0, False) and bytes(rec) == bytes(48) and code(p.stream_delay, S) == ERR_ARG
    p.set_delays(False, 0)                                       # off before any on: nothing to do, whatever the capacity
    for cap in (0, 63, (1 << 18) + 1, 0xFFFFFFFF):
        assert code(p.set_delays, True, cap) == ERR_ARG, cap
    assert not p.delays and L.aidax_pool_set_delays(None, 1, 300) == ERR_ARG and L.aidax_pool_delays(None) == 0
    p.set_delays(True, 256)
    assert p.delays
    for cap in (255, 257, 64, 1 << 18):
        assert code(p.set_delays, True, cap) == ERR_STATE, cap
    p.set_delays(True, 256)                                      # the same capacity again: fine
    p.set_delays(False, 1)
    assert not p.delays
    p.set_delays(True, 256)
    # refused records change nothing
    p.set_delay(params, 1)
    p.set_delay_rec(to_c(good), 2)
    want = dh.design(2.0, 0.5, 0.3, 0.5, 1.0, 1.0, 0.1, 5.0, 48000.0)
    pr, rec, on = p.stream_delay(1)
    assert on and (rec.m, rec.depth_q16, rec.lfo_step, rec.fade, rec.on) == (want.m, want.depth_q16, want.lfo_step, want.fade, 1) == (96, 314573, 89478, 240, 1)
    assert (pr.time_ms, pr.fade_ms) == (2.0, 5.0)
    pr, rec, on = p.stream_delay(2)
    assert on and rec.m == 100 and pr.time_ms == 0.0

    def state():
        return [(bytes(q), bytes(rec), on) for q, rec, on in (p.stream_delay(s) for s in range(S))]

    def bad(**kw):
        c = to_c(good)
        for k, v in kw.items():
            setattr(c, k, v)
        return c

    before = state()
    assert [s[2] for s in before] == [False, True, True]
    nan = float("nan")
    for stream, rec in ((S, to_c(good)), (-2, to_c(good)), (S, None), (0, bad(m=63)), (0, bad(m=257)), (ax.ALL_STREAMS, bad(m=247)),      # 247 + 10 > 256
                        (1, bad(m=(1 << 18) + 1)), (1, bad(depth_q16=(4096 << 16) + 1)), (1, bad(fade=(1 << 20) + 1)), (1, bad(fb=0.99)), (1, bad(fb=-0.99)),
                        (2, bad(fb=nan)), (0, bad(damp=0.51)), (0, bad(damp=-0.1)), (0, bad(damp=nan)), (0, bad(wet=4.5)), (0, bad(dry=-4.5)),
                        (0, bad(wet=nan)), (0, bad(dry=float("inf")))):
        assert code(p.set_delay_rec, rec, stream) == ERR_ARG, (stream, rec)
    for stream, pr in ((S, params), (-2, params), (S, None), (0, ax.DelayParams(6.0, 0.5, 0.3, 0.5, 1.0, 0.0, 0.0, 0.0)),       # 288 frames: beyond 256
                       (ax.ALL_STREAMS, ax.DelayParams(1.0, 0.5, 0.3, 0.5, 1.0, 0.0, 0.0, 0.0)), (1, ax.DelayParams(2.0, 0.99, 0.3, 0.5, 1.0, 0.0, 0.0, 0.0)),
                       (2, ax.DelayParams(2.0, 0.5, nan, 0.5, 1.0, 0.0, 0.0, 0.0))):
        assert code(p.set_delay, pr, stream) == ERR_ARG, stream
    for stream in (S, -2, 7):
        assert code(p.reset_delay, stream) == ERR_ARG
    out = (ax.DelayStateStruct * S)()
    for first, count in ((0, 0), (S, 1), (1, S), (S + 1, 0)):
        assert L.aidax_pool_read_delays(p.h, first, count, out) == ERR_ARG
    assert L.aidax_pool_read_delays(p.h, 0, S, None) == ERR_ARG and L.aidax_pool_read_delays(None, 0, S, out) == ERR_ARG
    assert state() == before
    assert L.aidax_pool_stream_delay(p.h, 1, None, None, None) == 0
    # a pass, then every delay off: the twin's bits again
    x = modelgen.signal(S, 64, seed=312)
    twin = ax.Pool(S, 64)
    twin.set_model(model)
    assert same(p.process(x), twin.process(x))                  # (the lines are empty: wet * 0)
    y, t = p.process(x), twin.process(x)
    assert same(y[0], t[0]) and not same(y[1], t[1]) and not same(y[2], t[2]) and list(p.read_delays()["pos"]) == [0, 128, 128]
    p.set_delay(None)
    assert same(p.process(x), twin.process(x)) and [s[2] for s in state()] == [False] * S
    p.close()
    twin.close()
