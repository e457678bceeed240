"""The stream delays, the parts that need no device: aidax_delay_design against an fp64 restatement and its error cases; the numpy
restatement of the rule (tests/delayhelp.py) on an impulse; that the rule allows the kernel's shape (chunks of K frames read from the
memory as it stood before the chunk equal the frame-by-frame evaluation, bit for bit, on every GPU case); and the conditions the GPU
cases of tests/test_gpu_delay.py rest on, so that none of them can pass vacuously."""
import importlib

import numpy as np
import pytest

from tests import delayhelp as dh

ax = importlib.import_module("aidadsp-lv2_amd")
f32 = np.float32
ERR_ARG = -1


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def test_the_entry_points_and_constants():
    for name in ("aidax_delay_design", "aidax_pool_set_delays", "aidax_pool_delays", "aidax_pool_set_delay", "aidax_pool_set_delay_rec", "aidax_pool_stream_delay",
                 "aidax_pool_read_delays", "aidax_pool_reset_delay"):
        assert name in ax.declared_symbols() and hasattr(ax.lib(), name), name
    assert (ax.DELAY_MIN, ax.DELAY_MAX) == (dh.MIN_DELAY, dh.MAX_DELAY) == (64, 1 << 18)
    import ctypes as C
    assert C.sizeof(ax.DelayRec) == 48 and C.sizeof(ax.DelayStateStruct) == 32 == ax.DelayState.itemsize == dh.STATE_DTYPE.itemsize and C.sizeof(ax.DelayParams) == 32
    with open(f"{dh.__file__.rsplit('/tests/', 1)[0]}/include/aidax.h") as f:
        threads = f.read().split("/* Threads.")[1].split("*/")[0]
    for word in ("set_delay,", "set_delay_rec", "reset_delay", "read_delays", "aidax_pool_set_delays", "aidax_delay_design"):
        assert word in threads, word


@pytest.mark.parametrize("rate", [44100.0, 48000.0, 96000.0])
def test_design_against_the_fp64_restatement(rate):
    rng = np.random.default_rng(7)
    for _ in range(200):
        p = (rng.uniform(2.0, 900.0), rng.uniform(-0.98, 0.98), rng.uniform(0, 1), rng.uniform(-4, 4), rng.uniform(-4, 4), rng.uniform(0, 50.0),
             rng.uniform(0, 20.0), rng.uniform(0, 500.0))
        got, want = ax.delay_design(ax.DelayParams(*p), rate), dh.design(*p, rate)
        assert (got.m, got.depth_q16, got.lfo_step, got.fade, got.on) == (want.m, want.depth_q16, want.lfo_step, want.fade, 1)
        assert (f32(got.fb), f32(got.damp), f32(got.wet), f32(got.dry)) == (want.fb, want.damp, want.wet, want.dry) and tuple(got.reserved) == (0, 0, 0)
        assert want.valid()
    edge = ax.delay_design(ax.DelayParams(64000.0 / rate, 0.98, 1.0, 4.0, -4.0, 0.0, 0.0, 0.0), rate)
    assert (edge.m, edge.depth_q16, edge.lfo_step, edge.fade, edge.damp) == (64, 0, 0, 0, 0.5)


def test_design_errors():
    good = dict(time_ms=10.0, feedback=0.5, damping=0.3, wet=0.5, dry=1.0, mod_rate_hz=1.0, mod_depth_ms=1.0, fade_ms=20.0)
    nan, inf = float("nan"), float("inf")

    def code(rate=48000.0, **kw):
        with pytest.raises(ax.AidaxError) as e:
            ax.delay_design(ax.DelayParams(**dict(good, **kw)), rate)
        return e.value.code

    ax.delay_design(ax.DelayParams(**good), 48000.0)
    for kw in (dict(time_ms=1.3), dict(time_ms=0.0), dict(time_ms=-5.0), dict(time_ms=5462.0), dict(time_ms=1e30), dict(time_ms=nan), dict(time_ms=inf),
               dict(feedback=0.99), dict(feedback=-0.99), dict(feedback=nan), dict(damping=-0.1), dict(damping=1.1), dict(damping=nan),
               dict(wet=4.5), dict(dry=-4.5), dict(wet=nan), dict(dry=inf), dict(mod_rate_hz=-1.0), dict(mod_rate_hz=1001.0), dict(mod_rate_hz=nan),
               dict(mod_depth_ms=-0.1), dict(mod_depth_ms=86.0), dict(mod_depth_ms=nan), dict(mod_depth_ms=1e30), dict(fade_ms=-1.0), dict(fade_ms=21900.0),
               dict(fade_ms=nan), dict(fade_ms=1e30)):
        assert code(**kw) == ERR_ARG, kw
    for rate in (0.0, -48000.0, nan, inf):
        assert code(rate=rate) == ERR_ARG, rate
    assert code(rate=1000.0, mod_rate_hz=501.0, time_ms=100.0) == ERR_ARG           # above half the samplerate
    L = ax.lib()
    out = ax.DelayRec()
    assert L.aidax_delay_design(None, 48000.0, out) == ERR_ARG and L.aidax_delay_design(ax.DelayParams(**good), 48000.0, None) == ERR_ARG
    assert bytes(out) == bytes(48)                                                  # a refused call leaves `out` alone


def test_an_impulse_echoes_in_exact_halves():
    m = 100
    x = np.zeros(5 * m + 7, f32)
    x[0] = 1.0
    y = dh.delay(x, dh.Rec(m, fb=0.5, damp=0.0, wet=1.0, dry=0.0))
    want = np.zeros_like(x)
    for k in range(1, 6):
        want[k * m] = 0.5 ** (k - 1)
    assert np.array_equal(bits(y), bits(want))


def test_dry_alone_returns_the_bits_and_the_line_stays_finite_under_the_largest_input():
    x = dh.signal(5, 3000)
    y = dh.delay(x, dh.Rec(64, dh._q16(9.5), dh._step(7.0), 0, 0.98, 0.5, 0.0, 1.0))
    assert np.array_equal(bits(y), bits(x))
    ref = dh.Reference(1, 70)
    ref.set(0, dh.Rec(64, 0, 0, 0, 0.98, 0.0, 4.0, 4.0))
    big = np.full((1, 64 * 600), 3e38, f32)
    y = ref.process(big, chunk=64)
    assert np.isfinite(y).all() and np.abs(y).max() < 2.0 ** 72 and np.abs(ref.hist).max() < 2.0 ** 70 and y[0, -1] > 2.0 ** 71


def test_the_old_delay_of_a_fade_is_held_to_the_capacity():
    """560 -> 100 over 400 frames under a record whose depth grows to 60 frames in the same change, capacity 600: the old delay's read
    position would pass the capacity, the rule holds it there, and chunks still equal the frame-by-frame evaluation"""
    x = dh.signal(9, 1500)
    outs = []
    for chunk in (1, None):
        ref = dh.Reference(1, 600)
        ref.set(0, dh.Rec(560, fb=0.7, damp=0.2, wet=0.8, dry=1.0))
        y0 = ref.process(x[None, :900], chunk=chunk)
        deep = dh.Rec(100, dh._q16(60.0), dh._step(100.0), 400, 0.7, 0.2, 0.8, 1.0)
        ref.set(0, deep)
        outs.append(np.concatenate([y0, ref.process(x[None, 900:1200], chunk=chunk), ref.process(x[None, 1200:], chunk=chunk)], axis=1))
        assert tuple(ref.state[0])[1:5] == (100, 560, 400, 0)
    assert np.array_equal(bits(outs[0]), bits(outs[1]))
    free = dh.Reference(1, 700)                                  # the same line with room for 560 + 60: other bits inside the fade only
    free.set(0, dh.Rec(560, fb=0.7, damp=0.2, wet=0.8, dry=1.0))
    z = [free.process(x[None, :900])]
    free.set(0, deep)
    z.append(free.process(x[None, 900:]))
    differs = bits(np.concatenate(z, axis=1))[0] != bits(outs[0])[0]
    assert not differs[:900].any() and differs[900:1300].sum() >= 50


def _run(name, s, chunk, x):
    """stream s of the case over the signal x, cut by the case's plan: (the output, the reference, facts about the fades)"""
    cap, plan, changes = dh.case(name)
    ref = dh.Reference(1, cap)
    outs, in_fade, left_at_change = [], 0, []
    for at, n, recs in dh.walk(plan, changes):
        for r in recs:
            left_at_change.append(int(ref.state[0]["fade_left"]))
            ref.set(0, dh.of_stream(r, s))
        outs.append(ref.process(x[None, at:at + n], chunk=chunk)[0])
        if n and ref.state[0]["fade_left"] > 0:
            in_fade += 1                                         # the boundary behind this pass falls inside a fade
    return np.concatenate(outs), ref, in_fade, left_at_change


@pytest.fixture(scope="module")
def frame_by_frame():
    out = {}
    for name, _, _, _ in dh.CASES:
        _, plan, _ = dh.case(name)
        for s in range(dh.CASE_STREAMS):
            x = dh.signal(dh.SEED + s, sum(plan), "wild" if s == 1 else "plain")
            out[name, s] = (x,) + _run(name, s, 1, x)
    return out


@pytest.mark.parametrize("chunk", [64, 128, 192, 256, None])
@pytest.mark.parametrize("name", [c[0] for c in dh.CASES])
def test_chunks_of_independent_frames_equal_the_frame_by_frame_rule(frame_by_frame, name, chunk):
    """chunk: the K asked for, held per pass to what the shortest delay in force allows; None: the kernel's choice per pass"""
    for s in range(dh.CASE_STREAMS):
        x, want, ref, _, _ = frame_by_frame[name, s]
        got, ref_k, _, _ = _run(name, s, chunk, x)
        assert np.array_equal(bits(got), bits(want)) and ref_k.state.tobytes() == ref.state.tobytes() and np.array_equal(bits(ref_k.hist), bits(ref.hist))


@pytest.mark.parametrize("name", [c[0] for c in dh.CASES])
def test_the_conditions_the_gpu_cases_rest_on(frame_by_frame, name):
    cap, plan, changes = dh.case(name)
    T = sum(plan)
    assert T >= 2 * dh.ring_row(cap), "every ring row wraps at least twice"
    assert dh.ring_row(300) == 1024 and dh.ring_row(1100) == 2048
    assert all(r.valid(cap) for _, r in changes)
    modulated = changes[0][1].depth_q16 != 0
    for s in range(dh.CASE_STREAMS):
        x, y, ref, in_fade, left_at_change = frame_by_frame[name, s]
        assert np.isfinite(y).all() and ref.state[0]["pos"] == T
        assert T >= 8 * max(r.m for _, r in changes), "the feedback goes round at least 8 times"
        dry = dh.of_stream(changes[0][1], s).dry * dh.sanitise(x)
        assert int((bits(y) != bits(dry)).sum()) >= 0.8 * T, "at least 80 % of the output differs from dry * x"
        assert all(left == 0 for left in left_at_change) and ref.state[0]["fade_left"] == 0, "every fade runs to its end"
        if len(changes) > 1 and changes[0][1].fade:
            assert in_fade >= 5, f"{in_fade} pass boundaries inside a fade"
        if modulated:
            assert T * changes[0][1].lfo_step >= 2 << 32, "the LFO completes two periods"
            assert 2 * ref.fr_nonzero[0] >= T, "fr != 0 on at least half the frames"
        if s == 1:
            assert ref.state[0]["replaced"] == int((~np.isfinite(x)).sum()) > 10


def test_the_mixed_case_stands_on_both_sides_of_every_chunk_switch():
    recs = [dh.mixed_rec(s) for s in range(dh.MIXED_S)]
    ms = {r.m for r in recs if r is not None}
    assert {64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 257} <= ms
    assert all(r is None or r.valid(dh.MIXED_CAP) for r in recs) and all(r is None or r.valid(dh.MIXED_CAP) for r in (dh.mixed_rec(s, True) for s in range(dh.MIXED_S)))
    assert sum(r is None for r in recs) == 14 and all(recs[s] is not None for s in dh.MIXED_DISABLED)
    changed = [s for s in range(dh.MIXED_S) if recs[s] is not None and dh.mixed_rec(s, True).m != recs[s].m]
    assert len(changed) >= 10
    # ... and at least one launch finds a stream in the middle of a fade
    first = sum(dh.MIXED_PLAN[:dh.MIXED_CHANGE_AT + 1])
    assert any(recs[s].fade > sum(dh.MIXED_PLAN[dh.MIXED_CHANGE_AT:dh.MIXED_CHANGE_AT + 4]) for s in changed) and first < sum(dh.MIXED_PLAN)
