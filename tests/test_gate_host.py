"""The noise gate, host side (no device): aidax_gate_design's record (integers exact, thresholds within an ulp of the fp64 value rounded
by numpy), every refusal with its message, the three structs' layouts as the binding sees them, and the pool calls' answers for a null
pool."""
import ctypes as C
import importlib
import math

import numpy as np
import pytest

ax = importlib.import_module("aidadsp-lv2_amd")

ERR_ARG = -1
P = 1 << 24


def _params(**kw):
    base = dict(open_db=-20.0, close_db=-30.0, floor_db=-40.0, attack_ms=1.0, hold_ms=10.0, release_ms=50.0)
    base.update(kw)
    return ax.GateParams(**base)


def test_the_structs_are_the_headers():
    assert (C.sizeof(ax.GateParams), C.sizeof(ax.GateRec), C.sizeof(ax.GateState)) == (24, 32, 8)
    assert [n for n, _ in ax.GateParams._fields_] == ["open_db", "close_db", "floor_db", "attack_ms", "hold_ms", "release_ms"]
    assert [(n, getattr(ax.GateRec, n).offset) for n, _ in ax.GateRec._fields_] == [
        ("t_open", 0), ("t_close", 4), ("floor", 8), ("span", 12), ("hold", 16), ("up", 20), ("down", 24), ("on", 28)]
    assert [(n, getattr(ax.GateState, n).offset) for n, _ in ax.GateState._fields_] == [("hold_left", 0), ("atten", 4)]
    assert ax.GATE_STATE_DTYPE.itemsize == 8 and ax.GATE_STATE_DTYPE.names == ("hold_left", "atten")
    assert [ax.GATE_STATE_DTYPE.fields[n][1] for n in ax.GATE_STATE_DTYPE.names] == [0, 4]


def test_the_calls_are_declared_and_exported():
    for name in ("aidax_gate_design", "aidax_pool_set_gate", "aidax_pool_stream_gate", "aidax_pool_read_gate"):
        assert name in ax.declared_symbols() and hasattr(ax.lib(), name)


def test_the_integers_are_exact():
    r = ax.gate_design(_params(attack_ms=1.0, hold_ms=10.0, release_ms=50.0), 48000.0)
    assert (r.hold, r.up, r.down, r.on) == (480, -(-P // 48), -(-P // 2400), 1)
    r = ax.gate_design(_params(attack_ms=1.0, hold_ms=10.0, release_ms=50.0), 44100.0)
    assert (r.hold, r.up, r.down) == (441, -(-P // 44), -(-P // 2205))
    # a time of 0 is one frame (up = P: the gate opens within the frame), the longest time at the highest rate is capped at 2^24 frames
    r = ax.gate_design(_params(attack_ms=0.0, hold_ms=0.0, release_ms=0.0), 48000.0)
    assert (r.hold, r.up, r.down) == (1, P, P)
    r = ax.gate_design(_params(attack_ms=10000.0, hold_ms=10000.0, release_ms=10000.0), 4.0e6)
    assert (r.hold, r.up, r.down) == (P, 1, 1)
    r = ax.gate_design(_params(attack_ms=10000.0, hold_ms=10000.0, release_ms=10000.0), 48000.0)
    assert (r.hold, r.up, r.down) == (480000, -(-P // 480000), -(-P // 480000))


@pytest.mark.parametrize("rate", (8000.0, 44100.0, 48000.0, 96000.0, 192000.0))
def test_a_ramp_ends_within_its_frames_and_not_a_frame_sooner(rate):
    """step = ceil(P / frames): the smallest integer step that ends the ramp within its frames (step x frames >= P > (step - 1) x frames).
    Up to 4096 frames the ramp then takes exactly its frames, P > step x (frames - 1): step < P / frames + 1 gives step x (frames - 1) <
    P + frames - 1 - P / frames, which is <= P when frames x (frames - 1) <= P = 2^24. A longer ramp may end early: no integer step of
    2^-24 per frame lies between P / frames and P / (frames - 1) there."""
    rs = np.random.RandomState(int(rate))
    for ms in [0.0, 0.01, 0.02, 1.0, 3.3, 10.0, 9999.0, 10000.0] + list(rs.uniform(0.0, 10000.0, 40)):
        ms = float(np.float32(ms))
        r = ax.gate_design(_params(attack_ms=ms, release_ms=ms, hold_ms=ms), rate)
        frames = min(P, max(1, int(math.floor(ms * rate / 1000.0 + 0.5))))
        assert r.hold == frames, (ms, rate)
        for step in (r.up, r.down):
            assert step * frames >= P > (step - 1) * frames, (ms, rate, step, frames)
            if frames * (frames - 1) <= P:
                assert P > step * (frames - 1), (ms, rate, step, frames)


def test_the_levels():
    for db in (0.0, -0.5, -6.0, -20.0, -30.0, -59.9, -90.0, -119.0, -120.0):
        r = ax.gate_design(_params(open_db=db, close_db=db, floor_db=max(db, -119.5)), 48000.0)
        want = np.float32(10.0 ** (float(np.float32(db)) / 20.0))
        for got in (r.t_open, r.t_close):
            assert abs(np.float32(got) - want) <= np.spacing(want), db
        assert r.t_close <= r.t_open
    r = ax.gate_design(_params(floor_db=-120.0), 48000.0)
    assert (r.floor, r.span) == (0.0, 1.0)
    r = ax.gate_design(_params(floor_db=-300.0), 48000.0)
    assert (r.floor, r.span) == (0.0, 1.0)
    r = ax.gate_design(_params(floor_db=0.0), 48000.0)
    assert (r.floor, r.span) == (1.0, 0.0)
    r = ax.gate_design(_params(floor_db=-40.0), 48000.0)
    assert abs(np.float32(r.floor) - np.float32(0.01)) <= np.spacing(np.float32(0.01))
    assert np.float32(r.span) == np.float32(1.0 - float(np.float32(r.floor)))
    r = ax.gate_design(_params(open_db=-10.0, close_db=-40.0), 48000.0)
    assert r.t_close < r.t_open


REFUSED = [
    (dict(open_db=float("nan")), 48000.0, "finite"),
    (dict(close_db=float("inf")), 48000.0, "finite"),
    (dict(floor_db=float("-inf")), 48000.0, "finite"),
    (dict(attack_ms=float("nan")), 48000.0, "finite"),
    (dict(hold_ms=float("inf")), 48000.0, "finite"),
    (dict(release_ms=float("nan")), 48000.0, "finite"),
    (dict(open_db=0.5), 48000.0, "open_db"),
    (dict(open_db=-121.0, close_db=-121.0), 48000.0, "open_db"),
    (dict(close_db=-120.5), 48000.0, "close_db"),
    (dict(open_db=-30.0, close_db=-20.0), 48000.0, "close_db must not exceed open_db"),
    (dict(floor_db=0.25), 48000.0, "floor_db"),
    (dict(attack_ms=-0.001), 48000.0, "attack_ms"),
    (dict(hold_ms=10000.5), 48000.0, "hold_ms"),
    (dict(release_ms=-1.0), 48000.0, "release_ms"),
    ({}, 0.0, "samplerate"),
    ({}, -48000.0, "samplerate"),
    ({}, float("nan"), "samplerate"),
]


@pytest.mark.parametrize("change,rate,word", REFUSED)
def test_refusals(change, rate, word):
    out = ax.GateRec(1.0, 2.0, 3.0, 4.0, 5, 6, 7, 8)
    before = bytes(out)
    p = _params(**change)
    assert ax.lib().aidax_gate_design(C.byref(p), rate, C.byref(out)) == ERR_ARG
    assert word in ax.last_error(), ax.last_error()
    assert bytes(out) == before                                  # a refused call changes nothing


def test_null_pointers():
    L = ax.lib()
    out, p = ax.GateRec(), _params()
    assert L.aidax_gate_design(None, 48000.0, C.byref(out)) == ERR_ARG and b"null" in L.aidax_last_error()
    assert L.aidax_gate_design(C.byref(p), 48000.0, None) == ERR_ARG and b"null" in L.aidax_last_error()


def test_a_null_pool_is_an_argument_error_without_a_device():
    L = ax.lib()
    p, on = _params(), C.c_int(7)
    assert L.aidax_pool_set_gate(None, ax.ALL_STREAMS, C.byref(p)) == ERR_ARG and b"null" in L.aidax_last_error()
    assert L.aidax_pool_set_gate(None, 0, None) == ERR_ARG
    assert L.aidax_pool_stream_gate(None, 0, C.byref(p), C.byref(on)) == ERR_ARG and b"null" in L.aidax_last_error()
    assert on.value == 7
    st = np.full(1, 9, ax.GATE_STATE_DTYPE)
    assert L.aidax_pool_read_gate(None, 0, 1, st.ctypes.data_as(C.POINTER(ax.GateState))) == ERR_ARG and b"null" in L.aidax_last_error()
    assert st["hold_left"][0] == 9 and st["atten"][0] == 9
