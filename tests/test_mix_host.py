"""The mix buses, host side (no device): aidax_mix_gain, the pure function behind a send's ramp frame, against the formula of
include/aidax.h in Python floats (IEEE doubles: every operation rounded on its own, then one rounding to float32) and against the numpy
restatement the GPU tests use (tests/mixhelp.py); the arguments it refuses; the names the header declares."""
import ctypes as C
import importlib
import struct

import numpy as np
import pytest

from tests import mixhelp as mh

ax = importlib.import_module("aidadsp-lv2_amd")
ERR_ARG = -1


def f32(v):
    return struct.unpack("f", struct.pack("f", v))[0]


def want(g0, g1, R, k):
    g0, g1 = f32(g0), f32(g1)
    if k + 1 >= R:
        return g1
    return f32(g0 + (g1 - g0) * float(k + 1) / float(R))


def bits(v):
    return struct.pack("f", v)


RAMPS = (0, 1, 2, 3, 48000, 1 << 24)
PAIRS = ((0.0, 1.0), (1.0, 0.0), (0.25, -0.75), (-2.0, 2.0), (0.7, 0.7), (1e-30, 3e-30), (0.0, 2.0 ** -10), (-16.0, 16.0), (0.1, 0.30000001),
         (1.0, 0.99999994))


def test_the_header_declares_the_calls_and_the_library_exports_them():
    names = ("aidax_pool_set_buses", "aidax_pool_buses", "aidax_pool_set_send", "aidax_pool_stream_send", "aidax_mix_gain", "aidax_pool_read_buses",
             "aidax_pool_buses_device", "aidax_pool_process_buses")
    declared = ax.declared_symbols()
    for name in names:
        assert name in declared and hasattr(ax.lib(), name), name
    assert (ax.SENDS, ax.BUS_NONE, ax.MAX_BUSES) == (4, -1, 4096) == (mh.SENDS, mh.BUS_NONE, 4096)


@pytest.mark.parametrize("R", RAMPS)
def test_mix_gain_is_the_formula(R):
    ks = sorted({k for k in (0, 1, 2, 3, R // 3, R // 2, R - 3, R - 2, R - 1, R, R + 1, R + 1000, 1 << 25, 0xFFFFFFFF) if k >= 0})
    for g0, g1 in PAIRS:
        for k in ks:
            got = ax.mix_gain(g0, g1, R, k)
            assert bits(got) == bits(want(g0, g1, R, k)), (g0, g1, R, k, got)
            if k < 1 << 30:
                assert bits(got) == mh.gain(g0, g1, R, k).tobytes(), (g0, g1, R, k)
        if R:
            assert bits(ax.mix_gain(g0, g1, R, R - 1)) == bits(f32(g1))          # the last ramp frame is the target itself


def test_a_ramp_moves_and_ends():
    # between equal gains every frame is that gain; a long ramp's first frame has left g0, its last but one has not reached g1
    assert all(ax.mix_gain(0.7, 0.7, 1000, k) == f32(0.7) for k in (0, 1, 500, 998, 999))
    assert 0.0 < ax.mix_gain(0.0, 1.0, 1 << 24, 0) == 2.0 ** -24 and ax.mix_gain(0.0, 1.0, 1 << 24, (1 << 24) - 2) == f32(1.0 - 2.0 ** -24)
    assert ax.mix_gain(1.0, -1.0, 2, 0) == 0.0 and ax.mix_gain(1.0, -1.0, 2, 1) == -1.0
    # tiny gains: the difference is formed in fp64, not lost in fp32
    assert ax.mix_gain(1e-30, 3e-30, 2, 0) == f32(f32(1e-30) + (f32(3e-30) - f32(1e-30)) * 1.0 / 2.0) != f32(1e-30)
    # a whole ramp, frame by frame, against the numpy restatement
    got = np.array([ax.mix_gain(0.25, -0.75, 97, k) for k in range(120)], np.float32)
    assert got.tobytes() == mh.gain(0.25, -0.75, 97, np.arange(120)).tobytes()
    assert np.all(np.diff(got[:97]) < 0) and np.all(got[96:] == np.float32(-0.75))


def test_refused_arguments():
    L = ax.lib()
    out = C.c_float(7.0)
    for g0, g1, R in ((float("nan"), 1.0, 8), (0.0, float("inf"), 8), (0.0, -float("inf"), 8), (16.5, 0.0, 8), (0.0, -16.000002, 8), (0.0, 1.0, (1 << 24) + 1),
                      (0.0, 1.0, 0xFFFFFFFF)):
        assert L.aidax_mix_gain(g0, g1, R, 0, C.byref(out)) == ERR_ARG, (g0, g1, R)
        assert out.value == 7.0 and L.aidax_last_error()
        with pytest.raises(ax.AidaxError) as e:
            ax.mix_gain(g0, g1, R, 0)
        assert e.value.code == ERR_ARG
    assert L.aidax_mix_gain(0.0, 1.0, 8, 0, None) == ERR_ARG and b"null" in L.aidax_last_error()
    assert ax.mix_gain(-16.0, 16.0, 1 << 24, 0) == f32(-16.0 + 32.0 / (1 << 24))      # the bounds themselves are fine
