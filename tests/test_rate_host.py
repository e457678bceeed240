"""The rate adapter's parts that need no device: the exports from both builds of the library, aidax_resampler_row against
tests/rateref.py (an independent numpy fp64 statement of the formulas in include/aidax.h that never calls the library), the latencies,
and the argument checks with their aidax_last_error texts.

Bound on a weight, against the helper: 2^-23 |v| + 1e-12 -- both sides round an fp64 value once to fp32 (half an ulp each, so one ulp
= 2^-23 |v| apart at most when the fp64 values straddle a rounding boundary), and the fp64 values differ by the noise of two libms,
some 1e-16 for weights of at most 1: the argument of tests/test_ir_resample_host.py for one term."""
import ctypes as C
import importlib

import numpy as np
import pytest

from tests import conftest, rateref as rr

ax = importlib.import_module("aidadsp-lv2_amd")
ERR_ARG = -1
NEW = ("aidax_resampler_create", "aidax_resampler_destroy", "aidax_resampler_row", "aidax_resampler_process_device", "aidax_resampler_process",
       "aidax_resampler_ready", "aidax_resampler_reset_stream", "aidax_pool_samplerate", "aidax_rate_create", "aidax_rate_destroy",
       "aidax_rate_latency_frames", "aidax_rate_latency", "aidax_rate_process", "aidax_rate_process_device", "aidax_rate_reset_stream")
# (rate_in, rate_out): L / M = 160 / 147, 147 / 160, 1 / 2, 2 / 1, 147 / 640, with the row length T = 2 ceil(32 max(L, M) / L) + 1;
# then the pairs of tests/test_gpu_rate_wide.py around the staged form's limit (77 -> 6 fills the LDS window, 90 -> 7 is the first in
# place), the longest row the API admits (640 -> 1) and the most phases at the largest term (640 -> 639: all 639 run once)
ROW_PAIRS = (((44100, 48000), 160, 65), ((48000, 44100), 147, 71), ((96000, 48000), 1, 129), ((48000, 96000), 2, 65), ((192000, 44100), 147, 281),
             ((13, 1), 1, 833), ((77, 6), 6, 823), ((90, 7), 7, 825), ((96000, 7000), 7, 879), ((192000, 8000), 1, 1537), ((640, 1), 1, 40961),
             ((640, 639), 639, 67))
_fp = C.POINTER(C.c_float)


def test_both_libraries_export_the_entry_points():
    names = ax.declared_symbols()
    for path in (conftest.SHIP_LIB, conftest.HOOKS_LIB):
        L = C.CDLL(path)
        for n in NEW:
            assert n in names, n
            assert hasattr(L, n), (path, n)
    with open(f"{conftest.ROOT}/include/aidax.h") as f:
        threads = f.read().split("/* Threads.")[1].split("*/")[0]
    audio = threads.split("plus, concurrently")[0]
    for n in ("aidax_rate_process", "aidax_rate_process_device", "aidax_rate_reset_stream"):
        assert n in audio, n
    assert "aidax_rate_create and aidax_rate_destroy are set-up side calls" in threads
    for n in ("Resampler", "RateAdapter", "resampler_row", "rate_latency"):
        assert hasattr(ax, n), n
    for cls in (ax.Resampler, ax.RateAdapter):
        for n in ("process", "process_device", "latency_frames", "reset_stream", "close"):
            assert hasattr(cls, n), (cls, n)


@pytest.mark.parametrize("pair,L,T", ROW_PAIRS)
def test_every_row_against_the_fp64_statement(pair, L, T):
    ri, ro = pair
    assert rr.params(ri, ro)[0] == L and rr.params(ri, ro)[5] == T
    want = rr.rows64(ri, ro)
    assert want.shape == (L, T)
    for phase in range(L):
        w = ax.resampler_row(float(ri), float(ro), phase)
        assert w.dtype == np.float32 and w.size == T, (phase, w.size)
        assert np.all(np.abs(w.astype(np.float64) - want[phase]) <= 2.0 ** -23 * np.abs(want[phase]) + 1e-12), phase
    # a cap below T cuts the row and still reports T; nothing is written past the cap
    buf = np.full(T + 4, 7.0, np.float32)
    n = C.c_uint32(0)
    assert ax.lib().aidax_resampler_row(float(ri), float(ro), L - 1, buf.ctypes.data_as(_fp), 5, C.byref(n)) == 0
    assert n.value == T and np.array_equal(buf[:5], ax.resampler_row(float(ri), float(ro), L - 1)[:5]) and np.all(buf[5:] == 7.0)


def test_the_exact_rows():
    for rate in (48000, 44100, 1):
        w = ax.resampler_row(float(rate), float(rate), 0)                   # equal rates: L = M = 1, H = 32, a delta
        delta = np.zeros(65, np.float32)
        delta[32] = 1.0
        assert np.array_equal(w, delta), rate
    w = ax.resampler_row(48000.0, 96000.0, 0)                               # 2 / 1: phase 0 sits on the input frames
    assert np.array_equal(w, delta)
    assert np.count_nonzero(ax.resampler_row(48000.0, 96000.0, 1)) == 64    # ... and phase 1 between them: 32 a side


def test_latency():
    for host, pool, want in ((44100, 48000, 66), (96000, 48000, 130), (192000, 48000, 260), (48000, 44100, 71), (48000, 48000, 0)):
        assert ax.rate_latency(float(host), float(pool)) == want == rr.latency(host, pool), (host, pool)
    for host, pool in ((88200, 48000), (44100, 192000), (192000, 44100)):
        assert ax.rate_latency(float(host), float(pool)) == rr.latency(host, pool), (host, pool)


def test_argument_checks():
    L = ax.lib()
    n = C.c_uint32(12345)
    buf = np.full(300, 7.0, np.float32)

    def row(ri, ro, phase=0, w=buf, cap=300, with_n=True):
        rc = L.aidax_resampler_row(ri, ro, phase, None if w is None else w.ctypes.data_as(_fp), cap, C.byref(n) if with_n else None)
        return rc, L.aidax_last_error().decode()

    def lat(host, pool, with_n=True):
        rc = L.aidax_rate_latency(host, pool, C.byref(n) if with_n else None)
        return rc, L.aidax_last_error().decode()

    for call in (row, lat):
        for ri, ro in ((48000.5, 44100.0), (48000.0, 0.0), (-48000.0, 44100.0), (48000.0, float("nan")), (float("inf"), 44100.0), (48000.0, 2.0 ** 24 + 2)):
            rc, msg = call(ri, ro)
            assert rc == ERR_ARG and "sample rates must be positive integers" in msg and n.value == 0, (ri, ro, msg)
        for ri, ro in ((48000.0, 44101.0), (641.0, 1.0), (1.0, 641.0), (44100.0, 32000.0)):          # 441 / 320 is in range, 320 / 441 too
            rc, msg = call(ri, ro)
            if max(rr.params(ri, ro)[:2]) > 640:
                assert rc == ERR_ARG and "must not exceed 640" in msg, (ri, ro, msg)
            else:
                assert rc == 0, (ri, ro, msg)
        rc, msg = call(48000.0, 44100.0, with_n=False)
        assert rc == ERR_ARG and "null argument" in msg
    assert row(1.0, 640.0, cap=0, w=None)[0] == 0 and n.value == 65
    assert row(640.0, 1.0, cap=0, w=None)[0] == 0 and n.value == 2 * 32 * 640 + 1
    rc, msg = row(48000.0, 44100.0, w=None)                                  # cap > 0 wants a buffer
    assert rc == ERR_ARG and "null argument" in msg
    rc, msg = row(48000.0, 44100.0, phase=147)
    assert rc == ERR_ARG and "phase must be below L = 147" in msg
    assert np.all(buf[281:] == 7.0)                                          # no call wrote past a row
    out = C.c_void_p(1)
    assert L.aidax_rate_create(None, 44100.0, 256, C.byref(out)) == ERR_ARG and out.value is None
    assert "null argument" in L.aidax_last_error().decode()
    assert L.aidax_resampler_create(1, 44100.0, 48000.0, 0, 0, 256, 0, None) == ERR_ARG
    assert L.aidax_resampler_create(0, 44100.0, 48000.0, 0, 0, 256, 0, C.byref(out)) == ERR_ARG
    assert "n_streams" in L.aidax_last_error().decode()
    assert L.aidax_resampler_create(1, 44100.0, 48001.0, 0, 0, 256, 0, C.byref(out)) == ERR_ARG
    assert "must not exceed 640" in L.aidax_last_error().decode()
    for fn in (L.aidax_rate_process, L.aidax_rate_process_device):
        assert fn(None, None, None, 0, *([None] if fn is L.aidax_rate_process_device else [])) == ERR_ARG
    assert L.aidax_resampler_process_device(None, None, 0, None, 0, None) == ERR_ARG and L.aidax_resampler_ready(None) == 0
    assert L.aidax_rate_latency_frames(None) == 0 and L.aidax_pool_samplerate(None) == 0.0
    L.aidax_rate_destroy(None)
    L.aidax_resampler_destroy(None)
