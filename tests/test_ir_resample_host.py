"""aidax_ir_resample and the pool's IR capacity, the parts that need no device: the exports from both builds of the library, the argument
checks with their aidax_last_error texts, the length formula, the exact cases (equal rates, ratios 2 and 4, the lead), and the values
against tests/irresample.py, an independent numpy fp64 statement of the formula in include/aidax.h that never calls the library.

Bounds. Per tap, against the helper: 2^-23 |v| + 1e-12 sum|in| -- both sides round an fp64 value once to fp32 (half an ulp each, so one
ulp = 2^-23 |v| apart at most when the fp64 values straddle a rounding boundary), and the fp64 values differ by the noise of two libms
and two orders of addition, some 1e-16 of the sum of the absolute terms, which sum|in| bounds with four decades to spare.
Spectrum: the helper's own output on the test IR (8192 taps of rng(3) noise under exp(-k / 600), h[0] = 1), full lead, 200 frequencies
from 20 Hz to 0.8 of the lower Nyquist, is within 4.7e-7 .. 9.75e-7 of max|H| of the input's DTFT over the six rate pairs below (a
prototype of the same formula gave 5.3e-7 .. 9.6e-7 over five of them). The bound is five times the helper's worst, 4.875e-6 (to
cover fp32 rounding on other seeds); it was never derived from the library's output."""
import ctypes as C
import importlib

import numpy as np
import pytest

from tests import conftest, irresample as rs

ax = importlib.import_module("aidadsp-lv2_amd")
ERR_ARG = -1
NEW = ("aidax_ir_resample", "aidax_pool_set_ir_capacity", "aidax_pool_ir_capacity")
PAIRS = ((48000, 44100), (48000, 88200), (48000, 96000), (48000, 192000), (48000, 32000), (44100, 48000))
SPECTRUM_BOUND = 5 * 9.75e-7
_fp = C.POINTER(C.c_float)


def _raw(taps, n_in, rate_in, rate_out, lead, out, cap, with_n=True):
    """the C call as it is: (return code, n_full, aidax_last_error)"""
    L = ax.lib()
    n = C.c_uint32(12345)
    rc = L.aidax_ir_resample(None if taps is None else taps.ctypes.data_as(_fp), n_in, rate_in, rate_out, lead,
                             None if out is None else out.ctypes.data_as(_fp), cap, C.byref(n) if with_n else None)
    return rc, n.value, L.aidax_last_error().decode()


def test_both_libraries_export_the_entry_points():
    names = ax.declared_symbols()
    for path in (conftest.SHIP_LIB, conftest.HOOKS_LIB):
        L = C.CDLL(path)
        for n in NEW:
            assert n in names, n
            assert hasattr(L, n), (path, n)
    with open(f"{conftest.ROOT}/include/aidax.h") as f:
        text = f.read()
    threads = text.split("/* Threads.")[1].split("*/")[0]
    assert "set_ir_capacity is a set-up side call" in threads and "aidax_ir_resample" in threads and "host only" in threads
    assert "#define AIDAX_IR_MAX_CAPACITY 65536" in text
    assert hasattr(ax, "resample_ir") and hasattr(ax, "load_ir_wav_for")
    assert hasattr(ax.Pool, "set_ir_capacity") and hasattr(ax.Pool, "ir_capacity")


def test_capacity_argument_checks_without_a_pool():
    L = ax.lib()
    assert L.aidax_pool_ir_capacity(None) == 0
    assert L.aidax_pool_set_ir_capacity(None, 16384) == ERR_ARG
    assert "null pool" in L.aidax_last_error().decode()
    for bad in (0, 8191, 65537, 0xffffffff):
        assert L.aidax_pool_set_ir_capacity(None, bad) == ERR_ARG
        assert "IR capacity must be 8192 .. 65536" in L.aidax_last_error().decode()


def test_resample_argument_checks():
    h = np.ones(4, np.float32)
    out = np.zeros(64, np.float32)
    rc, n, msg = _raw(None, 4, 48000.0, 44100.0, 0, out, 64)
    assert rc == ERR_ARG and "null argument" in msg
    rc, n, msg = _raw(h, 4, 48000.0, 44100.0, 0, None, 64)                  # cap > 0 wants a buffer
    assert rc == ERR_ARG and "null argument" in msg
    rc, n, msg = _raw(h, 4, 48000.0, 44100.0, 0, out, 64, with_n=False)
    assert rc == ERR_ARG and "null argument" in msg
    rc, n, msg = _raw(h, 0, 48000.0, 44100.0, 0, out, 64)
    assert rc == ERR_ARG and "no input taps" in msg and n == 0
    for ri, ro in ((48000.5, 44100.0), (48000.0, 0.0), (-48000.0, 44100.0), (48000.0, float("nan")), (float("inf"), 44100.0),
                   (48000.0, 2.0 ** 24 + 2)):
        rc, n, msg = _raw(h, 4, ri, ro, 0, out, 64)
        assert rc == ERR_ARG and "sample rates must be positive integers" in msg, (ri, ro, msg)
    rc, n, msg = _raw(h, 4, 48000.0, 44100.0, 1025, out, 64)
    assert rc == ERR_ARG and "lead must be 0 .. 1024" in msg
    assert _raw(h, 4, 48000.0, 44100.0, 1024, out, 64)[0] == 0
    for v in (np.nan, np.inf, -np.inf):
        bad = h.copy()
        bad[2] = v
        rc, n, msg = _raw(bad, 4, 48000.0, 44100.0, 0, out, 64)
        assert rc == ERR_ARG and "tap 2 is not finite" in msg
    # 2^31 frames or more: 2^20 taps up by 2^24 / 1 -- refused before anything is written (a length query: nothing could be)
    big = np.zeros(1 << 20, np.float32)
    rc, n, msg = _raw(big, big.size, 1.0, 2.0 ** 24, 0, None, 0)
    assert rc == ERR_ARG and "2^31 frames" in msg and n == 0
    assert np.array_equal(out, np.zeros(64, np.float32))                    # no failed call wrote a tap


@pytest.mark.parametrize("pair", PAIRS + ((48000, 48000), (1, 7), (7, 1), (44100, 192000), (96000, 44100)))
def test_the_length_formula_and_the_length_query(pair):
    ri, ro = pair
    for n_in in (1, 2, 100, 8192):
        for lead in (0, 1, 37, 1024):
            want = rs.n_full(n_in, ri, ro, lead)
            h = np.ones(n_in, np.float32)
            rc, n, _ = _raw(h, n_in, float(ri), float(ro), lead, None, 0)   # cap == 0, out == NULL: the length alone
            assert rc == 0 and n == want, (n_in, lead, n, want)
    # min(cap, n_full) taps are written and no more; n_full is reported whatever the cap
    h = rs.noise_ir(300)
    full, n = ax.resample_ir(h, ri, ro, 5)
    assert n == full.size == rs.n_full(300, ri, ro, 5)
    buf = np.full(n + 8, 7.0, np.float32)
    rc, n2, _ = _raw(h, 300, float(ri), float(ro), 5, buf, n + 8)
    assert rc == 0 and n2 == n and np.array_equal(buf[:n], full) and np.all(buf[n:] == 7.0)
    cap = n // 2
    buf = np.full(cap + 8, 7.0, np.float32)
    rc, n2, _ = _raw(h, 300, float(ri), float(ro), 5, buf, cap)
    assert rc == 0 and n2 == n and np.array_equal(buf[:cap], full[:cap]) and np.all(buf[cap:] == 7.0)   # cut, not faded
    cut, n3 = ax.resample_ir(h, ri, ro, 5, cap=cap)
    assert n3 == n and np.array_equal(cut, full[:cap])


def test_the_whole_pre_ringing():
    assert rs.full_lead(48000, 44100) == 32 and rs.full_lead(48000, 96000) == 64 and rs.full_lead(48000, 192000) == 128
    assert rs.full_lead(44100, 48000) == 35 and rs.full_lead(48000, 32000) == 32
    # frames before the kernel's support are zeros: with a lead longer than the pre-ringing, the first lead - full are 0 and the next is not
    for ri, ro in PAIRS:
        full = rs.full_lead(ri, ro)
        got, _ = ax.resample_ir(np.array([1.0, 0.5, 0.25], np.float32), ri, ro, full + 10)
        assert np.all(got[:10] == 0.0) and np.count_nonzero(got[10:20]) >= 4, (ri, ro, got[:20])   # (zero crossings fall on frames too)


def test_equal_rates_are_a_bit_copy_behind_the_lead():
    h = rs.noise_ir(1000)
    h[5] = -0.0
    h[6] = np.float32(1e-42)                                                # a denormal stays one
    for rate in (48000, 44100, 1):
        for lead in (0, 3, 1024):
            got, n = ax.resample_ir(h, rate, rate, lead)
            assert n == lead + 1000 + 32
            want = np.concatenate([np.zeros(lead, np.float32), h, np.zeros(32, np.float32)])
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


@pytest.mark.parametrize("r", [2, 4])
def test_integer_ratios_keep_the_input_taps_on_the_even_phases(r):
    """c = 1: an integer u weighs exactly 0 and u = 0 exactly 1, so out[lead + r k] = in[k] / r (M / L = 1 / r, a power of two)"""
    h = rs.noise_ir(2000)
    for lead in (0, 7, r * 32):
        got, _ = ax.resample_ir(h, 48000, 48000 * r, lead)
        assert np.array_equal(got[lead:lead + r * 2000:r], h / np.float32(r))
        if lead:
            assert np.all(got[lead % r:lead:r] == 0.0)                      # the same phase before t = 0: whole periods of the sinc
        assert np.count_nonzero(got[lead + 1:lead + r * 2000:r]) > 1900     # the phases in between are interpolated


@pytest.mark.parametrize("pair", PAIRS)
def test_the_lead_shifts_the_result_and_changes_no_value(pair):
    ri, ro = pair
    h = rs.noise_ir(700)
    full = rs.full_lead(ri, ro)
    base, n = ax.resample_ir(h, ri, ro, full)
    for lead in (0, 1, full // 2, full + 9, 1024):
        got, m = ax.resample_ir(h, ri, ro, lead)
        assert m == n - full + lead
        if lead <= full:
            assert np.array_equal(got, base[full - lead:])                  # the earlier pre-ringing is dropped, nothing else moves
        else:
            assert np.all(got[:lead - full] == 0.0) and np.array_equal(got[lead - full:], base)


def test_a_fixed_input_gives_the_same_bits_every_time():
    h = rs.noise_ir(3000)
    for ri, ro in PAIRS + ((44100, 192000),):                               # (the last pair: D = 640)
        a, _ = ax.resample_ir(h, ri, ro, 16)
        for _ in range(3):
            b, _ = ax.resample_ir(h.copy(), ri, ro, 16)
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    # ... and a cut result is the head of the whole one, whichever way the weights were computed (table or direct: the table serves
    # results longer than max(L, M) frames)
    a, _ = ax.resample_ir(h, 48000, 44100, 16)
    b, _ = ax.resample_ir(h, 48000, 44100, 16, cap=100)
    assert np.array_equal(a[:100].view(np.uint32), b.view(np.uint32))
    # ratios too large for a table of weights (max(L, M) > 4096) go the direct way
    a, _ = ax.resample_ir(h[:200], 48000, 44101, 8)
    w = rs.resample64(h[:200], 48000, 44101, 8)
    assert np.all(np.abs(a.astype(np.float64) - w.astype(np.float32)) <= 2.0 ** -23 * np.abs(w) + 1e-12 * np.abs(h[:200]).sum())


@pytest.mark.parametrize("pair", PAIRS)
def test_every_tap_against_the_fp64_helper(pair):
    ri, ro = pair
    h = rs.noise_ir()
    for lead in (0, rs.full_lead(ri, ro)):
        got, n = ax.resample_ir(h, ri, ro, lead)
        w64 = rs.resample64(h, ri, ro, lead)
        assert n == w64.size == got.size
        err = np.abs(got.astype(np.float64) - w64.astype(np.float32).astype(np.float64))
        bound = 2.0 ** -23 * np.abs(w64) + 1e-12 * np.abs(h.astype(np.float64)).sum()
        print(f"{ri} -> {ro} lead {lead}: worst error / bound {np.max(err / bound):.3g}, taps that differ {np.count_nonzero(err)}")
        assert np.all(err <= bound), (int(np.argmax(err / bound)), float(np.max(err / bound)))
    # the discrete convolution's gain is kept: the DC gains agree to the filter's stopband leakage
    assert abs(float(got.astype(np.float64).sum()) - float(h.astype(np.float64).sum())) < 1e-4 * np.abs(h).sum()


@pytest.mark.parametrize("pair", PAIRS)
def test_the_spectrum_is_kept_up_to_the_lower_nyquist(pair):
    ri, ro = pair
    h = rs.noise_ir()
    lead = rs.full_lead(ri, ro)
    f = np.geomspace(20.0, 0.8 * min(ri, ro) / 2, 200)
    H = rs.dtft(h, ri, f)
    scale = np.abs(H).max()
    helper = np.abs(rs.dtft(rs.resample(h, ri, ro, lead), ro, f, lead) - H).max() / scale
    got, _ = ax.resample_ir(h, ri, ro, lead)
    err = np.abs(rs.dtft(got, ro, f, lead) - H).max() / scale
    print(f"{ri} -> {ro}: library {err:.3g}, helper {helper:.3g} of max|H|")
    assert helper <= 1e-6                                                   # what the bound was derived from still holds
    assert err <= SPECTRUM_BOUND
    # lead = 0 costs what the header says: about 0.1 % down to 44.1 kHz, about 2 % going up
    cut, _ = ax.resample_ir(h, ri, ro, 0)
    e0 = np.abs(rs.dtft(cut, ro, f, 0) - H).max() / scale
    print(f"{ri} -> {ro}: lead 0 costs {e0:.3g}")
    assert 1e-4 < e0 < 3e-2
