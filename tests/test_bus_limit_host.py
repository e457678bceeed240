"""The bus limiters, host side (no device): aidax_bus_limit_design against the formula of include/aidax.h in Python floats and what it
refuses; the names the header declares; the three properties of the rule (the ceiling holds without a clamp, block cuts do not show,
a bus under its ceiling keeps its bits) on the numpy restatement the GPU tests compare the kernel with (tests/limithelp.py); and the
condition on the GPU tests' inputs: by the restatement alone every limited bus there is limited somewhere, not everywhere, and reaches its
ceiling, so a limiter that never acts cannot pass them."""
import ctypes as C
import importlib
import struct

import numpy as np
import pytest

from tests import limithelp as lh

ax = importlib.import_module("aidadsp-lv2_amd")
ERR_ARG = -1
f32 = np.float32


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def _params(ceiling_db=-1.0, lookahead_ms=1.0, hold_ms=0.0):
    return ax.BusLimitParams(ceiling_db, lookahead_ms, hold_ms)


def test_the_header_declares_the_calls_and_the_library_exports_them():
    names = ("aidax_bus_limit_design", "aidax_pool_set_bus_limiting", "aidax_pool_bus_limiting", "aidax_pool_set_bus_limiter", "aidax_pool_bus_limiter",
             "aidax_pool_read_bus_meters")
    declared = ax.declared_symbols()
    for name in names:
        assert name in declared and hasattr(ax.lib(), name), name
    assert (ax.ALL_BUSES, ax.BUS_LOOKAHEAD_MAX, ax.BUS_HOLD_MAX) == (-1, 512, 4096) == (lh.ALL_BUSES, lh.LOOKAHEAD_MAX, lh.HOLD_MAX)
    assert C.sizeof(ax.BusLimitRec) == 16 and C.sizeof(ax.BusMeter) == 48 == ax.BUS_METER_DTYPE.itemsize and C.sizeof(ax.BusLimitParams) == 12
    assert ax.BUS_METER_DTYPE == lh.METER_DTYPE
    for m in ("set_bus_limiting", "bus_limiting", "set_bus_limiter", "bus_limiter", "read_bus_meters"):
        assert hasattr(ax.Pool, m), m
    with open(ax.binding._HEADER) as f:
        text = f.read()
    for word in ("#define AIDAX_ALL_BUSES (-1)", "#define AIDAX_BUS_LOOKAHEAD_MAX 512", "#define AIDAX_BUS_HOLD_MAX 4096", "NOT click-free"):
        assert word in text, word


@pytest.mark.parametrize("rate", (44100.0, 48000.0, 96000.0))
def test_design_is_the_formula(rate):
    for db in (-60.0, -20.0, -6.0, -3.0, -0.1, 0.0, 3.3, 12.0):
        for look_ms, hold_ms in ((0.02, 0.0), (1.0, 0.0), (1.33, 10.0), (5.0, 42.5), (lh.ms(512, rate), lh.ms(4096, rate)), (lh.ms(1, rate), lh.ms(1, rate))):
            r = ax.bus_limit_design(_params(db, look_ms, hold_ms), rate)
            Cw, L, H = lh.design(db, look_ms, hold_ms, rate)
            assert struct.pack("f", r.ceiling) == Cw.tobytes() and (r.lookahead, r.hold, r.on) == (L, H, 1), (db, look_ms, hold_ms)
            assert r.ceiling > 0 and 1 <= r.lookahead <= 512 and r.hold <= 4096
    r = ax.bus_limit_design(_params(0.0, lh.ms(64), lh.ms(100)), 48000.0)
    assert (r.ceiling, r.lookahead, r.hold) == (1.0, 64, 100)


def test_design_refuses():
    L = ax.lib()
    out = ax.BusLimitRec(7.0, 7, 7, 7)
    nan, inf = float("nan"), float("inf")
    bad = [(nan, 1.0, 0.0), (0.0, nan, 0.0), (0.0, 1.0, nan), (inf, 1.0, 0.0), (0.0, inf, 0.0), (0.0, 1.0, inf), (0.0, 1.0, -inf),
           (-60.1, 1.0, 0.0), (12.1, 1.0, 0.0),
           (0.0, 0.0, 0.0), (0.0, 0.01, 0.0), (0.0, -1.0, 0.0),              # a look-ahead below one frame (0.48 of one at 48 kHz)
           (0.0, lh.ms(513), 0.0), (0.0, 1e30, 0.0),                         # ... beyond 512 frames
           (0.0, 1.0, lh.ms(4097)), (0.0, 1.0, 1e30), (0.0, 1.0, -0.5)]      # a hold beyond 4096 frames, a negative one
    for db, look, hold in bad:
        p = _params(db, look, hold)
        assert L.aidax_bus_limit_design(C.byref(p), 48000.0, C.byref(out)) == ERR_ARG, (db, look, hold)
        assert (out.ceiling, out.lookahead, out.hold, out.on) == (7.0, 7, 7, 7) and L.aidax_last_error()
        with pytest.raises(ax.AidaxError) as e:
            ax.bus_limit_design(p, 48000.0)
        assert e.value.code == ERR_ARG
    p = _params()
    for rate in (0.0, -48000.0, nan, inf):
        assert L.aidax_bus_limit_design(C.byref(p), rate, C.byref(out)) == ERR_ARG, rate
    assert L.aidax_bus_limit_design(None, 48000.0, C.byref(out)) == ERR_ARG and b"null" in L.aidax_last_error()
    assert L.aidax_bus_limit_design(C.byref(p), 48000.0, None) == ERR_ARG
    # the bounds themselves are fine
    for db, look, hold in ((-60.0, lh.ms(1), 0.0), (12.0, lh.ms(512), lh.ms(4096))):
        ax.bus_limit_design(_params(db, look, hold), 48000.0)


def test_a_null_pool_is_an_argument_error_without_a_device():
    L = ax.lib()
    p = _params()
    m = ax.BusMeter()
    assert L.aidax_pool_set_bus_limiting(None, 1, 64, 0) == ERR_ARG and b"null" in L.aidax_last_error()
    assert L.aidax_pool_bus_limiting(None) == 0
    assert L.aidax_pool_set_bus_limiter(None, 0, C.byref(p)) == ERR_ARG
    assert L.aidax_pool_bus_limiter(None, 0, None, None, None) == ERR_ARG
    assert L.aidax_pool_read_bus_meters(None, 0, 1, C.byref(m), 0) == ERR_ARG


# ---- the restatement's properties ------------------------------------------------------------------------------------------------------
LS, HS = (1, 2, 63, 64, 65, 512), (0, 1, 100, 4096)
CUTS = [1, 3, 0, 63, 64, 65, 200, 4]


def _through(x, C_, L, H, cuts):
    ref = lh.Reference(1)
    ref.set(0, (C_, L, H))
    at, outs, i = 0, [], 0
    while at < len(x):
        n = min(cuts[i % len(cuts)], len(x) - at)
        i += 1
        outs.append(ref.process(x[None, at:at + n])[0])
        at += n
    return np.concatenate(outs), ref


@pytest.mark.parametrize("L", LS)
def test_the_ceiling_holds_and_cuts_do_not_show(L):
    for k, H in enumerate(HS):
        for db in (-60.0, -7.0, 12.0):
            C_ = f32(10.0 ** (db / 20.0))
            n = 700 + 2 * L + (H if H <= 100 else 300)
            x = lh.signal(C_, 1000 * L + k, n=n, kind="wild" if k % 2 else "peaks")
            rng = np.random.default_rng(L + k)
            x[rng.integers(0, n, 6)] = (C_ * f32(10.0) ** rng.uniform(0, 6, 6)).astype(f32)      # peaks of every size up to 1e6 C
            x[rng.integers(0, n, 2)] = np.nextafter(C_, f32(np.inf))
            out, g, s = lh.limit(x, C_, L, H)
            assert np.isfinite(out).all() and (np.abs(out) <= C_).all(), (L, H, db)
            assert 0 < (s < L * lh.U).sum() and (g <= 1).all() and (g >= 0).all()
            # the bound behind it: g[n] <= q[n - L] / U, exactly
            q = lh.gain_positions(lh.sanitise(x), C_)
            assert (s[L:] <= L * q[:-L]).all()
            cut, ref = _through(x, C_, L, H, CUTS)
            assert np.array_equal(bits(cut), bits(out)), (L, H, db)
            m = ref.read_meters()[0]
            assert m["frames"] == n and m["limited"] == (s < L * lh.U).sum() and m["min_gain"] == g.min() and m["out_peak"] == np.abs(out).max()
            assert m["in_nonfinite"] == (~np.isfinite(x)).sum() and m["in_peak"] == np.abs(lh.sanitise(x)).max()


@pytest.mark.parametrize("L", LS)
def test_transparency_is_exact(L):
    for H in HS:
        C_ = f32(0.7071068)
        x = lh.signal(C_, 7 * L + H, n=900, kind="quiet")
        x[17] = -C_                                              # at the ceiling is not beyond it
        x[40] = f32(1e-41)                                       # a denormal stays one
        out, g, s = lh.limit(x, C_, L, H)
        assert (g == 1).all() and (s == L * lh.U).all()
        assert np.array_equal(bits(out[L:]), bits(x[:-L])) and not out[:L].any()
        # one ulp more at one frame and the limiter acts, over 2 L + H + 1 frames
        x[450] = np.nextafter(C_, f32(np.inf))
        out, g, s = lh.limit(x, C_, L, H)
        acted = np.flatnonzero(s < L * lh.U)
        assert len(acted) and acted[0] == 450 and acted[-1] == min(450 + 2 * L + H - 1, 899)
        assert (np.abs(out) <= C_).all()


def test_the_integer_test_is_not_the_float_test():
    """at L = 512 one frame of q = U - 1 gives s = L U - 1, which rounds to g == 1.0f: `limited` counts it all the same"""
    C_ = f32(1.0)
    x = np.zeros(2000, f32)
    x[1000] = np.nextafter(C_, f32(np.inf))
    out, g, s = lh.limit(x, C_, 512, 0)
    assert (s < 512 * lh.U).sum() > 0 and (g[s == 512 * lh.U - 1] == 1).all() and (s == 512 * lh.U - 1).any()


# ---- the condition on the GPU tests' inputs ---------------------------------------------------------------------------------------------
def gpu_inputs():
    """(what, signal, (C, L, H)) of every limited bus of tests/test_gpu_bus_limit.py's bit-for-bit cases"""
    for name, db, recs, _ in lh.CASES:
        C_ = lh.design(db, 1.0, 0.0, 48000.0)[0]
        for b, (L, H) in enumerate(recs):
            yield f"{name} bus {b}", lh.signal(C_, lh.SEEDS[b], kind=lh.KINDS[b]), (C_, L, H)
    for b, x, rec in lh.mixed_buses(lambda db: lh.design(db, 1.0, 0.0, 48000.0)[0]):
        if rec is not None and x is not None:
            yield f"mixed bus {b}", x, rec


def test_the_gpu_inputs_make_every_limiter_act():
    seen = 0
    for what, x, (C_, L, H) in gpu_inputs():
        assert lh.design(0.0, lh.ms(L), lh.ms(H), 48000.0)[1:] == (L, H), what
        out, g, s = lh.limit(x, C_, L, H)
        limited = int((s < L * lh.U).sum())
        assert 0 < limited < len(x), (what, limited)
        assert (np.abs(out) == C_).any(), what
        assert (np.abs(out) <= C_).all(), what
        seen += 1
    assert seen >= 6 + 20
