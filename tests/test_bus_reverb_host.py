"""The bus reverbs, host side (no device): aidax_bus_reverb_design against the formulas of include/aidax.h in Python floats and what it
refuses; the names the header declares; the properties of the rule (block cuts do not show, a changed gain keeps the tail, other delays,
off -> on and a reset cut it, wet = 0 and dry = 1 returns the sanitised input, the state stays bounded) on the numpy restatement the GPU
tests compare the kernel with (tests/reverbhelp.py); and the conditions on the GPU tests' inputs: by the restatement alone, for every
bit-for-bit case and every bus with its reverb on, the output differs from dry * x in at least half of the frames after the first m_min,
the frames issued are at least two ring rows (every line wraps) and eight times the longest delay (the feedback has gone round), and the
output is finite. A reverb that never sounds, or that never wraps, cannot pass them."""
import ctypes as C
import importlib
import struct

import numpy as np
import pytest

from tests import reverbhelp as rh

ax = importlib.import_module("aidadsp-lv2_amd")
ERR_ARG = -1
f32 = np.float32


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def _params(rt60_s=1.0, size=1.0, damping=0.3, wet=0.5, dry=1.0, variant=0):
    return ax.BusReverbParams(rt60_s, size, damping, wet, dry, variant)


def test_the_header_declares_the_calls_and_the_library_exports_them():
    names = ("aidax_bus_reverb_design", "aidax_pool_set_bus_reverbs", "aidax_pool_bus_reverbs", "aidax_pool_set_bus_reverb", "aidax_pool_set_bus_reverb_rec",
             "aidax_pool_bus_reverb", "aidax_pool_reset_bus_reverb")
    declared = ax.declared_symbols()
    for name in names:
        assert name in declared and hasattr(ax.lib(), name), name
    assert (ax.BUS_REVERB_LINES, ax.BUS_REVERB_MIN_DELAY, ax.BUS_REVERB_MAX_DELAY) == (8, 64, 32768) == (rh.LINES, rh.MIN_DELAY, rh.MAX_DELAY)
    assert C.sizeof(ax.BusReverbRec) == 96 and C.sizeof(ax.BusReverbParams) == 24
    for m in ("set_bus_reverbs", "bus_reverbs", "set_bus_reverb", "set_bus_reverb_rec", "bus_reverb", "reset_bus_reverb"):
        assert hasattr(ax.Pool, m), m
    with open(ax.binding._HEADER) as f:
        text = f.read()
    for word in ("#define AIDAX_BUS_REVERB_MIN_DELAY 64", "#define AIDAX_BUS_REVERB_MAX_DELAY 32768", "Bus reverbs", "a wet-only return to another bus"):
        assert word in text, word
    threads = text.split("/* Threads.")[1].split("*/")[0]
    for word in ("set_bus_reverbs after its first enabling call", "set_bus_reverb,", "set_bus_reverb_rec", "reset_bus_reverb", "aidax_bus_reverb_design"):
        assert word in threads, word


def _ulps(a, b):
    a, b = (int(np.asarray(v, f32).view(np.int32)) for v in (a, b))
    return abs(a - b)


@pytest.mark.parametrize("rate", (44100.0, 48000.0, 96000.0, 192000.0))
def test_design_is_the_formula(rate):
    seen = set()
    for variant in range(4):
        for size in (0.05, 0.1, 0.33, 1.0, 1.37, 2.0):
            for rt60 in (0.1, 0.5, 1.0, 3.3, 20.0):
                damping, wet, dry = 0.1 * variant + 0.05, 0.25 * variant - 0.3, 1.0 - variant
                r = ax.bus_reverb_design(_params(rt60, size, damping, wet, dry, variant), rate)
                want = rh.design(rt60, size, damping, wet, dry, variant, rate)
                assert tuple(r.m) == want.m, (variant, size, rt60)
                assert all(_ulps(g, w) <= 1 for g, w in zip(r.gq, want.gq)) and _ulps(r.a, want.a) <= 1
                assert (struct.pack("f", r.wet), struct.pack("f", r.dry)) == (want.wet.tobytes(), want.dry.tobytes()) and r.on == 1 and r.epoch == 0
                # ... and the record is one the pool admits
                assert want.valid() and all(k % 2 == 1 and k >= 65 for k in r.m) and len(set(r.m)) == 8
                assert all(0 < g < 1 / np.sqrt(8.0) for g in r.gq) and 0 <= r.a <= 0.5
                if size >= 0.33:
                    seen.add(tuple(r.m))
    assert len(seen) == 4 * 4                                     # from a third of the full size on every variant and size has delays of its own
    # a small room ends on the floor of 64 frames: made odd, then distinct
    assert tuple(ax.bus_reverb_design(_params(size=0.05, variant=0), 16000.0).m) == (65, 67, 69, 71, 73, 75, 77, 79) == rh.design(1.0, 0.05, 0.3, 0.5, 1.0, 0, 16000.0).m
    r = ax.bus_reverb_design(_params(), 48000.0)
    assert tuple(r.m) == rh.BASE[0]


def test_design_refuses():
    L = ax.lib()
    nan, inf = float("nan"), float("inf")

    def marked():
        out = ax.BusReverbRec()
        C.memset(C.byref(out), 0x5A, C.sizeof(out))
        return out

    out = marked()
    untouched = bytes(out)
    bad = [dict(rt60_s=0.09), dict(rt60_s=20.1), dict(rt60_s=nan), dict(rt60_s=inf), dict(rt60_s=-1.0),
           dict(size=0.049), dict(size=2.01), dict(size=nan), dict(size=0.0), dict(size=inf),
           dict(damping=-0.01), dict(damping=1.01), dict(damping=nan),
           dict(wet=4.01), dict(wet=-4.01), dict(wet=nan), dict(wet=inf), dict(dry=4.01), dict(dry=-4.01), dict(dry=nan), dict(dry=-inf),
           dict(variant=4), dict(variant=0xFFFFFFFF)]
    for kw in bad:
        p = _params(**kw)
        assert L.aidax_bus_reverb_design(C.byref(p), 48000.0, C.byref(out)) == ERR_ARG, kw
        assert bytes(out) == untouched and L.aidax_last_error()
        with pytest.raises(ax.AidaxError) as e:
            ax.bus_reverb_design(p, 48000.0)
        assert e.value.code == ERR_ARG
    p = _params()
    for rate in (0.0, -48000.0, nan, inf, 1e9):                  # (1e9: a delay beyond 32768 frames)
        assert L.aidax_bus_reverb_design(C.byref(p), rate, C.byref(out)) == ERR_ARG and bytes(out) == untouched, rate
    assert L.aidax_bus_reverb_design(None, 48000.0, C.byref(out)) == ERR_ARG and b"null" in L.aidax_last_error()
    assert L.aidax_bus_reverb_design(C.byref(p), 48000.0, None) == ERR_ARG
    # the bounds themselves are fine
    for kw in (dict(rt60_s=0.1, size=0.05, damping=0.0, wet=-4.0, dry=4.0, variant=3), dict(rt60_s=20.0, size=2.0, damping=1.0, wet=4.0, dry=-4.0)):
        ax.bus_reverb_design(_params(**kw), 192000.0)


def test_a_null_pool_is_an_argument_error_without_a_device():
    L = ax.lib()
    p, r = _params(), ax.BusReverbRec()
    assert L.aidax_pool_set_bus_reverbs(None, 1, 4096) == ERR_ARG and b"null" in L.aidax_last_error()
    assert L.aidax_pool_bus_reverbs(None) == 0
    assert L.aidax_pool_set_bus_reverb(None, 0, C.byref(p)) == ERR_ARG
    assert L.aidax_pool_set_bus_reverb_rec(None, 0, C.byref(r)) == ERR_ARG
    assert L.aidax_pool_bus_reverb(None, 0, None, None, None, None) == ERR_ARG
    assert L.aidax_pool_reset_bus_reverb(None, 0) == ERR_ARG


# ---- the restatement's properties ------------------------------------------------------------------------------------------------------
def _through(x, ref, cuts, between=None):
    at, outs, i = 0, [], 0
    while at < len(x):
        n = min(cuts[i % len(cuts)], len(x) - at)
        if between:
            between(i, at)
        i += 1
        outs.append(ref.process(x[None, at:at + n])[0])
        at += n
    return np.concatenate(outs)


SMALL = rh.CASES[0][1]


def test_cuts_do_not_show_and_the_state_stays_bounded():
    for k, rec in enumerate(SMALL):
        x = rh.signal(10 + k, 1500, "wild" if k == 1 else "plain")
        whole = rh.reverb(x, rec)
        ref = rh.Reference(1, 128)
        ref.set(0, rec)
        assert np.array_equal(bits(_through(x, ref, rh.PLAN1)), bits(whole)), k
        assert np.isfinite(whole).all() and np.isfinite(ref.hist).all() and ref.since[0] == 1500
    # full-scale noise into the longest decay a design admits, on short lines: bounded
    rec = rh.design(20.0, 0.05, 0.0, 1.0, 0.0, 0, 48000.0)
    y = rh.reverb(np.random.default_rng(3).choice(np.array([-1, 1], f32), 6000), rec)
    assert np.isfinite(y).all() and np.abs(y).max() < 1e4


def test_the_first_frames_are_dry_and_the_tail_sounds():
    rec = SMALL[0]
    x = np.zeros(1200, f32)
    x[0] = 1.0
    y = rh.reverb(x, rec)
    m_min = min(rec.m)
    assert y[0] == rec.dry and not y[1:m_min].any() and y[m_min] != 0 and np.count_nonzero(y[m_min:]) > 500
    # energy falls: the last third is quieter than the first
    assert np.abs(y[800:]).max() < np.abs(y[m_min:400]).max()


def test_wet_zero_dry_one_returns_the_sanitised_input():
    rec = rh.Rec(SMALL[1].m, SMALL[1].gq, SMALL[1].a, 0.0, 1.0)
    x = rh.signal(21, 900, "wild")
    assert np.array_equal(rh.reverb(x, rec), rh.sanitise(x)) and not np.isfinite(x).all()


def test_which_changes_cut_the_tail():
    base = SMALL[0]
    x = np.concatenate([rh.signal(31, 600), np.zeros(400, f32)]).astype(f32)
    m_min = min(base.m)

    def run(change):
        ref = rh.Reference(1, 128)
        ref.set(0, base)
        return _through(x, ref, [600, 400], lambda i, at: change(ref) if i == 1 else None)

    kept = run(lambda ref: None)
    assert kept[600:600 + m_min].any()                           # the tail of the first 600 frames sounds into the silence
    louder = run(lambda ref: ref.set(0, rh.Rec(base.m, base.gq * f32(0.5), 0.5, 2.0, base.dry)))
    assert louder[600:600 + m_min].any() and not np.array_equal(louder[600:], kept[600:])      # another gain: the memories stay
    other = tuple(k + 2 for k in base.m)
    for change in (lambda ref: ref.set(0, rh.Rec(other, base.gq, base.a, base.wet, base.dry)), lambda ref: ref.reset(0),
                   lambda ref: (ref.set(0, None), ref.set(0, base))):
        cut = run(change)
        assert np.array_equal(bits(cut[:600]), bits(kept[:600])) and not cut[600:].any()      # dry * 0 for good: nothing is left to sound


# ---- the conditions on the GPU tests' inputs --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [c[0] for c in rh.CASES])
def test_the_gpu_inputs_make_every_reverb_sound_wrap_and_go_round(name):
    recs, capacity, plan, x = rh.case(name)
    T = sum(plan)
    assert x.shape == (len(recs), T) and T >= 2 * rh.ring_row(capacity) and max(plan) <= rh.MAXF and 0 in plan
    ref = rh.Reference(len(recs), capacity)
    at, outs = 0, []
    for b, rec in enumerate(recs):
        assert rec.valid(capacity)
        ref.set(b, rec)
    for n in plan:
        outs.append(ref.process(x[:, at:at + n]))
        at += n
    out = np.concatenate(outs, axis=1)
    assert np.isfinite(out).all() and not np.isfinite(x[1]).all()
    for b, rec in enumerate(recs):
        m_min, m_max = min(rec.m), max(rec.m)
        assert T >= 8 * m_max, (name, b)
        dry = rec.dry * rh.sanitise(x[b])
        differs = bits(out[b, m_min:]) != bits(dry[m_min:])
        assert 2 * int(differs.sum()) >= T - m_min, (name, b, int(differs.sum()))
        assert np.array_equal(bits(out[b, :m_min]), bits(dry[:m_min] + rec.wet * f32(0)))      # ... and the first m_min frames are dry (+ wet * 0): nothing has come round yet
    if name == "smallest":
        assert all(min(r.m) == 64 and max(r.m) <= 79 for r in recs) and capacity == 128
    if name == "edges":
        assert [min(r.m) for r in recs] == [65, 255, 256, 257]
    if name == "long":
        assert [r.m for r in recs] == [rh.BASE[v] for v in (0, 1, 2)] and capacity == 4096


def test_the_mixed_case_covers_every_chunk_size():
    layout = list(rh.mixed_layout())
    assert len(layout) == 70 and sum(1 for _, s, _, _ in layout if s is not None) == 48 and sum(1 for *_, r in layout if r is None) == 14
    mins = {min(r.m) for *_, r in layout if r is not None}
    assert mins == set(rh.MIXED_MMIN) and all(r.valid(rh.MIXED_CAPACITY) for *_, r in layout if r is not None)
    assert {min(256, k) // 64 for k in mins} == {1, 2, 3, 4}
    assert sum(rh.MIXED_PLAN) >= 2 * rh.ring_row(rh.MIXED_CAPACITY)
