"""The stream tuners, host side (no device): the header declares the calls and both library builds export them, the structs' layouts as
the binding sees them, the argument checks made before any device is touched, aidax_tuner_design against the restatement
(tests/tunehelp.py) at 44.1, 48 and 96 kHz, aidax_tuner_note around a note's edges, and the restatement itself in fp64 on synthetic
plucked strings: within 1 cent of f0 (measured on the CPU: 0.24 cents at worst), white noise unvoiced."""
import ctypes as C
import importlib
import os

import numpy as np
import pytest

from tests import tunehelp as th

ax = importlib.import_module("aidadsp-lv2_amd")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG = -1
CALLS = ("aidax_tuner_params_default", "aidax_tuner_design", "aidax_tuner_note", "aidax_pool_set_tuning", "aidax_pool_tuning",
         "aidax_pool_set_tuner", "aidax_pool_stream_tuner", "aidax_pool_read_tuners", "aidax_pool_read_tuner_curve")


def test_the_calls_are_declared_and_both_builds_export_them():
    for name in CALLS:
        assert name in ax.declared_symbols() and hasattr(ax.lib(), name), name
    for build in ("lib", os.path.join("lib", "hooks")):
        so = C.CDLL(os.path.join(ROOT, "aidadsp-lv2_amd", build, "libaidax_hip.so"))
        for name in CALLS:
            assert hasattr(so, name), (build, name)


def test_the_structs_are_the_headers():
    assert (C.sizeof(ax.TunerParams), C.sizeof(ax.TunerRec), C.sizeof(ax.TunerReadingStruct), ax.TunerReading.itemsize) == (28, 40, 32, 32)
    assert [(n, getattr(ax.TunerRec, n).offset) for n, _ in ax.TunerRec._fields_] == [
        ("window", 0), ("hop", 4), ("tmin", 8), ("tmax", 12), ("threshold", 16), ("clarity_min", 20), ("level_min", 24), ("reserved", 28), ("samplerate", 32)]
    assert [(n, getattr(ax.TunerReadingStruct, n).offset) for n, _ in ax.TunerReadingStruct._fields_] == [
        ("frame", 0), ("analyses", 8), ("lag", 12), ("hz", 16), ("period", 20), ("clarity", 24), ("level", 28)]
    assert ax.TunerReading.names == tuple(n for n, _ in ax.TunerReadingStruct._fields_)
    assert [ax.TunerReading.fields[n][1] for n in ax.TunerReading.names] == [0, 8, 12, 16, 20, 24, 28]
    p = ax.tuner_params()
    assert (p.window, p.hop, p.f_min, p.f_max, p.clarity_min, p.level_min_db) == (2048, 1024, 70.0, 1400.0, 0.5, -60.0)
    assert np.float32(p.threshold) == np.float32(0.93)


def _refused(samplerate=48000.0, **kw):
    with pytest.raises(ax.AidaxError) as e:
        ax.tuner_design(samplerate, ax.tuner_params(**kw))
    assert e.value.code == ERR_ARG and th.design(samplerate, **kw) is None, kw
    return str(e.value)


def test_the_argument_checks_ahead_of_any_device():
    L = ax.lib()
    assert L.aidax_pool_set_tuning(None, C.byref(ax.tuner_params())) == ERR_ARG and b"null pool" in L.aidax_last_error()
    assert L.aidax_pool_set_tuning(None, None) == ERR_ARG
    assert L.aidax_pool_set_tuner(None, 0, 1) == ERR_ARG and b"null pool" in L.aidax_last_error()
    assert L.aidax_pool_stream_tuner(None, 0, None, None) == ERR_ARG
    out = ax.TunerReadingStruct()
    assert L.aidax_pool_read_tuners(None, 0, 1, C.byref(out)) == ERR_ARG and b"null" in L.aidax_last_error()
    assert L.aidax_pool_read_tuner_curve(None, 0, None, 1) == ERR_ARG
    assert L.aidax_pool_tuning(None, None) == 0
    rec = ax.TunerRec()
    assert L.aidax_tuner_design(48000.0, None, C.byref(rec)) == ERR_ARG and L.aidax_tuner_design(48000.0, C.byref(ax.tuner_params()), None) == ERR_ARG
    for window in (0, 512, 1000, 2047, 3072, 8192):
        assert "window" in _refused(window=window)
    for hop in (0, 16, 48, 63, 65, 1000, 65537, 65552, 1 << 20):
        assert "hop" in _refused(hop=hop)
    assert "tmax" in _refused(f_min=46.0)                                 # ceil(48000 / 46) = 1044 > 1023
    assert "tmax" in _refused(window=1024, f_min=93.0)                    # 517 > 511
    assert "tmax" in _refused(samplerate=96000.0, f_min=70.0)             # 1372 > 1023
    assert "tmin" in _refused(f_max=30000.0)
    assert "f_min" in _refused(f_min=2000.0)                              # above f_max
    assert "f_min" in _refused(f_min=0.0) and "finite" in _refused(f_max=float("inf")) and "finite" in _refused(threshold=float("nan"))
    assert "threshold" in _refused(threshold=0.0) and "threshold" in _refused(threshold=1.5)
    assert "clarity_min" in _refused(clarity_min=-0.1) and "level_min_db" in _refused(level_min_db=1.0)
    assert "samplerate" in _refused(samplerate=0.0) and "samplerate" in _refused(samplerate=float("nan"))


@pytest.mark.parametrize("rate", (44100.0, 48000.0, 96000.0))
def test_the_design_is_the_restatements(rate):
    rs = np.random.RandomState(int(rate))
    cases = [dict(window=4096), dict(window=4096, hop=64, f_min=50.0, f_max=2000.0), dict(window=1024, hop=65536, f_min=200.0, f_max=4000.0, level_min_db=-300.0),
             dict(window=4096, f_min=rate / 2047.0 * 1.0001, f_max=rate / 2.0), dict(f_min=441.0, f_max=441.0, threshold=1.0, clarity_min=0.0, level_min_db=0.0)]
    cases += [dict(window=4096, hop=16 * int(rs.randint(4, 4097)), f_min=float(rs.uniform(50, 300)), f_max=float(rs.uniform(300, 5000)),
                   threshold=float(rs.uniform(0.5, 1.0)), clarity_min=float(rs.uniform(0, 1)), level_min_db=float(rs.uniform(-120, 0))) for _ in range(40)]
    for kw in cases:
        want = th.design(rate, **kw)
        assert want is not None, kw
        got = ax.tuner_design(rate, ax.tuner_params(**kw))
        assert (got.window, got.hop, got.tmin, got.tmax, got.samplerate, got.reserved) == (want["window"], want["hop"], want["tmin"], want["tmax"], rate, 0.0), kw
        assert (np.float32(got.threshold), np.float32(got.clarity_min)) == (want["threshold"], want["clarity_min"])
        assert abs(np.float32(got.level_min) - want["level_min"]) <= np.spacing(want["level_min"]), kw
        assert got.tmin >= 2 and got.tmax <= got.window // 2 - 1 and rate / got.tmax <= kw.get("f_min", 70.0) * (1 + 1e-6) and rate / got.tmin >= kw.get("f_max", 1400.0) * (1 - 1e-6)
    assert ax.tuner_design(rate, ax.tuner_params(window=4096, level_min_db=-300.0)).level_min == 0.0


def test_the_note_of_a_frequency():
    assert ax.tuner_note(440.0) == (69, 0.0)
    note, cents = ax.tuner_note(82.41)                                    # E2
    assert note == 40 and abs(cents - 1200.0 * np.log2(82.41 / (440.0 * 2.0 ** ((40 - 69) / 12.0)))) < 1e-4 and abs(cents) < 0.1
    assert ax.tuner_note(432.0, 432.0) == (69, 0.0) and ax.tuner_note(880.0)[0] == 81 and ax.tuner_note(27.5)[0] == 21
    for base in (40, 69, 88):
        f = 440.0 * 2.0 ** ((base - 69) / 12.0)
        for off, want_note, want_cents in ((49.9, base, 49.9), (-49.9, base, -49.9), (50.1, base + 1, -49.9), (-50.1, base - 1, 49.9)):
            note, cents = ax.tuner_note(f * 2.0 ** (off / 1200.0))
            assert note == want_note and abs(cents - want_cents) < 1e-3, (base, off, note, cents)
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ax.AidaxError) as e:
            ax.tuner_note(bad)
        assert e.value.code == ERR_ARG
    with pytest.raises(ax.AidaxError):
        ax.tuner_note(440.0, 0.0)
    assert ax.lib().aidax_tuner_note(440.0, 440.0, None, None) == ERR_ARG


def test_the_boundary_rule():
    assert th.crosses(0, 1024, 1024, 256) == (True, 1024) and th.crosses(0, 1023, 1024, 256) == (False, 768)
    assert th.crosses(1024, 1279, 1024, 256) == (False, 1024) and th.crosses(1024, 1280, 1024, 256) == (True, 1280)
    assert th.crosses(960, 1160, 1024, 64) == (True, 1152) and th.crosses(900, 1000, 1024, 64) == (False, 960)
    tr = th.Tracker(dict(window=1024, hop=64))
    assert [tr.feed(np.zeros(n, np.float32)) for n in (1000, 23, 1, 63, 1, 200)] == [False, False, True, False, True, True]
    assert (tr.pos, tr.frame, tr.analyses, len(tr.window)) == (1288, 1280, 3, 1024)


def test_the_restatement_tracks_plucked_strings_within_a_cent():
    """W = 2048 at 48 kHz over 70 .. 1400 Hz: E2 .. E6, four mixes of five partials (one with its fundamental at 0.05 of the second
    partial), a slow decay, noise 50 dB below the partials"""
    rec = th.design(48000.0)
    worst = 0.0
    for i, f0 in enumerate(th.FUNDAMENTALS):
        for m, mix in enumerate(th.MIXES):
            rd, n = th.analyse(th.string(f0, mix, 2048, seed=100 * i + m), rec)
            assert rd["lag"] > 0 and n[0] == 1.0 and rd["clarity"] > 0.9, (f0, m, rd)
            assert abs(rd["period"] - rd["lag"]) <= 0.5 and abs(rd["level"] - 0.25) < 0.05
            worst = max(worst, abs(th.cents(rd["hz"], f0)))
            assert abs(th.cents(rd["hz"], f0)) <= 1.0, (f0, m, rd)
    print(f"worst deviation: {worst:.3f} cents")


def test_white_noise_is_unvoiced():
    rec = th.design(48000.0, level_min_db=-90.0)
    rng = np.random.default_rng(3)
    rd, _ = th.analyse((rng.standard_normal(2048) * 1e-3).astype(np.float32), rec)
    assert rd["lag"] == 0 and rd["hz"] == 0 and rd["period"] == 0 and rd["clarity"] < 0.2 and abs(rd["level"] - 1e-3) < 1e-4, rd
    rd, _ = th.analyse(np.zeros(2048, np.float32), rec)
    assert (rd["lag"], rd["hz"], rd["clarity"], rd["level"]) == (0, 0.0, 0.0, 0.0)
    # a string below the level floor is unvoiced by its level alone: its clarity is still reported
    rd, _ = th.analyse(th.string(220.0, th.MIXES[0], 2048, level=1e-6, seed=9), rec)
    assert rd["lag"] == 0 and rd["hz"] == 0 and rd["clarity"] > 0.9 and rd["level"] < rec["level_min"]


def test_the_pick_on_rows_made_by_hand():
    n = np.zeros(42, np.float32)
    n[:4] = [1.0, 0.6, 0.2, -0.1]                                         # the lobe around lag 0
    n[8:13] = [0.1, 0.5, 0.5, 0.3, -0.2]                                  # a plateau: the later of two equal lags is the candidate ...
    n[20:25] = [0.2, 0.9, 0.4, 0.95, 0.1]                                 # ... two candidates in a lobe: the larger
    n[30:33] = [0.3, 0.9, 0.2]
    assert th.pick(n, 2, 40, 0.93) == (23, [10, 23, 31])
    assert th.pick(n, 2, 40, 0.5) == (10, [10, 23, 31])
    assert th.pick(n, 2, 40, 0.94) == (23, [10, 23, 31]) and th.pick(n, 24, 40, 0.93) == (31, [31])
    assert th.pick(n, 11, 22, 0.93) == (21, [21])                         # the range cuts candidates, not lobes
    n[23] = 0.9
    assert th.pick(n, 2, 40, 1.0) == (21, [10, 21, 31])                   # a tie inside a lobe: the earlier lag
    assert th.pick(np.ones(42, np.float32), 2, 40, 0.93) == (0, [])       # one lobe from lag 0 to the end
    n[:] = np.nan
    assert th.pick(n, 2, 40, 0.93) == (0, [])
