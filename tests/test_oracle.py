"""Pins the CPU oracle before anything is compared with it (CPU-only tests).

  1. the reference's own golden vectors: input_batch/output_batch of the six
     bundled models, threshold TEST_MODEL_THR = 1e-5 (rt-neural-generic.h:182,
     testModel rt-neural-generic.cpp:900-955);
  2. dsp_ref.npz: outputs of the reference's own Biquad.cpp / ValueSmoother.hpp
     (bit-exact), dsp_ref_random.json: digests of its Biquad's outputs for random
     designs, and live against oracle/_ref when that library is present;
  3. nn_*.npz: torch-CPU outputs for what the reference leaves unpinned.
"""
import ctypes as C
import os

import numpy as np
import pytest

from oracle import oracle as O
from tests import modelgen

THR = 1.0e-5          # rt-neural-generic.h:182


def test_bundled_goldens_pin_lstm(bundled_models):
    assert len(bundled_models) == 6
    for path in bundled_models:
        spec = O.load_model(path)
        assert (spec.rnn_type, spec.hidden, spec.input_size, spec.input_skip) == ("lstm", 12, 1, 0)
        assert spec.samplerate == 48000.0            # metadata.samplerate is a string -> default applies
        assert spec.input_batch.size == 2048 and spec.output_batch.size == 2048
        m = O.OracleModel(spec, warmup=False)        # DEBUG self-test path starts from reset()
        n_err, max_err, _ = m.test_model(spec.input_batch, spec.output_batch, THR)
        assert n_err == 0, (path, max_err)
        assert max_err < 2.5e-6


def test_gate_order_is_uniquely_pinned(bundled_models):
    """Swapping any two gate blocks must break the golden."""
    import copy
    import json
    with open(bundled_models[0]) as f:
        j = json.load(f)
    H = 12
    for a, b in ((0, 1), (0, 2), (1, 3), (2, 3)):
        jj = copy.deepcopy(j)
        for wi in range(3):
            w = np.asarray(jj["layers"][0]["weights"][wi], np.float32)
            blk_a = w[..., a * H:(a + 1) * H].copy()
            w[..., a * H:(a + 1) * H] = w[..., b * H:(b + 1) * H]
            w[..., b * H:(b + 1) * H] = blk_a
            jj["layers"][0]["weights"][wi] = w.tolist()
        spec = O.parse_model(jj)
        n_err, max_err, _ = O.OracleModel(spec, warmup=False).test_model(spec.input_batch, spec.output_batch, THR)
        assert n_err > 0 and max_err > 1e-3


def test_timing_flavour_with_vectorised_activations_also_meets_the_goldens(bundled_models):
    """The cpu_baseline leg of bench.py times flavour 2 (branch-free exp/tanh); it must be a correct
    implementation too, not just a fast one."""
    for path in bundled_models:
        spec = O.load_model(path)
        y = O.net_run(spec, spec.input_batch.reshape(-1, 1), flavour=2)
        assert np.abs(y - spec.output_batch).max() < 2.5e-6, path
    spec = O.parse_model(modelgen.make_model("gru", 24, 3, seed=5))
    X = modelgen.golden_inputs("x", 3)[:1024]
    assert np.abs(O.net_run(spec, X, flavour=2) - O.net_run(spec, X)).max() < 2e-6


def test_f64_shadow_agrees(bundled_models):
    spec = O.load_model(bundled_models[2])
    a = O.OracleModel(spec, warmup=False).test_model(spec.input_batch, spec.output_batch)[2]
    b = O.OracleModel(spec, warmup=False, f64=True).test_model(spec.input_batch, spec.output_batch)[2]
    assert np.abs(a - b).max() < 2e-6


@pytest.mark.parametrize("name", sorted(modelgen.GOLDEN_CASES))
def test_torch_goldens(name, golden_dir):
    kw = modelgen.GOLDEN_CASES[name]
    g = np.load(os.path.join(golden_dir, f"nn_{name}.npz"))
    spec = O.parse_model(modelgen.make_model(**kw))
    y = O.net_run(spec, g["X"])
    err = np.abs(y - g["y"]).max()
    assert err < THR, (name, err)


# ------------------------------------------------------------------ DSP half

def _fp(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def test_biquad_designs_and_responses_bit_exact(golden_dir):
    g = np.load(os.path.join(golden_dir, "dsp_ref.npz"))
    L = O.lib()
    for i, (t, fc, q, gain) in enumerate(g["designs"]):
        f = O.Biquad()
        L.orc_biquad_init(C.byref(f), int(t), fc, q, gain)
        got = np.array([f.a0, f.a1, f.a2, f.b1, f.b2])
        assert np.array_equal(got, g["coeffs"][i]), (i, got, g["coeffs"][i])
        out = np.empty_like(g["imp"])
        L.orc_biquad_block(C.byref(f), _fp(out), _fp(np.ascontiguousarray(g["imp"])), out.size)
        assert np.array_equal(out, g["imp_out"][i]), i
        L.orc_biquad_init(C.byref(f), int(t), fc, q, gain)
        out = np.empty_like(g["noise"])
        L.orc_biquad_block(C.byref(f), _fp(out), _fp(np.ascontiguousarray(g["noise"])), out.size)
        assert np.array_equal(out, g["noise_out"][i]), i


def test_biquad_coefficient_change_keeps_state(golden_dir):
    g = np.load(os.path.join(golden_dir, "dsp_ref.npz"))
    L = O.lib()
    noise = np.ascontiguousarray(g["noise"])
    f = O.Biquad()
    L.orc_biquad_init(C.byref(f), O.BQ_PEAK, 750.0 / 48000.0, 0.707, 0.0)
    out = np.empty_like(noise)
    L.orc_biquad_block(C.byref(f), _fp(out), _fp(noise), 400)
    L.orc_biquad_set(C.byref(f), O.BQ_BANDPASS, 900.0 / 48000.0, 2.5, 6.0)
    tail = np.empty(noise.size - 400, np.float32)
    L.orc_biquad_block(C.byref(f), _fp(tail), _fp(np.ascontiguousarray(noise[400:])), tail.size)
    out[400:] = tail
    assert np.array_equal(out, g["chg_out"])


def _run_smoother(kind, sr, tc, script, n):
    L = O.lib()
    s = (O.ExpSm if kind == "expsm" else O.LinSm)()
    getattr(L, f"orc_{kind}_init")(C.byref(s))
    getattr(L, f"orc_{kind}_set_sample_rate")(C.byref(s), sr)
    getattr(L, f"orc_{kind}_set_time_constant")(C.byref(s), tc)
    getattr(L, f"orc_{kind}_set_target")(C.byref(s), script[0][1])
    getattr(L, f"orc_{kind}_clear_to_target")(C.byref(s))
    out = np.zeros(n, np.float32)
    pos = 0
    nxt = getattr(L, f"orc_{kind}_next")
    for at, tgt in script[1:] + [(n, None)]:
        for i in range(pos, at):
            out[i] = nxt(C.byref(s))
        pos = at
        if tgt is not None:
            getattr(L, f"orc_{kind}_set_target")(C.byref(s), tgt)
    return out


def test_smoothers_bit_exact(golden_dir):
    g = np.load(os.path.join(golden_dir, "dsp_ref.npz"))
    cases = {
        "exp_a": ("expsm", 48000.0, 0.1, [(0, 0.0), (0, 1.0)], 6000),
        "exp_b": ("expsm", 44100.0, 0.1, [(0, 1.0), (0, 3.98107), (1000, 0.25), (1500, 0.0)], 4000),
        "lin_a": ("linsm", 48000.0, 0.1, [(0, 0.0), (0, 1.0)], 6000),
        "lin_b": ("linsm", 48000.0, 0.1, [(0, 0.2), (0, 0.9), (1000, 0.1), (1001, 0.1 + 1e-8), (3000, 0.5)], 9000),
    }
    for k, args in cases.items():
        assert np.array_equal(_run_smoother(*args), g[k]), k


def test_smoother_shapes_match_reference_smoke_program(golden_dir):
    """tests/src/test_smoothers.cpp prints 0->1 ramps: linear reaches 1.00 at i=4800,
    exponential reads ~1.00 (2 decimals) by ~i=4600."""
    g = np.load(os.path.join(golden_dir, "dsp_ref.npz"))
    lin, ex = g["lin_a"], g["exp_a"]
    assert lin[4800] == 1.0 and lin[4799] < 1.0         # i=4800 is the first printed 1.00
    assert round(float(ex[4600]), 2) == 1.00 and ex[5999] < 1.0      # asymptotic, never reaches


def test_live_reference_library_when_present(golden_dir):
    """Random designs + random audio through the restatement vs the reference's own
    Biquad, bit for bit: against the digests of its outputs recorded in
    dsp_ref_random.json everywhere, and live against oracle/_ref where that library
    is built."""
    import hashlib
    import json
    R = O.ref_lib()
    with open(os.path.join(golden_dir, "dsp_ref_random.json")) as f:
        rec = json.load(f)
    L = O.lib()
    rs = np.random.RandomState(rec["seed"])
    x = rs.uniform(-1, 1, rec["n_samples"]).astype(np.float32)
    assert len(rec["cases"]) == 200
    for t_, fc_, q_, gain_, digest in rec["cases"]:
        t = int(rs.randint(0, 7))
        fc = float(rs.uniform(0.0005, 0.49))
        q = float(rs.uniform(0.2, 5.0))
        gain = float(rs.uniform(-12, 12))
        assert (t, fc, q, gain) == (t_, fc_, q_, gain_)              # the recorded case is the one drawn here
        f = O.Biquad()
        L.orc_biquad_init(C.byref(f), t, fc, q, gain)
        got = np.empty_like(x)
        L.orc_biquad_block(C.byref(f), _fp(got), _fp(x), x.size)
        assert hashlib.sha256(got.tobytes()).hexdigest() == digest, (t, fc, q, gain)
        if R is not None:
            h = R.ref_biquad_new(t, fc, q, gain)
            want = np.empty_like(x)
            R.ref_biquad_block(h, _fp(want), _fp(x), x.size)
            R.ref_biquad_free(h)
            assert np.array_equal(got, want), (t, fc, q, gain)


# ------------------------------------------------------------------ chain semantics

def test_plugin_is_silent_until_a_model_is_applied():
    x = modelgen.signal(1, 512)[0]
    p = O.OraclePlugin()
    out = p.run(O.default_controls(), x)
    assert np.all(out == 0.0)            # loading=true -> master target 0, mem cleared to 0


def test_disabled_is_a_raw_copy_and_state_does_not_advance(bundled_models):
    spec = O.load_model(bundled_models[4])
    x = modelgen.signal(1, 512)[0]
    a, b = O.OraclePlugin(), O.OraclePlugin()
    a.set_model(O.OracleModel(spec))
    b.set_model(O.OracleModel(spec))
    off = O.default_controls(enabled=0.0)
    on = O.default_controls()
    assert np.array_equal(a.run(off, x[:256]), x[:256])
    assert np.array_equal(a.run(on, x[256:]), b.run(on, x[256:]))


def test_block_size_invariance(bundled_models):
    spec = O.load_model(bundled_models[0])
    x = modelgen.signal(1, 1024)
    c = O.default_controls(bass_boost_db=4.0, mid_boost_db=-3.0, mid_q=1.2, treble_boost_db=2.0,
                           depth_boost_db=3.0, presence_boost_db=3.0, pregain_db=3.0, master_db=-2.0)
    a = O.run_streams(spec, c, x, 256)
    b = O.run_streams(spec, c, x, 64)
    d = O.run_streams(spec, c, x, 1024)
    assert np.array_equal(a, b) and np.array_equal(a, d)


def test_bandpass_mode_runs_only_mid(bundled_models):
    spec = O.load_model(bundled_models[0])
    x = modelgen.signal(1, 512)
    c1 = O.default_controls(mid_type=1.0, bass_boost_db=6.0, treble_boost_db=-6.0)
    c2 = O.default_controls(mid_type=1.0)
    assert np.array_equal(O.run_streams(spec, c1, x, 256), O.run_streams(spec, c2, x, 256))


def test_cpu_bench_matches_python_driver(bundled_models):
    spec = O.load_model(bundled_models[1])
    x = modelgen.signal(3, 128)
    c = O.default_controls()
    secs, last = O.cpu_bench(spec, c, x, n_blocks=2, warm_blocks=1, n_threads=2)
    want = O.run_streams(spec, c, np.concatenate([x, x, x], axis=1), 128)[:, 256:]
    assert secs > 0 and np.array_equal(last, want)
