"""The streaming resampler (k_resample) and the rate adapter on the GPU (-m gpu), against tests/rateref.py, the independent numpy fp64
statement of the formulas in include/aidax.h. No test hook is used: the same tests run on the shipped library (the ship leg).

Bounds. A stage's output is an fp32 dot product of T terms: per sample |out - ref64| <= (T + 2) 2^-24 sum_i |w_i| |x_i| (T products and
T additions in fp32 with FMAs, gamma_T <= (T + 2) u for these T; the weights are the same fp32 numbers on both sides). No measured
number is in it; an fp32 emulation of the sum stays at <= 0.11 of it on these inputs. Around a transparent pool the second stage sees
the first one's error through its own weights: (T_B + 2) 2^-24 (|w_B| o |y|) + |w_B| o bound_A (rateref.adapter64; the emulation stays
at <= 0.04). The tone: the fp64 helper alone returns 0.5 sin(1 kHz) + 0.5 sin(5 kHz) delayed by the latency within 1.8e-7 (44.1 -> 48 kHz)
and 3.1e-7 (96 -> 48 kHz) after the first 400 frames, the passband ripple of the two filters; the bar, 1e-6, is that plus the typical
size of the fp32 bound (some 1e-7 per stage for samples of this size). Everything else is bit for bit.
Every ratio is printed before it is asserted and logged through tests/errlog.py; profiles/rate_adapter.txt keeps the largest."""
import importlib

import numpy as np
import pytest

from tests import errlog, modelgen, rateref as rr
from tests.ratehelp import adapter_and_its_parts, feed as _feed, noise as _noise, pool as _pool, stage as _stage

pytestmark = pytest.mark.gpu
ax = importlib.import_module("aidadsp-lv2_amd")
ERR_STATE = -6
RAGGED = (1, 7, 64, 255, 256, 17)                                          # 600 frames
N_IN = sum(RAGGED)
# (rate_in, rate_out, d_in, d_out): the five ratios, with and without delays on either side
STAGES = ((44100, 48000, 32, 0), (48000, 44100, 0, 34), (96000, 48000, 64, 0), (48000, 96000, 0, 0), (192000, 44100, 5, 3))


@pytest.mark.parametrize("ri,ro,d_in,d_out", STAGES)
def test_a_stage_against_fp64(ri, ro, d_in, d_out):
    S = 3
    x = _noise(S, N_IN, ri + ro)
    rs = _stage(S, ri, ro, d_in, d_out, 256)
    got = _feed(rs, x, RAGGED)
    rs.close()
    n_out = rr.ready(N_IN, ri, ro, d_in, d_out)
    assert got.shape == (S, n_out) and n_out > 100
    T = rr.params(ri, ro)[5]
    ref = rr.stage64(x, ri, ro, d_in, d_out, n_out)
    bound = (T + 2) * 2.0 ** -24 * rr.stage64(x, ri, ro, d_in, d_out, n_out, absolute=True)
    diff = np.abs(got.astype(np.float64) - ref)
    ratio = float(np.max(diff / np.maximum(bound, 1e-300)))
    print(f"rate stage {ri} -> {ro} (T = {T}): max |out - ref64| / bound = {ratio:.3f}")
    errlog.bound(ratio, 1.0 + 1e-12, f"rate_stage_{ri}_{ro}")
    assert np.all(diff <= bound)


@pytest.mark.parametrize("S", [3, 65])
@pytest.mark.parametrize("ri,ro,d_in,d_out", [STAGES[0], STAGES[4]])
def test_the_bits_do_not_depend_on_the_cut(S, ri, ro, d_in, d_out):
    x = _noise(S, N_IN, S)
    one = _stage(S, ri, ro, d_in, d_out, N_IN)
    whole = _feed(one, x, (N_IN,))
    one.close()
    rs = _stage(S, ri, ro, d_in, d_out, 256)
    ragged = _feed(rs, x, RAGGED)
    rs.close()
    assert whole.shape == ragged.shape and np.array_equal(whole.view(np.uint32), ragged.view(np.uint32))
    # stream 1 reset after 327 frames = a run whose stream 1 had zeros before that point
    at = sum(RAGGED[:4])
    rs = _stage(S, ri, ro, d_in, d_out, 256)
    with_reset = _feed(rs, x, RAGGED, reset=(1, at))
    rs.close()
    z = x.copy()
    z[1, :at] = 0.0
    rs = _stage(S, ri, ro, d_in, d_out, 256)
    zeros_before = _feed(rs, z, RAGGED)
    rs.close()
    done = rr.ready(at, ri, ro, d_in, d_out)                               # outputs taken before the reset keep the true past
    assert np.array_equal(with_reset[:, :done], ragged[:, :done])
    assert np.array_equal(with_reset[:, done:].view(np.uint32), zeros_before[:, done:].view(np.uint32))
    assert not np.array_equal(with_reset[1, done:], ragged[1, done:]) and np.array_equal(with_reset[0], ragged[0])


def test_the_exact_cases():
    S = 3
    x = _noise(S, N_IN, 11)
    x[0, 5] = -0.0
    rs = _stage(S, 48000, 48000, 3, 4, 256)                                 # equal rates: the input d_in + d_out frames late, bit for bit
    got = _feed(rs, x, RAGGED)
    rs.close()
    assert got.shape[1] == N_IN - 32 + 3 + 4
    want = np.concatenate([np.zeros((S, 7), np.float32), x], axis=1)[:, :got.shape[1]]
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    rs = _stage(S, 48000, 96000, 0, 0, 256)                                 # 2 / 1: every even output is an input frame
    got = _feed(rs, x, RAGGED)
    rs.close()
    n = got.shape[1]
    assert n == rr.ready(N_IN, 48000, 96000) and np.array_equal(got[:, 0:n:2], x[:, :(n + 1) // 2])


def test_an_output_too_many_is_refused_and_the_stage_goes_on():
    S, ri, ro = 2, 44100, 48000
    x = _noise(S, 200, 4)
    rs = _stage(S, ri, ro, 0, 0, 256)
    assert rs.ready == 0
    assert rs.process(x[:, :100], 0).shape == (S, 0)
    ready = rs.ready
    assert ready == rr.ready(100, ri, ro) > 0
    with pytest.raises(ax.AidaxError) as e:
        rs.process(x[:, :0], ready + 1)
    assert e.value.code == ERR_STATE and "outputs asked for" in str(e.value)
    with pytest.raises(ax.AidaxError) as e:                                 # ... also when the call brings frames: none of them is appended
        rs.process(x[:, 100:101], rr.ready(101, ri, ro) + 1)
    assert e.value.code == ERR_STATE and rs.ready == ready
    got = np.concatenate([rs.process(x[:, :0], ready), rs.process(x[:, 100:])], axis=1)
    rs.close()
    ref = rr.stage64(x, ri, ro, 0, 0, got.shape[1])
    assert got.shape[1] == rr.ready(200, ri, ro)
    assert np.all(np.abs(got - ref) <= 67 * 2.0 ** -24 * rr.stage64(x, ri, ro, 0, 0, got.shape[1], absolute=True))


# ---- the adapter

@pytest.fixture(scope="module")
def model(tmp_path_factory):
    p = str(tmp_path_factory.mktemp("rate") / "lstm16.json")
    modelgen.write_model(modelgen.make_model(kind="lstm", hidden=16, input_size=1, seed=5), p)
    return ax.Model(p)


@pytest.mark.parametrize("host", [44100, 96000])
def test_the_adapter_around_a_transparent_pool(model, host):
    S, pool_rate = 3, 48000
    p = _pool(model, S, 288, ax.default_controls(enabled=0.0))
    ad = ax.RateAdapter(p, float(host), 256)
    lat = ad.latency_frames
    assert lat == rr.latency(host, pool_rate) == ax.rate_latency(float(host), float(pool_rate))
    x = _noise(S, N_IN, host)
    got, at = [], 0
    for n in RAGGED:
        got.append(ad.process(np.ascontiguousarray(x[:, at:at + n])))
        at += n
    got = np.concatenate(got, axis=1)
    ref, bound = rr.adapter64(x, host, pool_rate)
    diff = np.abs(got.astype(np.float64) - ref)
    ratio = float(np.max(diff / np.maximum(bound, 1e-300)))
    print(f"rate adapter {host} -> {pool_rate} -> {host}: max |out - B64(A64(x))| / bound = {ratio:.3f}")
    errlog.bound(ratio, 1.0 + 1e-12, f"rate_adapter_{host}")
    assert np.all(diff <= bound)
    ad.close()
    # a tone comes back `latency_frames` late (a fresh adapter: the stages start from silence)
    ad = ax.RateAdapter(p, float(host), 256)
    N = 1024
    t = np.arange(N) / host
    tone = np.tile((0.5 * np.sin(2 * np.pi * 1000 * t) + 0.5 * np.sin(2 * np.pi * 5000 * t)).astype(np.float32), (S, 1))
    back = np.concatenate([ad.process(np.ascontiguousarray(tone[:, i:i + 256])) for i in range(0, N, 256)], axis=1)
    ad.close()
    p.close()
    err = float(np.abs(back[:, 400:].astype(np.float64) - tone[:, 400 - lat:N - lat]).max())
    print(f"rate adapter {host}: tone delayed by {lat} frames within {err:.3e}")
    errlog.bound(err, 1e-6, f"rate_tone_{host}")


HOST_BLOCKS = (64, 1, 0, 255, 17, 256, 0, 7, 128)


def _adapter_and_its_parts(model, ir):
    """LSTM-16 with the EQ and the gains on, 5 streams at 44.1 kHz around pools at 48 kHz, ragged host blocks with n = 1 and n = 0"""
    return adapter_and_its_parts(model, ir, HOST_BLOCKS)


@pytest.mark.parametrize("with_ir", [False, True])
def test_the_adapter_is_its_parts(model, with_ir):
    ir = (np.random.default_rng(8).standard_normal(8) * 0.3).astype(np.float32) if with_ir else None
    got, want, p1, ad, p2 = _adapter_and_its_parts(model, ir)
    assert got.shape == (5, sum(HOST_BLOCKS)) and np.abs(want).max() > 1e-3
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    # lifetime: after close() the pool plays on by itself, on its own stream, from the state the adapter's passes left
    ad.close()
    blk = modelgen.signal(5, 256, seed=3)
    assert np.array_equal(p1.process(blk).view(np.uint32), p2.process(blk).view(np.uint32))
    p1.sync()
    p1.close()
    p2.close()


def test_equal_rates_forward_to_the_pool(model):
    S = 3
    ctl = ax.default_controls(eq_bypass=0.0, bass_boost_db=4.0)
    p1, p2 = _pool(model, S, 256, ctl), _pool(model, S, 256, ctl)
    ad = ax.RateAdapter(p1, 48000.0, 256)
    assert ad.latency_frames == 0
    x = modelgen.signal(S, 320, seed=9)
    for a, b in ((0, 256), (256, 256), (256, 320)):                         # 256 frames, the pre-run, 64 frames
        blk = np.ascontiguousarray(x[:, a:b])
        assert np.array_equal(ad.process(blk).view(np.uint32), p2.process(blk).view(np.uint32))
    ad.close()
    blk = np.ascontiguousarray(x[:, :64])
    assert np.array_equal(p1.process(blk).view(np.uint32), p2.process(blk).view(np.uint32))
    p1.sync()
    p1.close()
    p2.close()


def test_the_adapter_refuses_what_the_pool_cannot_take(model):
    p = ax.Pool(2, 256, 48000.0)
    with pytest.raises(ax.AidaxError) as e:
        ax.RateAdapter(p, 44100.0, 256)                                     # 256 host frames are up to 279 at 48 kHz
    assert e.value.code == -1 and "279" in str(e.value)
    ad = ax.RateAdapter(p, 44100.0, 235)                                    # ceil(235 * 160 / 147) = 256
    with pytest.raises(ax.AidaxError):
        ad.process(np.zeros((2, 236), np.float32))
    ad.close()
    p.close()
