"""A 48 kHz cabinet IR in pools at other host rates (GPU, -m gpu): ax.load_ir_wav_for reads the file, converts it to the pool's rate
(aidax_ir_resample) and cuts it to the pool's capacity; the pool then plays it like any IR.

The source is an 8192-frame 48 kHz mono 24-bit PCM file the test writes itself, shaped like the cabinet IRs the reference ships:
seeded exponentially decaying noise. The taps the pool must be using are those of tests/irresample.py, the independent fp64 statement
of the resampler's formula, rounded once to fp32, and the pool's output is held to their fp64 convolution with the dry signal under the
project's bound for one convolution, TAU = 4e-6 per sample against (|h| * |dry|)_t (tests/test_gpu_ir.py). The pools run a real model
with every stream disabled, so the dry signal is the test's input bit for bit. 44.1 kHz fits the default capacity (7558 + lead taps);
96 and 192 kHz need it raised (16447 and 32893 + lead)."""
import importlib

import numpy as np
import pytest

from tests import irresample as rs, modelgen
from tests.test_gpu_ir import TAU, _tau
from tests.test_ir_host import _chunk, _encode, _fmt, _riff

pytestmark = pytest.mark.gpu
ax = importlib.import_module("aidadsp-lv2_amd")
FILE_RATE, FILE_FRAMES = 48000, 8192


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    p = str(tmp_path_factory.mktemp("ir_rates") / "lstm16.json")
    modelgen.write_model(modelgen.make_model(kind="lstm", hidden=16, input_size=1, seed=5), p)
    return ax.Model(p)


@pytest.fixture(scope="module")
def cabinet(tmp_path_factory):
    """(path, taps): the file and the samples a reader must return for it"""
    rng = np.random.default_rng(8192)
    h = rng.standard_normal(FILE_FRAMES) * np.exp(-np.arange(FILE_FRAMES) / 900.0)
    raw = np.round(h / np.abs(h).max() * 0.9 * (1 << 23)).astype(np.int64).reshape(-1, 1)
    path = tmp_path_factory.mktemp("ir_rates_wav") / "cab48k.wav"
    path.write_bytes(_riff(_fmt(1, 1, FILE_RATE, 24), _chunk(b"data", _encode(raw, 1, 24))))
    return str(path), (raw[:, 0] / float(1 << 23)).astype(np.float32)


def _pool(model, S, n, sr, capacity=None):
    p = ax.Pool(S, n, float(sr))
    p.set_model(model)
    p.set_controls(ax.default_controls(enabled=0.0))
    if capacity:
        p.set_ir_capacity(capacity)
    return p


@pytest.mark.parametrize("sr,capacity", [(44100, None), (96000, 32768), (192000, 65536)])
@pytest.mark.parametrize("full_lead", [False, True])
def test_a_48k_cabinet_plays_at_the_pools_rate(model, cabinet, sr, capacity, full_lead):
    path, file_taps = cabinet
    lead = rs.full_lead(FILE_RATE, sr) if full_lead else 0
    S, n = 3, 256
    p = _pool(model, S, n, sr, capacity)
    x0 = modelgen.signal(S, n, seed=1)
    assert np.array_equal(p.process(x0), x0)                            # the premise: dry = input
    # the pool refuses the file's taps at the file's rate, as ever: the conversion is the caller's step
    with pytest.raises(ax.AidaxError) as e:
        p.set_ir(file_taps, samplerate=float(FILE_RATE))
    assert "differs from the pool's" in str(e.value)
    taps = ax.load_ir_wav_for(p, path, lead)
    want = rs.resample(file_taps, FILE_RATE, sr, lead)
    assert want.size == rs.n_full(FILE_FRAMES, FILE_RATE, sr, lead) <= p.ir_capacity()
    # the library's taps against the helper's: the bound of tests/test_ir_resample_host.py
    w64 = rs.resample64(file_taps, FILE_RATE, sr, lead)
    assert taps.size == want.size
    assert np.all(np.abs(taps.astype(np.float64) - want) <= 2.0 ** -23 * np.abs(w64) + 1e-12 * np.abs(file_taps).sum())
    p.set_ir(taps)
    T = (want.size + 4 * n) // n * n
    x = modelgen.signal(S, T, seed=int(sr) + lead)
    got = np.concatenate([p.process(np.ascontiguousarray(x[:, i:i + n])) for i in range(0, T, n)], axis=1)
    p.close()
    worst = _tau(f"rates{sr}lead{lead}", got, x, want)
    print(f"ir_rates 48000 -> {sr}, lead {lead}, {want.size} taps: max |y - y64| / (|h| * |dry|) = {worst:.3e} (bound {TAU:.0e})")
    # with the full lead the cabinet is the file's, `lead` frames late: an impulse comes out as the file's DC gain, summed
    assert abs(float(want.astype(np.float64).sum()) - float(file_taps.astype(np.float64).sum())) < 1e-4 * np.abs(file_taps).sum()


def test_a_file_longer_than_the_capacity_is_cut_to_it(model, cabinet):
    """96 kHz at the default capacity: the first 8192 of the 16447 taps, not faded"""
    path, file_taps = cabinet
    p = _pool(model, 2, 256, 96000)
    taps = ax.load_ir_wav_for(p, path)
    assert taps.size == 8192 == p.ir_capacity()
    assert np.array_equal(taps, ax.resample_ir(file_taps, FILE_RATE, 96000)[0][:8192])
    p.set_ir(taps)
    x = modelgen.signal(2, 256, seed=2)
    got = p.process(x)
    p.close()
    _tau("rates96000cut", got, x, rs.resample(file_taps, FILE_RATE, 96000, 0, 8192))


def test_a_file_at_the_pools_rate_is_taken_as_it_is(model, cabinet):
    path, file_taps = cabinet
    p = _pool(model, 2, 256, FILE_RATE, 16384)
    assert np.array_equal(ax.load_ir_wav_for(p, path), np.concatenate([file_taps, np.zeros(32, np.float32)]))
    assert np.array_equal(ax.load_ir_wav_for(p, path, lead=5)[5:5 + FILE_FRAMES], file_taps)
    p.close()
