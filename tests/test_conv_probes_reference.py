"""The conv activation probes (tests/convprobes.py) as a REFERENCE, established on the CPU before any kernel is judged by them
(tests/test_gpu_conv_activations.py): for both activations, every observed channel and both shapes

  * the closed form is the fp64 oracle after rounding to float32, and the model's output is the observed channel's activation alone;
  * the sweep puts z on every magnitude of TARGETS with both signs, on the even and on the odd channels, and on the floats around 0;
  * the bound is no tighter than float32 allows: the plain fp32 oracle (libm's tanhf and expf, a multiply and an add for z) stays within
    it, and so does a numpy emulation of the header's own sequences — tanh_exp_pre on weights scaled by 2 log2 e, fast_sigmoid — with
    a correctly rounded exp2 and reciprocal;
  * the magnitudes at which the fp32 reference returns exactly 0, 1 or -1 — where the kernels must return those bits — are there on
    both sides: tanh from |z| = 17 on and at z = 0, the sigmoid from z = 17 on and from z = -110 down."""
import numpy as np
import pytest

from oracle import oracle as O
from tests import convdata, convprobes as cp

CASES = [(act, c, shape) for act in ("tanh", "sigmoid") for c in cp.OBSERVED for shape in cp.SHAPES]


@pytest.mark.parametrize("act,c,shape", CASES)
def test_closed_form_is_the_fp64_oracle_and_the_fp32_oracle_is_within_the_bound(act, c, shape):
    j = cp.make_probe(act, c, shape)
    spec = O.parse_model(j)
    xg = convdata.pre_chain(cp.probe_input(2, 256))
    for s in range(2):
        z, y = cp.closed_form(act, c, xg[s])
        assert np.all(np.isfinite(y))
        assert np.array_equal(O.net_run(spec, xg[s], f64=True), y.astype(np.float32))
        y32 = O.net_run(spec, xg[s])
        assert np.all(np.abs(y32 - y) <= cp.allowed(act, c, xg[s])), np.max(np.abs(y32 - y) / cp.allowed(act, c, xg[s]))


@pytest.mark.parametrize("c", cp.OBSERVED)
def test_the_sweep_reaches_every_target_on_every_observed_channel(c):
    z = cp.closed_form("tanh", c, convdata.pre_chain(cp.probe_input(1, 256))[0])[0]
    for t in cp.TARGETS:
        for sign in (1.0, -1.0):
            # (an odd channel reaches a small z through a cancellation, -128 x + 0.5: to the resolution of the float32 x — 128 times half
            # an ulp of x ~ 2^-8, 2^-25 — and of the pre gain)
            assert np.min(np.abs(z - sign * t)) <= max(1e-3 * t, 2.0 ** -24), (c, sign * t)
    assert np.any(z == 0.0) and z.max() >= 199.0 and z.min() <= -199.0
    if c % 2 == 0:
        assert np.any((z > 0) & (z < 1e-35)) and np.any((z < 0) & (z > -1e-35))          # the floats around 0


def _f32(a):
    return np.asarray(a, np.float64).astype(np.float32).astype(np.float64)


def emulate(act, c, xg):
    """the header's sequences in float32 steps (every step computed in fp64 and rounded once: FMA, correctly rounded exp2 and rcp)"""
    w, b = cp.channel_params(c)
    x = np.asarray(xg, np.float32).astype(np.float64)
    with np.errstate(over="ignore", divide="ignore"):
        if act == "tanh":
            k = _f32(2.0 * np.log2(np.e))
            z = _f32(_f32(k * w) * x + _f32(k * b))
            r = _f32(1.0 / _f32(1.0 + _f32(np.exp2(z))))
            return _f32(-2.0 * r + 1.0)
        z = _f32(w * x + b)
        e = _f32(np.exp2(_f32(z * _f32(-np.log2(np.e)))))
        return _f32(1.0 / _f32(1.0 + e))


@pytest.mark.parametrize("act", ["tanh", "sigmoid"])
@pytest.mark.parametrize("c", cp.OBSERVED)
def test_the_headers_own_sequences_are_within_the_bound(act, c):
    xg = convdata.pre_chain(cp.probe_input(1, 256))[0]
    z, y = cp.closed_form(act, c, xg)
    got = emulate(act, c, xg)
    ratio = np.abs(got - y) / cp.allowed(act, c, xg)
    assert ratio.max() <= 1.0, (ratio.max(), z[np.argmax(ratio)])
    # ... and they return the exact bits where float32's own functions do
    y32 = O.net_run(O.parse_model(cp.make_probe(act, c)), xg)
    exact = (y32 == 0.0) | (np.abs(y32) == 1.0)
    assert np.array_equal(got[exact], y32[exact].astype(np.float64))


@pytest.mark.parametrize("c", cp.OBSERVED)
def test_the_exact_magnitudes(c):
    for act in ("tanh", "sigmoid"):
        r = cp.pool_reference(act, c, "two layers")
        z, y32, exact = r["z"], r["y32"], r["exact"]
        assert np.all(exact[np.abs(z) >= 110.0]) and not np.any(exact[(np.abs(z) < 9.5) & (z != 0.0)])
        if act == "tanh":
            assert np.all(y32[z >= 16.9] == 1.0) and np.all(y32[z <= -16.9] == -1.0) and np.all(y32[z == 0.0] == 0.0)
        else:
            assert np.all(y32[z >= 16.9] == 1.0) and np.all(y32[z <= -109.0] == 0.0) and np.all(y32[(z < -80.0) & (z > -89.0)] > 0.0)
        assert 0.2 < np.mean(exact) < 0.8
        assert np.all(r["allowed"] > 0) and np.all(np.isfinite(r["allowed"]))
