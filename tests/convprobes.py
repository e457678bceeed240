"""Conv activation probes: the smallest stacks on which ONE evaluation of a conv epilogue's tanh or sigmoid is the model's output, with an
fp64 closed form and a per-sample error bound — the conv stacks' counterpart of tests/probes.py (the recurrent cells).

The conv epilogues use tanh_exp_pre (on weights and biases the packer scaled by 2 log2 e) and fast_sigmoid (aidax_device.h); their call
sites are cs_activate (k_conv_ms, k_conv_st's mixed instantiation), the switch of k_conv_mfma, the switch of k_conv. The random models of
the parity tests keep every pre-activation of order 1.

    two layers   layer 0: one tap, channel c has (w_c, b_c) = (200, 0) for even c, (-128, 0.5) for odd c, under tanh or sigmoid;
                 layer 1: linear, two taps, the newest through identity weights — exact in every form: w0 x0, w0 x1 and w0 x2 are all
                 kept, and x0 + x1 + x2 adds up without rounding in any order;
                 Dense: one-hot on the observed channel, no bias. The smallest stack k_conv_ms admits.
    StGeoC       the same probe in the shape k_conv_st is compiled for (six layers, three taps, dilations 1 .. 32): layer 0's newest tap
                 carries (w_c, b_c), layers 1 .. 5 pass the newest tap through identity weights.

So the model's output is act(w_c x + b_c) of the observed channel c — 0, 5, 10 or 15: every element of a lane's four, every quarter of the
fragment. `probe_input` sweeps z = w_c x + b_c over +-{1e-6, 1e-3, 0.1, 1, 5, 9, 17, 20, 88, 110, 200} for both kinds of channel, and the
floats around 0 (0, -0, the smallest denormal and normal, 1e-30).

THE BOUND (`allowed`), per sample, at the true value y = act(z), z = w_c x + b_c in fp64 on the float32 x the network is handed. It has
two parts, and a floor.
  1. The function, its argument taken as exact. aidax_device.h at tanh_exp, from one ulp (2^-23 relative) each for v_exp_f32 and
     v_rcp_f32, half an ulp for the sum 1 + e and half an ulp for the last FMA:
         tanh     2^-23 (1.5 (1 - y) + (1 - y^2) / 2) + 2^-24 |y|
     fast_sigmoid(v) = rcp(1 + exp2(-v log2 e)) from the same budget: y = 1 / (1 + e), dy/de = -y^2 and y e = 1 - y, so a relative error
     eps of e moves y by y (1 - y) eps; e carries the ulp of v_exp_f32 and the rounding of its argument -v log2 e (the constant and the
     product, 2^-24 each, on an argument of |v| log2 e: 2^-23 |v| relative in e); the sum and the reciprocal move y by 2^-24 y and 2^-23 y:
         sigmoid  2^-23 (y (1 - y) (1 + |z|) + 1.5 y)
  2. The argument. Layer 0 is one FMA per tap: z' = fma(w', x, b'), one rounding, 2^-24 |z|. A tanh layer's w' and b' are the packer's
     fl(fl(2 log2 e) w) and fl(fl(2 log2 e) b): two roundings each, 2^-23 (|w x| + |b|). A sigmoid layer's are the model's own. So
         |dz| <= 2^-24 (|z| + 2 (|w x| + |b|))  (tanh),   2^-24 |z|  (sigmoid)
     and the activation passes it on times its steepest slope within dz of z: 1 - tanh^2(|z| - dz), resp. s (1 - s) at |z| - dz.
  Floor: 2^-126. A result below the smallest normal may come out as zero (the header's budget says nothing about denormals, and the
  identity layers pass the value through matrix instructions).
None of this is measured. Where float32's own tanh / logistic function return exactly 0, 1 or -1 (`pool_reference`'s `exact`, from the fp32 oracle) the
kernels must return those bits instead."""
import numpy as np

TARGETS = (1e-6, 1e-3, 0.1, 1.0, 5.0, 9.0, 17.0, 20.0, 88.0, 110.0, 200.0)
OBSERVED = (0, 5, 10, 15)
FRAMES = 1024
STREAMS = 6
SHAPES = ("two layers", "StGeoC")
_STGEOC = (1, 2, 4, 8, 16, 32)


def channel_params(c):
    return (200.0, 0.0) if c % 2 == 0 else (-128.0, 0.5)


def make_probe(act, observed, shape="two layers"):
    """the json dict of a probe stack; act: "tanh" | "sigmoid" """
    C = 16
    k = 1 if shape == "two layers" else 3
    w0 = np.zeros((k, 1, C), np.float32)
    b0 = np.zeros(C, np.float32)
    for c in range(C):
        w0[k - 1, 0, c], b0[c] = channel_params(c)
    layers = [{"type": "conv1d", "activation": act, "shape": [None, None, C], "kernel_size": [k], "dilation": [1],
               "weights": [w0.tolist(), b0.tolist()]}]
    for dil in ((1,) if shape == "two layers" else _STGEOC[1:]):
        kk = 2 if shape == "two layers" else 3
        w = np.zeros((kk, C, C), np.float32)
        w[kk - 1] = np.eye(C, dtype=np.float32)
        layers.append({"type": "conv1d", "activation": "", "shape": [None, None, C], "kernel_size": [kk], "dilation": [dil],
                       "weights": [w.tolist(), np.zeros(C, np.float32).tolist()]})
    d = np.zeros((C, 1), np.float32)
    d[observed, 0] = 1.0
    layers.append({"type": "dense", "activation": "", "shape": [None, None, 1], "weights": [d.tolist(), [0.0]]})
    return {"in_shape": [None, None, 1], "layers": layers, "in_skip": 0, "in_gain": 0.0, "out_gain": 0.0,
            "metadata": {"name": f"conv probe {shape} {act} ch{observed}", "samplerate": "48000"}}


def sweep():
    """the float32 inputs that put z on +-TARGETS for the even and for the odd channels, and the floats around 0"""
    z = np.concatenate([np.asarray(TARGETS), -np.asarray(TARGETS)])
    xs = []
    for c in (0, 1):
        w, b = channel_params(c)
        xs.append((z - b) / w)
    tiny = np.array([0.0, -0.0, 1.4e-45, -1.4e-45, 1.17549435e-38, -1.17549435e-38, 1e-30, -1e-30, 0.5 / 128.0])      # (the last: z = 0 on the odd channels)
    return np.concatenate(xs + [tiny]).astype(np.float32)


def probe_input(n_streams=STREAMS, frames=FRAMES):
    """[n_streams][frames] float32: the sweep over and over, started at another phase per stream (another frame tile, another lane)"""
    sw = sweep()
    x = np.zeros((n_streams, frames), np.float32)
    for s in range(n_streams):
        x[s] = np.resize(np.roll(sw, 7 * s), frames)
    return x


def _act64(act, z):
    with np.errstate(over="ignore"):
        return np.tanh(z) if act == "tanh" else 1.0 / (1.0 + np.exp(-z))


def closed_form(act, observed, xg):
    """(z, y) in fp64 for the float32 network input xg"""
    w, b = channel_params(observed)
    z = np.float64(np.float32(w)) * np.asarray(xg, np.float32).astype(np.float64) + np.float64(np.float32(b))
    return z, _act64(act, z)


def allowed(act, observed, xg):
    """the bound of the module's docstring on |kernel's act - y|, per sample"""
    w, b = channel_params(observed)
    z, y = closed_form(act, observed, xg)
    wx = np.abs(w * np.asarray(xg, np.float32).astype(np.float64))
    if act == "tanh":
        f = 2.0 ** -23 * (1.5 * (1.0 - y) + 0.5 * (1.0 - y * y)) + 2.0 ** -24 * np.abs(y)
        dz = 2.0 ** -24 * (np.abs(z) + 2.0 * (wx + abs(b)))
        slope = 1.0 - np.tanh(np.maximum(np.abs(z) - dz, 0.0)) ** 2
    else:
        f = 2.0 ** -23 * (y * (1.0 - y) * (1.0 + np.abs(z)) + 1.5 * y)
        dz = 2.0 ** -24 * np.abs(z)
        s = _act64(act, np.maximum(np.abs(z) - dz, 0.0))
        slope = s * (1.0 - s)
    return f + dz * slope + 2.0 ** -126


_REF = {}


def pool_reference(act, observed, shape):
    """What a pool of STREAMS streams must give for the probe over probe_input() under the exact tests' controls (in_lpf_pc=0, dc_blocker=0,
    eq_bypass=1), from the oracle: dict(j, x, want = the fp32 oracle's full run, exact = where the fp32 oracle's network returns exactly 0,
    1 or -1, ref = y in fp64 times the master gain, allowed = the bound on |pool output - ref|). Computed once, shared by every form's test,
    read-only."""
    from oracle import oracle as O
    from tests import convdata
    key = (act, observed, shape)
    if key not in _REF:
        j = make_probe(act, observed, shape)
        spec = O.parse_model(j)
        x = probe_input()
        xg = convdata.pre_chain(x)
        master = convdata.gain_ramps(x.shape[1])[1].astype(np.float64)
        want = O.run_streams(spec, O.default_controls(in_lpf_pc=0.0, dc_blocker=0.0, eq_bypass=1.0), x, 256)
        y32 = np.stack([O.OracleModel(spec).apply(xg[s]) for s in range(x.shape[0])])
        assert np.array_equal(want, y32 * master.astype(np.float32)[None, :])
        z, y = closed_form(act, observed, xg)
        # the pool multiplies the network's output by the master gain in fp32: one more rounding, 2^-24 |y m|
        # (and the product may be a denormal in its turn: the floor once more)
        bound = (allowed(act, observed, xg) + 2.0 ** -24 * np.abs(y)) * master[None, :] + 2.0 ** -126
        r = dict(j=j, x=x, xg=xg, want=want, exact=(y32 == 0.0) | (np.abs(y32) == 1.0), y32=y32, z=z, ref=y * master[None, :], allowed=bound)
        for a in r.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _REF[key] = r
    return _REF[key]
