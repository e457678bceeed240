"""Conv stacks on which the conv1d kernels (k_conv_st, k_conv_ms, k_conv_mfma, k_conv) must be exact to the last bit, their inputs, and
their exact outputs computed in numpy, independently of the C oracle.

k_conv_ms and k_conv_st split a layer's weights and its input activations into three bf16 terms each (w = w0 + w1 + w2, x = x0 + x1 + x2) and
accumulate six of the nine term products in fp32: (w0 w1 w2) x0, (w0 w1) x1, w0 x2 — a three-tap layer's oldest tap through a packed first
k-step with hand-laid fragments (ConvLayer::ms_packed0). The random stacks of tests/test_gpu_parity.py are held to 3e-6 of full scale,
and a lost low-order product moves one of 32 - 64 summands by 2^-16 of itself: far below that bar. On the stacks built here every value
of every layer is a multiple of a power of two that fits fp32's 24 bits together with every partial sum that leads to it, so the correct
output is the true one bit for bit whatever the order of the additions, and a missing, doubled or misplaced term product changes bits
(tests/test_conv_arith.py checks both claims in numpy).

LAYER 0 IS A QUANTISER. The net's input is what the pre chain makes of the audio (x * pregain ramp: bit-identical to the oracle's, but
not on a grid). Layer 0 is fp32 FMAs in every kernel form; here it has weights W u_k (W = 1024, u_k a signed power of three per tap:
1, 3, 9, 27 ...) and thresholds 256 (m_c + 1/2) under tanh or sigmoid, and `signal` delivers 0.25 sigma, sigma in {-1, 0, +1} (noise
with stretches of silence). Then z / 256 = sum_k u_k sigma_k + m_c + 1/2 — an integer plus one half — and every pre-activation has
|z| >= 128 = MARGIN_NOMINAL, whatever the taps see (silence, the warm-up's zeros, block edges). tests/test_conv_arith.py holds the
oracle's own pre-chain output to MARGIN = 127 (the pre gain is 1 to an ulp). tanh(+-127) is +-1 and sigmoid(+-127) is 1 / 0 to the bit in
the oracle (expf overflows at 88.7) and must be in the kernels: e -> inf gives rcp -> 0, e -> 0 gives 1 — so layer 0 is a saturation probe
of every form too, and every channel leaves it as a one-term code, +-1 or 0 / 1.

MIXED-ACTIVATION FAMILIES (linear and relu layers behind layer 0: k_conv_st<.., false>, k_conv_ms, k_conv_mfma, k_conv). Unit in_gain,
out_gain, in_skip 0. The sixteen channels of every layer >= 1 play roles, dealt anew to the channel numbers per layer:

    S  the rest      codes passed on: one tap, one S channel below, weight +-1 (+-2 and bias -+1 behind a relu or the sigmoid quantiser):
                     always in [-1, 1]
    P  min(4, taps)  `producers` (eight channels: one, with every tap): channel i of them has tap i (and i + 4, ...: between them every tap
                     of the layer), each tap reading one S channel below, no bias: +-w or 0, with w's own terms
    Q  two           `consumers`: every tap of the layer split between them, tap t reading P channel t mod n_P below (every P is read);
                     a bias of odd / 256
    C  one           the accumulator: C + Q_0 + Q_1 of the layer below through weights +1 — what carries a layer's Q to the Dense layer
    q, c  two, one   the negative parts of Q and C in a relu layer (the same row negated: x = relu(x) - relu(-x), and the layer above
                     reads both, the second through weights of the other sign, so nothing a relu clamps is lost); zero rows in a linear layer
    Z  two (C = 16)  all-zero rows (the output is the bias, 0)

    family   layer 0   P's weights                      Q's weights                   term products exercised at every tap of a layer >= 2
    T3       tanh      odd 18-bit integers 2^-16,       +-1                           P: w0 x0, w1 x0, w2 x0;  Q: w0 x0, w0 x1, w0 x2
                       all three terms non-zero
    T2       sigmoid   odd 9-bit integers 2^-8          odd 9-bit integers 2^-8       P: w0 x0, w1 x0;  Q: w0 x0, w1 x0, w0 x1, w1 x1

Layer 1 reads the quantiser's one-term codes in every role, so only (w0 w1 w2) x0 can be non-zero there; from layer 2 on the Q channels
read the multi-term P values of the layer below. The three dropped products (w1 x2, w2 x1, w2 x2) are zero at every (weight, input)
pair: a three-term weight only ever meets a code, a one-term weight meets anything, two-term weights meet two-term values. Worst case
(`budget`): the sum of the magnitudes of bias and all kept term products of any output, over the finest power of two any of them is a
multiple of, stays below 2^24 — in every layer and in the Dense layer, whose row is +-1.

ALL-TANH FAMILY `SIGN` (k_conv_st<.., true>, the instantiation BASELINE cfg4 itself runs): every layer saturates. Weights 64 * (+-1 | +-2)
on a few (tap, channel) pairs of every output, at least one per tap, and a bias 32 * (+-1 | +-3): z / 32 is an odd integer whatever
the inputs in {-1, 0, 1} are, |z| >= 32, every output exactly +-1, and the Dense layer (odd integers / 16) is exact. This is a ROUTING
test: a misplaced tap, channel, frame, ring slot or tile flips signs (the sums are small: +-1 .. +-11). It is NOT a low-order-term test —
the packer scales a tanh layer's weights by 2 log2 e, so its sums are inexact in every term — the term coverage comes from the mixed
families, which run the same MFMA code.

`truth` evaluates a model in fp64 on its float32 weights from the codes on, asserts every layer and the output exact in float32, and
returns what the bare network must give; the expected POOL output is the oracle's full run (the master gain fades in), and
tests/test_conv_arith.py shows the oracle's network equal to `truth` bit for bit on every family."""
import zlib

import numpy as np

from tests.test_split_arith import bf16_rne, split3          # noqa: F401  (re-exported: the split the kernels and the packer use)

# the six term products as (term of w, term of x), in the order the kernels issue them, and the three they drop
KEPT = ((0, 0), (1, 0), (2, 0), (0, 1), (1, 1), (0, 2))
DROPPED = ((1, 2), (2, 1), (2, 2))
# what each mixed family exercises at every tap of a layer >= 2, and of layer 1 (tests/test_conv_arith.py holds the families to these claims)
EXERCISES = {"T3": ((0, 0), (1, 0), (2, 0), (0, 1), (0, 2)),
             "T2": ((0, 0), (1, 0), (0, 1), (1, 1))}
EXERCISES_L1 = {"T3": ((0, 0), (1, 0), (2, 0)),
                "T2": ((0, 0), (1, 0))}
MIXED = ("T3", "T2")
FAMILIES = MIXED + ("SIGN",)

W0, LEVEL = 1024.0, 0.25
MARGIN_NOMINAL, MARGIN = 128.0, 127.0
WARMUP = 2048                      # frames of silence a model sees before its first block (rt-neural-generic.cpp:1077-1078)

_A = [(3, 1)] + [(3, d) for d in (2, 4, 8, 16, 32, 64, 128)]
# name: (channels, [(taps, dilation) per layer, layer 0 first]); the first five are the geometries k_conv_st is compiled for (aidax_layout.h)
STACKS = {
    "StGeoA": (16, _A),
    "StGeoB": (16, [(2, d) for d in (1, 2, 4, 8, 16, 1, 2, 4, 8, 16)]),
    "StGeoC": (16, [(3, d) for d in (1, 2, 4, 8, 16, 32)]),
    "StGeoD": (16, [(3, d) for d in (1, 2, 4, 8, 1, 2, 4, 8)]),
    "StGeoE": (16, [(2, d) for d in (1, 2, 4, 8, 16, 32, 64, 128)]),
    "three taps, deep oldest tap": (16, [(3, 2), (3, 5), (3, 100)]),                              # 200 frames back: beyond the plane, through the packed k-step
    "four taps, two deep taps in one k-step": (16, [(4, 5), (4, 1), (4, 85), (4, 7)]),           # shifts 255 / 170 share k-step 0: per-lane sources
    "two taps, one deep": (16, [(2, 3), (2, 1), (2, 200)]),
    "twelve channels": (12, [(3, 1), (3, 2), (3, 4)]),                                            # zero-padded on k_conv_mfma
    "eight channels, five taps": (8, [(5, 1), (5, 2), (5, 3)]),                                   # zero-padded on k_conv_mfma
}
# (the corners' deep layer — a history beyond the 128 frames k_conv_ms's plane holds, its oldest taps read from HBM — is layer 2 or 3, never
# layer 1: layer 1 reads the quantiser's one-term codes, and the x1 and x2 terms of the deep taps would never be non-zero)
ST_STACKS = ("StGeoA", "StGeoB", "StGeoC", "StGeoD", "StGeoE")
MS_STACKS = ("three taps, deep oldest tap", "four taps, two deep taps in one k-step", "two taps, one deep")
MFMA_STACKS = ("twelve channels", "eight channels, five taps")


def receptive_field(j):
    """frames of input history the model's output depends on"""
    return sum((int(l["kernel_size"][0]) - 1) * int(l["dilation"][0]) for l in j["layers"][:-1])


def _roles(C, k):
    n_p = min(4 if C >= 12 else 1, k)
    n_z = 2 if C == 16 else 0
    return ["S"] * (C - n_p - 6 - n_z) + ["P"] * n_p + ["Q", "Q", "q", "q", "C", "c"] + ["Z"] * n_z


def _terms_nonzero(v):
    return [bool(np.all(t != 0)) for t in split3(np.asarray([v], np.float32))]


def _weight(rs, family, role):
    sign = -1.0 if rs.rand() < 0.5 else 1.0
    if family == "T3" and role == "P":
        while True:
            w = sign * (2 * int(rs.randint(1 << 16, 1 << 17)) + 1) * 2.0 ** -16
            if all(_terms_nonzero(w)):
                return w
    if family == "T3":
        return sign
    return sign * (2 * int(rs.randint(128, 256)) + 1) * 2.0 ** -8          # 257 .. 511, odd: two terms, never three


def _layer(k, dil, act, w, b):
    return {"type": "conv1d", "activation": act, "shape": [None, None, int(w.shape[2])], "kernel_size": [int(k)], "dilation": [int(dil)],
            "weights": [w.astype(np.float32).tolist(), b.astype(np.float32).tolist()]}


def _quantiser(rs, C, k, dil, act):
    w = np.zeros((k, 1, C))
    b = np.zeros(C)
    for c in range(C):
        u = 3.0 ** rs.permutation(k) * np.where(rs.rand(k) < 0.5, -1.0, 1.0)
        w[:, 0, c] = W0 * u
        b[c] = W0 * LEVEL * (int(rs.randint(-3, 3)) + 0.5)
    return _layer(k, dil, act, w, b)


def _grid_layer0(rs, C, k, dil):
    """the bare-model runs' layer 0: linear, one tap per channel with weight +-1 — inputs in {-1, 0, 1} leave as one-term codes"""
    w = np.zeros((k, 1, C))
    for c in range(C):
        w[int(rs.randint(k)), 0, c] = -1.0 if rs.rand() < 0.5 else 1.0
    return _layer(k, dil, "", w, np.zeros(C))


_MADE = {}


def make_stack(stack, family, quantiser=True):
    """-> (json dict of the model, meta). meta["roles"][l][c]: the role of channel c of layer l (layer 0: all "S"). quantiser=False: layer
    0 linear on grid inputs (the bare-model runs). A mixed stack is drawn again (meta["salt"]) until it exercises what its family claims
    on a probe signal — a producer's few distinct values may all happen to have a zero third term, say. Cached: treat as read-only."""
    key = (stack, family, quantiser)
    salt = 0
    while key not in _MADE:
        j, meta = _make_stack(stack, family, quantiser, salt)
        if family != "SIGN":
            x = LEVEL * grid_signal(1200, seed=99) if quantiser else grid_signal(1200, seed=99)
            acts = truth(j, x, warm=quantiser)[1]
            if not claims_hold(j, family, acts):
                salt += 1
                assert salt < 64
                continue
        _MADE[key] = (j, meta)
    return _MADE[key]


def _make_stack(stack, family, quantiser, salt):
    C, geo = STACKS[stack]
    rs = np.random.RandomState(zlib.crc32(f"{stack}/{family}/{quantiser}/{salt}".encode()) & 0x7FFFFFFF)
    act0 = "sigmoid" if family == "T2" else "tanh"
    layers = [_quantiser(rs, C, geo[0][0], geo[0][1], act0) if quantiser else _grid_layer0(rs, C, geo[0][0], geo[0][1])]
    roles = [["S"] * C]
    acts = [act0 if quantiser else ""]
    for l in range(1, len(geo)):
        k, dil = geo[l]
        w = np.zeros((k, C, C))
        b = np.zeros(C)
        if family == "SIGN":
            act = "tanh"
            role = ["T"] * C
            for co in range(C):
                for tap in range(k):
                    for ci in rs.choice(C, size=int(rs.randint(1, 3)), replace=False):
                        w[tap, ci, co] = 64.0 * rs.choice([-1.0, 1.0, -2.0, 2.0])
                b[co] = 32.0 * rs.choice([-1.0, 1.0, -3.0, 3.0])
        else:
            act = "relu" if l % 2 else ""
            role = [str(r) for r in rs.permutation(_roles(C, k))]
            below = {r: [c for c in range(C) if roles[-1][c] == r] for r in "SPQqCc"}
            unit_range = acts[-1] in ("relu", "sigmoid")              # the S channels below are in [0, 1], not [-1, 1]
            mine = {r: [c for c in range(C) if role[c] == r] for r in "SPQqCc"}
            for co in mine["S"]:
                s = -1.0 if rs.rand() < 0.5 else 1.0
                w[int(rs.randint(k)), int(rs.choice(below["S"])), co] = 2.0 * s if unit_range else s
                b[co] = -s if unit_range else 0.0
            for i, co in enumerate(mine["P"]):
                for tap in range(i, k, len(mine["P"])):               # (no bias: a one-tap P is +-w or 0, w's own three or two terms)
                    w[tap, int(rs.choice(below["S"])), co] = _weight(rs, family, "P")
                if unit_range and act == "relu":                      # (codes in [0, 1] under a relu: a negative weight would leave the channel dead)
                    w[:, :, co] = np.abs(w[:, :, co])
            src = [int(c) for c in rs.permutation(below["P"])] if below["P"] else [int(c) for c in rs.choice(below["S"], size=k)]
            for i, co in enumerate(mine["Q"]):
                for tap in range(i, k, 2):                            # tap t reads producer t mod n_p: every producer below is read
                    w[tap, src[tap % len(src)], co] = _weight(rs, family, "Q")
                b[co] = (2 * int(rs.randint(-8, 8)) + 1) * 2.0 ** -8
            # the accumulator: (C - c) + sum (Q_i - q_i) of the layer below (layer 1: one code)
            co = mine["C"][0]
            if below["C"]:
                w[k - 1, below["C"][0], co], w[k - 1, below["c"][0], co] = 1.0, -1.0
                for qp, qn in zip(below["Q"], below["q"]):
                    tap = int(rs.randint(k))
                    w[tap, qp, co], w[tap, qn, co] = 1.0, -1.0
            else:
                w[k - 1, int(rs.choice(below["S"])), co] = 1.0
            # the negative parts: behind a relu x = relu(x) - relu(-x), so nothing a relu clamps is lost to the layers above; a linear layer
            # leaves them zero
            if act == "relu":
                for pos, neg in zip(mine["Q"] + mine["C"], mine["q"] + mine["c"]):
                    w[:, :, neg], b[neg] = -w[:, :, pos], -b[pos]
        layers.append(_layer(k, dil, act, w, b))
        roles.append(role)
        acts.append(act)
    if family == "SIGN":
        d = (2.0 * rs.randint(-8, 8, size=C) + 1.0) / 16.0
        bd = 0.25
    else:
        d = np.where(rs.rand(C) < 0.5, -1.0, 1.0)
        d[[c for c in range(C) if roles[-1][c] in "qc"]] = -1.0          # positive parts +1, negative parts -1: the Dense layer sees C and Q whole
        d[[c for c in range(C) if roles[-1][c] in "QC"]] = 1.0
        bd = -3.0
    layers.append({"type": "dense", "activation": "", "shape": [None, None, 1], "weights": [d[:, None].astype(np.float32).tolist(), [bd]]})
    j = {"in_shape": [None, None, 1], "layers": layers, "in_skip": 0, "in_gain": 0.0, "out_gain": 0.0,
         "metadata": {"name": f"exact {stack} {family}", "samplerate": "48000"}}
    assert receptive_field(j) < WARMUP
    return j, dict(roles=roles, acts=acts, family=family, stack=stack, channels=C, salt=salt)


def signal(S, T, seed, silence=True):
    """[S][T] float32: LEVEL * sigma, sigma = +-1 noise with, per stream, stretches of silence (sigma = 0) of 1 .. 300 frames"""
    x = np.zeros((S, T), np.float32)
    for s in range(S):
        rs = np.random.RandomState((seed * 1000003 + s) & 0x7FFFFFFF)
        v = np.where(rs.rand(T) < 0.5, -1.0, 1.0)
        if silence:
            for n in (1, 7, 40, 300):
                p = int(rs.randint(0, max(T - n, 1)))
                v[p:p + n] = 0.0
        x[s] = LEVEL * v
    return x


def grid_signal(T, seed):
    """[T] float32 in {-1, 0, 1}: the bare-model runs' input"""
    return (signal(1, T, seed)[0] / LEVEL).astype(np.float32)


def layer_params(layer):
    w, b = (np.asarray(a, np.float32).astype(np.float64) for a in layer["weights"])
    return w, b, int(layer["kernel_size"][0]), int(layer["dilation"][0]), layer["activation"]


def contract(x, w):
    """sum_i x[s][i][t] w[i][o] -> [s][o][t]"""
    return np.matmul(np.ascontiguousarray(w.T), x)


def shifted(a, n):
    """a[..., t - n], zeros before the start"""
    if n == 0:
        return a
    out = np.zeros_like(a)
    out[..., n:] = a[..., :-n] if n < a.shape[-1] else 0.0
    return out


def preactivation(layer, a):
    """z[s][co][t] = b[co] + sum_tap sum_ci w[tap][ci][co] a[s][ci][t - (k - 1 - tap) dil] in fp64 (exact on these stacks)"""
    w, b, k, dil, _ = layer_params(layer)
    z = np.zeros((a.shape[0], w.shape[2], a.shape[2])) + b[None, :, None]
    for tap in range(k):
        z += contract(shifted(a, (k - 1 - tap) * dil), w[tap])
    return z


def activate(z, act, saturating_margin=None):
    if act == "tanh":
        assert np.abs(z).min() >= (saturating_margin or 20.0), np.abs(z).min()
        return np.sign(z)
    if act == "sigmoid":
        assert np.abs(z).min() >= (saturating_margin or 100.0), np.abs(z).min()
        return (z > 0).astype(np.float64)
    return np.maximum(z, 0.0) if act == "relu" else z


def _exact32(a, what):
    assert np.array_equal(a.astype(np.float32).astype(np.float64), a), f"{what}: not exact in float32"


def forward_from(j, a, first, check=True, shift=None):
    """layers first .. and the Dense layer on the activations a[s][c][t] of layer first - 1, in fp64 -> (y[s][t], [activations per layer]).
    check=False: no assertion that the values are exact in float32 (for deliberately wrong inputs). shift = (layer, tap, frames): that
    tap reads `frames` further back than it should (a deliberately wrong model)."""
    acts = []
    for l in range(first, len(j["layers"]) - 1):
        layer = j["layers"][l]
        z = preactivation(layer, a)
        if shift is not None and shift[0] == l:
            w, _, k, dil, _ = layer_params(layer)
            back = (k - 1 - shift[1]) * dil
            z += contract(shifted(a, back + shift[2]) - shifted(a, back), w[shift[1]])
        a = activate(z, layer["activation"], MARGIN if l == 0 else None)
        if check:
            _exact32(a, f"layer {l}")
        acts.append(a)
    d, bd = (np.asarray(v, np.float32).astype(np.float64) for v in j["layers"][-1]["weights"])
    y = np.einsum("sct,c->st", a, d[:, 0]) + bd[0]
    if check:
        _exact32(y, "output")
    return y, acts


def truth(j, xg, warm=True):
    """The bare network on xg[s][t] (what the pre chain hands it), exactly. warm: after the warm-up's silence (any number of zeros beyond
    the receptive field gives the same state); else from reset state, every history zero. -> (y[s][t] float32, activations per layer [s][c][t])"""
    xg = np.atleast_2d(np.asarray(xg, np.float32)).astype(np.float64)
    pad = receptive_field(j) if warm else 0
    a = np.concatenate([np.zeros((xg.shape[0], pad)), xg], axis=1)[:, None, :]
    y, acts = forward_from(j, a, 0)
    return y[:, pad:].astype(np.float32), [v[:, :, pad:] for v in acts]


def lsb_exponent(a):
    """the largest e such that every element of a is a multiple of 2^e (a: fp64, not all zero)"""
    a = np.abs(np.asarray(a, np.float64).ravel())
    a = a[a != 0]
    m, e = np.frexp(a)
    q = (m * 2.0 ** 53).astype(np.int64)
    tz = np.zeros(q.shape, np.int64)
    for sh in (32, 16, 8, 4, 2, 1):
        low = (q & ((1 << sh) - 1)) == 0
        tz += np.where(low, sh, 0)
        q = np.where(low, q >> sh, q)
    return int((e - 53 + tz).min())


def _channel_lsb(x):
    """per channel c of x[s][c][t]: lsb_exponent(x[:, c, :]), None for an all-zero channel (one pass: the values are multiples of 2^-40 below 2^22)"""
    q = np.abs(x) * 2.0 ** 40
    qi = q.astype(np.int64)
    assert np.array_equal(qi.astype(np.float64), q) and q.max(initial=0.0) < 2.0 ** 62
    low = np.where(qi == 0, np.int64(1) << 62, qi & -qi).min(axis=(0, 2))
    return [None if v == (1 << 62) else int(v).bit_length() - 1 - 40 for v in low]


def budget(j, acts):
    """per layer >= 1 and for the Dense layer: the largest, over the output channels, of log2 of (the largest sum of |bias| and |kept term
    products| the channel forms over the run whose activations are `acts`) / (the finest power of two all of those summands are multiples
    of). Below 24: every partial sum, in any order and grouping, is exact in fp32."""
    out = []
    n = len(j["layers"]) - 1
    for l in range(1, n + 1):
        a = acts[l - 1]
        if l < n:
            w, b, k, dil, _ = layer_params(j["layers"][l])
            pairs = KEPT
            ws, xs = [t.astype(np.float64) for t in split3(w.astype(np.float32))], [t.astype(np.float64) for t in split3(a.astype(np.float32))]
        else:
            d, bd = (np.asarray(v, np.float32).astype(np.float64) for v in j["layers"][-1]["weights"])
            w, b, k, dil, pairs, ws, xs = d[None, :, :], bd, 1, 1, ((0, 0),), [d[None, :, :]], [a]
        co_n = w.shape[2]
        mag = np.zeros((a.shape[0], co_n, a.shape[2])) + np.abs(b)[None, :, None]
        unit = np.array([lsb_exponent(b[c]) if b[c] != 0 else 99 for c in range(co_n)])
        xlsb = [_channel_lsb(xt) for xt in xs]
        # (per tap ONE contraction: the three terms of x stacked along the channels, against the sums of |w_i| each of them meets)
        xabs = np.abs(np.concatenate(xs, axis=1))
        for tap in range(k):
            wsum = [sum(np.abs(ws[wi][tap]) for wi, xj in pairs if xj == xi) + np.zeros_like(ws[0][tap]) for xi in range(len(xs))]
            mag += shifted(contract(xabs, np.concatenate(wsum, axis=0)), (k - 1 - tap) * dil)
            for wi, xi in pairs:
                for ci, co in zip(*np.nonzero(ws[wi][tap])):
                    if xlsb[xi][ci] is not None:
                        unit[co] = min(unit[co], lsb_exponent(ws[wi][tap, ci, co]) + xlsb[xi][ci])
        top = mag.max(axis=(0, 2))
        out.append(max(float(np.log2(top[c])) - unit[c] for c in range(co_n) if top[c] > 0))
    return out


def active_taps(w_term, x_term, k, dil):
    """[tap]: does the product of these two terms have a non-zero summand at that tap, anywhere in the run"""
    T = x_term.shape[2]
    out = []
    for tap in range(k):
        back = (k - 1 - tap) * dil
        x_live = np.any(x_term[:, :, :max(T - back, 0)] != 0, axis=(0, 2))      # per input channel: non-zero where this tap reads it
        out.append(bool(np.any(x_live[:, None] & (w_term[tap] != 0))))
    return out


def term_activity(j, acts, l):
    """{(term of w, term of x): [tap] active?} for all nine products of layer l >= 1 over the run whose activations are `acts`"""
    w, b, k, dil, _ = layer_params(j["layers"][l])
    ws = [t.astype(np.float64) for t in split3(w.astype(np.float32))]
    xs = [t.astype(np.float64) for t in split3(acts[l - 1].astype(np.float32))]
    return {(wi, xi): active_taps(ws[wi], xs[xi], k, dil) for wi in range(3) for xi in range(3)}


def claims_hold(j, family, acts):
    """the dropped products zero and the family's claimed ones non-zero at every tap of every layer >= 1"""
    for l in range(1, len(j["layers"]) - 1):
        live = term_activity(j, acts, l)
        if any(any(live[p]) for p in DROPPED):
            return False
        if not all(all(live[p]) for p in (EXERCISES_L1 if l == 1 else EXERCISES)[family]):
            return False
    return True


def gain_ramps(n):
    """(pre gain[n], master gain[n]) float32: the oracle's two smoothers over the first n frames of a stream under default gains
    (orc_plugin_init, orc_plugin_run: the pre gain starts at its target 1, the master gain fades in from 0)"""
    import ctypes
    from oracle import oracle as O
    L = O.lib()
    out = []
    for start in (1.0, 0.0):
        s = O.ExpSm()
        L.orc_expsm_init(ctypes.byref(s))
        L.orc_expsm_set_sample_rate(ctypes.byref(s), 48000.0)
        L.orc_expsm_set_time_constant(ctypes.byref(s), 0.1)
        L.orc_expsm_set_target(ctypes.byref(s), start)
        L.orc_expsm_clear_to_target(ctypes.byref(s))
        L.orc_expsm_set_target(ctypes.byref(s), O.db_co(0.0))
        out.append(np.array([L.orc_expsm_next(ctypes.byref(s)) for _ in range(n)], np.float32))
    return out


def pre_chain(x):
    """what the oracle's plugin hands the network for the audio x[s][t] under the exact tests' controls (in_lpf_pc=0: the input is copied,
    then x * pre gain)"""
    x = np.atleast_2d(np.asarray(x, np.float32))
    return (x * gain_ramps(x.shape[1])[0][None, :]).astype(np.float32)
