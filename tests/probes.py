"""Diagonal probe models: recurrent layers with U = 0 and a Dense readout, so that every unit evolves on its own and its
gates are functions of the input sample alone —

    LSTM   c_t = f c_{t-1} + i g,  h_t = o tanh(c_t)           i, f, o = sigmoid(w x + b), g = tanh(w x + b)
    GRU    h_t = (1 - z) n + z h_{t-1}                         z, r = sigmoid(w x + b0 + b1), n = tanh(w x + b0 + r b1)

— and the fp64 reference is the few lines of numpy in `closed_form`, independent of the C oracle. Each unit gets its own (w, b)
per gate, so the units of ONE model sweep different parts of an activation's domain while each of them sits in another lane,
tile and wave of every kernel form (widths that are no multiple of 16 run zero-padded). Stacked probes keep U = 0 in every
layer and give the upper layers a diagonal W: unit j reads unit j below, the closed form stays per unit.

Families (tests/test_probes_reference.py establishes each as a reference, tests/test_gpu_activations.py runs them):
  tanh     the candidate alone: i = o = 1 (bias +40), f = 0 (bias -40), g = tanh(w_j (x + k_j / 2)), |w_j| log-spaced 1e-3 .. 8 with
           alternating sign, k_j in {-1, 0, 1}. GRU: z = 0, h = n.
  sigmoid  i and o (GRU: z and r) with |w_j| log-spaced 0.1 .. 200, alternating sign: pre-activations reach +-200, past the point
           where exp overflows fp32 (|z| > 88); f and g (GRU: n) moderate. (GRU: z on the overflowing side and at exactly 1 only —
           see _units.)
  clamp    LSTM only: f = i = 1, g = tanh(+-(24 .. 40) x) on a +-0.5 square wave: c integrates +-1 per sample — steps that fp32
           represents exactly — up to about +-40 and back, across the clamp of the kernels' tanh (7.9), several times.
  reset    GRU only: n = tanh(w x + b0 + r b1) with |b1| up to 3 and r sweeping as in `sigmoid`.
"""
import numpy as np

FAMILIES = {"lstm": ("tanh", "sigmoid", "clamp"), "gru": ("tanh", "sigmoid", "reset")}
BLOCKS = (256, 256, 37, 1)                      # what every probe run is cut into
N = sum(BLOCKS)
ONE, ZERO = 40.0, -40.0                         # gate biases: sigmoid(+-40) is 1 / 0 to fp64 rounding
_f32 = np.float32


def _logspace(lo, hi, H, shift=0):
    """|w_j| log-spaced over the units (rotated by `shift`: another layer, another unit), alternating sign"""
    j = (np.arange(H) + shift) % H
    mag = lo * (hi / lo) ** (j / max(H - 1, 1))
    return mag * np.where(j % 2, -1.0, 1.0)


def _units(kind, family, H, shift, upper=False):
    """per gate: (w[H], b[H]) in fp64; GRU also the recurrent bias b1[3][H]. `upper`: a layer that reads the h of the layer below,
    which carries that layer's error: its weights stay at 1 or below so that the error is not amplified (a weight of 200 would turn
    the 1e-7 a unit below is allowed into 2e-5 of pre-activation), and its gates reach overflow through their BIASES instead —
    the sweep is over the units then, not over time."""
    j = (np.arange(H) + shift) % H
    zero = np.zeros(H)
    const = lambda v: (zero, np.full(H, v))
    if upper:
        wu, sweep = np.sin(1.0 + j), _logspace(0.1, 200.0, H, shift)
        cand = (wu, 0.3 * np.cos(3.0 * j))
        if family == "tanh":
            cand = (_logspace(1e-3, 1.0, H, shift), zero)
            return dict(i=const(ONE), f=const(ZERO), g=cand, o=const(ONE)) if kind == "lstm" else dict(z=const(ZERO), r=const(0.0), n=cand, b1=np.zeros((3, H)))
        if family == "clamp":                  # (an integrator here would integrate what layer 0 leaves of its own rounding at every zero crossing)
            return dict(i=const(ONE), f=const(ZERO), g=(wu, zero), o=(zero, 1.0 + 0.1 * (j % 7)))
        if kind == "lstm":
            return dict(i=(0.5 * wu, sweep), o=(0.5 * np.cos(j), sweep[::-1]), f=(0.5 * np.cos(j), 0.5 * np.sin(2.0 * j) - 1.0), g=cand)
        if family == "sigmoid":
            return dict(z=(0.5 * wu, np.where(j % 8 == 7, 250.0, -np.abs(sweep))), r=(0.5 * np.cos(j), sweep[::-1]), n=cand, b1=np.stack([zero, zero, 0.5 * np.cos(j)]))
        return dict(z=(0.5 * np.sin(j), 0.4 * np.cos(2.0 * j)), r=(0.5 * np.cos(j), sweep), n=cand,
                    b1=np.stack([zero, zero, 3.0 * np.cos(0.7 * j) * (1.0 - 0.5 * (j % 2))]))
    if family == "tanh":
        w = _logspace(1e-3, 8.0, H, shift)
        cand = (w, 0.5 * w * ((j % 3) - 1))
        if kind == "lstm":
            return dict(i=const(ONE), f=const(ZERO), g=cand, o=const(ONE))
        return dict(z=const(ZERO), r=const(0.0), n=cand, b1=np.zeros((3, H)))
    if family == "sigmoid":
        wa, wb = _logspace(0.1, 200.0, H, shift), _logspace(0.1, 200.0, H, shift + H // 2 + 1)
        ba, bb = 0.25 * ((j % 5) - 2), 0.5 * ((j % 3) - 1)
        if kind == "lstm":
            # (f stays below 0.65: |c| below 3, so that c keeps an absolute precision of 1e-7 in fp32)
            return dict(i=(wa, ba), o=(wb, bb), f=(np.cos(j), 0.5 * np.sin(2.0 * j) - 1.0), g=(4.0 * np.sin(1.0 + j), 0.3 * np.cos(3.0 * j)))
        # An update gate held near but not at 1 (z in 0.9 .. 1 - 1e-7) has no relative precision left in 1 - z in fp32, and h integrates
        # that: the fp32 oracle itself ends 7e-6 from fp64 on such a unit. So z sweeps the side where exp overflows, w (x -+ 1) in
        # -2|w| .. 0.5 — z in 0 .. 0.62 —, every eighth unit sits at exactly 1 (w x + 250 >= 50: h never moves), and r takes both sides.
        bz = np.where(j % 8 == 7, 250.0, ba - np.abs(wa))
        return dict(z=(wa, bz), r=(wb, bb), n=(4.0 * np.sin(1.0 + j), 0.3 * np.cos(3.0 * j)), b1=np.stack([zero, zero, 0.5 * np.cos(j)]))
    if family == "clamp":
        assert kind == "lstm"
        w = (24.0 + 16.0 * j / max(H - 1, 1)) * np.where(j % 2, -1.0, 1.0)      # |w| / 2 >= 12: g is +-1 exactly in fp32, c takes exact steps
        return dict(i=const(ONE), f=const(ONE), g=(w, zero), o=(zero, 1.0 + 0.1 * (j % 7)))
    if family == "reset":
        assert kind == "gru"
        b1n = 3.0 * np.cos(0.7 * j) * (1.0 - 0.5 * (j % 2))
        return dict(z=(0.5 * np.sin(j), 0.4 * np.cos(2.0 * j)), r=(_logspace(0.1, 200.0, H, shift), 0.25 * ((j % 5) - 2)),
                    n=(4.0 * np.sin(1.0 + j), 0.3 * np.cos(3.0 * j)), b1=np.stack([zero, zero, b1n]))
    raise ValueError(family)


def make_probe(kind, family, hidden, n_rnn=1):
    """the json dict of a probe model (the schema of workloads.make_model); input_size 1"""
    H = hidden
    gates = "ifgo" if kind == "lstm" else "zrn"
    layers = []
    for l in range(n_rnn):
        u = _units(kind, family, H, 5 * l, upper=l > 0)
        w = np.concatenate([u[g][0] for g in gates]).astype(_f32)
        b = np.concatenate([u[g][1] for g in gates]).astype(_f32)
        if l == 0:
            W = w[None, :]
        else:                                   # unit j reads unit j of the layer below, in every gate
            W = np.zeros((H, len(gates) * H), _f32)
            for g in range(len(gates)):
                W[np.arange(H), g * H + np.arange(H)] = w[g * H:(g + 1) * H]
        U = np.zeros((H, len(gates) * H), _f32)
        bias = b if kind == "lstm" else np.stack([b, u["b1"].reshape(-1).astype(_f32)])
        layers.append({"type": kind, "activation": "", "shape": [None, None, H], "weights": [W.tolist(), U.tolist(), bias.tolist()]})
    j = np.arange(H)
    d = (np.where(j % 2, -1.0, 1.0) * (0.25 + 0.75 * ((7 * j) % H) / H) / np.sqrt(H)).astype(_f32)
    layers.append({"type": "dense", "activation": "", "shape": [None, None, 1], "weights": [d[:, None].tolist(), [0.125]]})
    return {"in_shape": [None, None, 1], "layers": layers,
            "metadata": {"name": f"probe_{kind}{H}x{n_rnn}_{family}", "samplerate": "48000"}}


def dense_l1(j):
    """sum |d_j| of the readout: what an error of 1 in every unit's h can add up to in the output"""
    return float(np.abs(np.asarray(j["layers"][-1]["weights"][0], np.float64)).sum())


def probe_input(family, n_streams):
    """[n_streams][N] float32 in [-1, 1], a different phase per stream.
    tanh / sigmoid / reset: block 0 a slow ramp then noise, block 1 held at one value, block 2 at another, block 3 one sample;
    clamp: a +-0.5 square wave of 40 .. 80 sample halves, started s samples late on stream s."""
    x = np.zeros((n_streams, N), np.float64)
    t = np.arange(N)
    for s in range(n_streams):
        if family == "clamp":
            edges = np.cumsum([0, 40, 80, 80, 80, 80, 80, 80])
            sq = 0.5 * np.where(np.searchsorted(edges, t, side="right") % 2, 1.0, -1.0)
            x[s, s:] = sq[:N - s]
            continue
        rs = np.random.RandomState(0x9E37 + s)
        sign = -1.0 if s % 2 else 1.0
        x[s, :128] = sign * (np.arange(128) / 127.0 * 2.0 - 1.0) * (1.0 - 0.03 * (s % 8))
        u = rs.uniform(-1.0, 1.0, 128)
        x[s, 128:256] = u if family == "tanh" else np.sign(u) * np.abs(u) ** (1.0 / 3.0)      # (the gate sweeps: mostly near full scale)
        held = (1.0, -0.25, 0.75, -1.0, 0.3, -0.8, 0.05, -0.002) if family == "tanh" else (1.0, -0.9, 0.75, -1.0, 0.6, -0.5, 0.95, -0.02)
        x[s, 256:512] = held[s % 8]
        x[s, 512:549] = -held[(s + 3) % 8]
        x[s, 549] = sign
    return x.astype(_f32)


def _sigm(v):
    with np.errstate(over="ignore"):
        return 1.0 / (1.0 + np.exp(-v))


def closed_form(j, x):
    """The probe `j` over the input x[T] from reset state, in fp64 on the model's float32 weights, every sum in the oracle's order
    (oracle/nn_impl.inc). -> dict(h=[layer][T][H], c=[layer][T][H] (LSTM; GRU: zeros), y=[T], pre=[layer] {gate: [T][H]} the
    gates' pre-activations). Raises on a model that is no diagonal probe."""
    cur = np.asarray(x, _f32).astype(np.float64).reshape(-1, 1)
    T = cur.shape[0]
    hs, cs, pres = [], [], []
    for l, layer in enumerate(j["layers"][:-1]):
        kind = layer["type"]
        G = 4 if kind == "lstm" else 3
        W, U, b = (np.asarray(a, _f32).astype(np.float64) for a in layer["weights"])
        H = U.shape[0]
        if np.any(U != 0.0):
            raise ValueError("not a diagonal probe: U != 0")
        if l == 0:
            if W.shape[0] != 1:
                raise ValueError("not a diagonal probe: input_size != 1")
            wx = cur[:, :1] * W[0][None, :]
        else:
            band = np.zeros_like(W)
            for g in range(G):
                band[np.arange(H), g * H + np.arange(H)] = 1.0
            if np.any(W[band == 0.0] != 0.0):
                raise ValueError("not a diagonal probe: W of an upper layer is no diagonal band")
            wx = np.concatenate([cur * W[np.arange(H), g * H + np.arange(H)][None, :] for g in range(G)], axis=1)
        h = np.zeros((T, H))
        c = np.zeros((T, H))
        if kind == "lstm":
            z = b[None, :] + wx
            gi, gf, gg, go = _sigm(z[:, :H]), _sigm(z[:, H:2 * H]), np.tanh(z[:, 2 * H:3 * H]), _sigm(z[:, 3 * H:])
            cp = np.zeros(H)
            for t in range(T):
                cp = gf[t] * cp + gi[t] * gg[t]
                c[t] = cp
            h = go * np.tanh(c)
            pres.append(dict(i=z[:, :H], f=z[:, H:2 * H], g=z[:, 2 * H:3 * H], o=z[:, 3 * H:]))
        else:
            b0, b1 = b[0], b[1]
            pz = wx[:, :H] + 0.0 + (b0[:H] + b1[:H])[None, :]
            pr = wx[:, H:2 * H] + 0.0 + (b0[H:2 * H] + b1[H:2 * H])[None, :]
            gz, gr = _sigm(pz), _sigm(pr)
            pn = wx[:, 2 * H:] + b0[None, 2 * H:] + gr * (0.0 + b1[None, 2 * H:])
            gn = np.tanh(pn)
            hp = np.zeros(H)
            for t in range(T):
                hp = (1.0 - gz[t]) * gn[t] + gz[t] * hp
                h[t] = hp
            pres.append(dict(z=pz, r=pr, n=pn))
        hs.append(h)
        cs.append(c)
        cur = h
    d, bd = (np.asarray(a, _f32).astype(np.float64) for a in j["layers"][-1]["weights"])
    y = np.zeros(T)
    for k in range(d.shape[0]):
        y = y + d[k, 0] * cur[:, k]
    return dict(h=hs, c=cs, y=y + bd[0], pre=pres)


STREAMS = 20                                    # a pool's worth: one full 16-stream group and a ragged one, five 4-stream groups


def pool_controls(family):
    """The controls a probe pool runs under: the defaults — the whole chain in circuit — but for the clamp family, whose input
    low-pass is off: its steps of exactly +-1 are what keeps an integrator that climbs to 40 comparable at 1e-6 when it is back
    near 0, and a filtered edge would put a fraction into c that fp32 then rounds at every binade it crosses."""
    return dict(in_lpf_pc=0.0) if family == "clamp" else {}


_POOL_REF = {}


def pool_reference(kind, family, hidden, n_rnn=1, f64=True):
    """What a warmed-up pool of STREAMS streams must give for the probe over BLOCKS, from the oracle's plugin mirror around the fp64
    network (f64=False: the plain fp32 oracle, for the conditioning tests): dict(y=[STREAMS][N], h / c = [block][layer][STREAMS][H]
    after each block). Computed once per probe, shared by every kernel form's test, read-only."""
    from oracle import oracle as O
    key = (kind, family, hidden, n_rnn, f64)
    if key not in _POOL_REF:
        j = make_probe(kind, family, hidden, n_rnn)
        spec = O.parse_model(j)
        x = probe_input(family, STREAMS)
        ctl = O.default_controls(**pool_controls(family))
        y = np.empty_like(x)
        hs = np.zeros((len(BLOCKS), n_rnn, STREAMS, hidden), _f32)
        cs = np.zeros_like(hs)
        for s in range(STREAMS):
            m = O.OracleModel(spec, f64=f64)
            plug = O.OraclePlugin()
            plug.set_model(m)
            pos = 0
            for bi, n in enumerate(BLOCKS):
                y[s, pos:pos + n] = plug.run(ctl, x[s, pos:pos + n])
                pos += n
                for l in range(n_rnn):
                    hs[bi, l, s], cs[bi, l, s] = m.state(l)
        for a in (x, y, hs, cs):
            a.setflags(write=False)
        _POOL_REF[key] = dict(j=j, x=x, y=y, h=hs, c=cs, l1=dense_l1(j))
    return _POOL_REF[key]
