"""Sparse-recurrent probe models: ONE bf16 term-product family stands alone in a pre-activation, and h is read back.

The recurrent matrix-core kernels (k_gru_gs, k_lstm_gs, k_mfma_ls, k_mfma_ls1) compute every contraction as six (or all nine) of the
nine bf16 term products of operands split into three bf16 terms — the weights by the packer, h on the device. The diagonal probes
of tests/probes.py have U = 0 and hold no recurrent product at all; the random models of tests/test_gpu_parity.py bury a lost
low-order product (2^-17 of one product) under a dense row's sum at 2e-6 of full scale. Here a layer is cut into SOURCES and SINKS:

  sources   the units of one index parity p. Their U rows are zero: h is a function of the layer's input alone, the `tanh` family of
            tests/probes.py — LSTM i = o = 1, f = 0 (biases +-40), g = tanh(w x + b), so h = tanh(tanh(w x + b)); GRU z = 0, h = n =
            tanh(w x + b) — with |h| a little above 0.5 on every held input value and another value per stream.
  sinks     the units of the other parity. Each probes ONE gate G: the gate's W row is zero and its U row has exactly ONE non-zero
            u_j, at column k = (j + s) mod H with s odd — a source. The other gates sit on biases, so that the sink's new state is
            a few-line fp64 function of G's activation of z = u_j h_k + b_j:
                LSTM g   c = tanh(z), h = tanh(c)                      LSTM i   c = sigmoid(z) tanh(b_g)
                LSTM o   h = sigmoid(z) tanh(tanh(b_g))                LSTM f   c <- sigmoid(z) c + tanh(b_g), sigmoid(z) <= 0.6
                GRU n    r = 1: h = tanh(b0 + (u h_k + b1))            GRU r    h = tanh(b0 + sigmoid(z) b1), |b1| in 2 .. 3
                GRU z    h <- n + sigmoid(z) (h - n), n = tanh(w x + b0): shows while h is on its way from one n to another
            The probed gate rotates over the sinks, (j // 2 + rot) mod G: one model probes every gate.
  stacked   the sources of a layer above read ONE source of the layer below through W (candidate row, column (j + s + 1) mod H), and
            its sinks take their one non-zero — rotating with the gate — from U (an own source) or from W (a source of the layer
            below): the hand-over ring's fragments, term by term. (W reads SOURCES only, not every unit of the layer below: a source is a
            function of the held input alone, so the value a frame multiplied with is the value read back whatever the block length.)

There is no recurrent LOOP: a loop with the gain to show a 2^-17 term is no contraction and amplifies every rounding. And nothing is
exact: the reference of a unit is ONE step (or the n steps of a block) in fp64 FROM THE BITS THAT WERE READ BACK — the sources' h after
the block before (what frame 1 multiplied with) and after this block (frames 2 .. n: the input is held and the pre-chain is the
identity under `pool_controls`), the unit's own h / c from before the block. A source's own error never enters a sink's bar.

The weights: u_j is chosen so that the value the kernels hold — fl32(scale * u_j), scale = -log2 e on the sigmoid rows and 2 log2 e on
a GRU's candidate rows (aidax_pack.cpp, mfma_weight) — has |t1| >= 2^-10 |t0| and |t2| >= 2^-18 |t0| (`kernel_weight`, `tune_weight`).
The reference uses the model's own float32 weight; the scaling's rounding belongs to the bar.

The bar (`Layer.cell`, first order, composed through the cell's closed form), from aidax_device.h's stated bounds alone:
    tanh_rat      3.6e-7 relative                                  tanh_exp   2^-23 (1.5 (1 - y) + (1 - y^2) / 2) + 2^-24 |y|
    sigmoid_pre   2^-23 (1.5 s + s (1 - s)): v_exp_f32 and v_rcp_f32 an ulp each, the sum half an ulp — the statement tanh_exp's bound is
                  derived from (tanh_exp = 1 - 2 s); a gate on a bias of +-40 is 1 / 4e-18 to the bit (1 + 2^-58 rounds to 1, rcp(1) = 1)
    pre-activation  C_Z 2^-24 (|W||in| + |U||h| + |b|), C_Z = 10: one for the packer's fp32 multiply of weight and bias by the scale, nine
                  for the accumulation — the accumulator starts from the bias and takes one rounding per term product, each of at most
                  half an ulp of a partial sum that is never above |u h| + |b|; six products: six roundings and the three dropped
                  products, together 2^-23 |u h|, count for two more. The fp32 forms (one product, one rounding) are far inside.
    plus half an ulp for every multiply, add and FMA of the cell update.
It is computed by the reference, before any kernel is looked at. tests/test_term_probes_reference.py shows that an fp32 emulation of the
six-product accumulation stays inside it with the activation errors at their bounds, and that a lost, doubled or misplaced term does not.
"""
import numpy as np

from tests import probes
from tests.test_split_arith import split3

_f32 = np.float32
ONE, ZERO = probes.ONE, probes.ZERO
STREAMS = probes.STREAMS
BLOCKS = (64, 37, 1, 1, 2, 3, 5, 4)                   # frames; every block holds one value per stream (`held`). 64 is the pool's full length.
GATES = {"lstm": "ifgo", "gru": "zrn"}
NEG_LOG2E = _f32(-1.44269504088896340736)       # aidax_pack.cpp: kNegLog2e, kTwoLog2e
TWO_LOG2E = _f32(2.88539008177792681472)
C_Z = 10.0
TANH_RAT_REL = 3.6e-7
EPS = 2.0 ** -24
PRODUCTS6 = ((0, 2), (1, 1), (2, 0), (0, 1), (1, 0), (0, 0))          # (weight term, h term), smallest first: tests/test_split_arith.py, k_*_gs
PRODUCTS6_LS = ((0, 0), (1, 0), (2, 0), (0, 1), (1, 1), (0, 2))       # k_mfma_ls: by h term, the large ones first


def pool_controls():
    """the input low-pass off (as the clamp family of tests/probes.py): the pre-chain is then a copy times a gain ramp that rests at
    exactly 1 — the network's input IS the held value (tests/test_term_probes_reference.py checks that on the oracle)"""
    return dict(in_lpf_pc=0.0)


def held(n_streams=STREAMS):
    """[block][stream] float32: the value each stream holds in each block. |x| in 0.3 .. 1, another value per stream and block, the sign
    alternating from block to block (a GRU's update gate shows only while h moves)."""
    s = np.arange(n_streams)
    out = []
    for b in range(len(BLOCKS)):
        mag = 0.3 + 0.7 * (((7 * s + 3 * b) % 20) + 0.37 * ((s + b) % 3)) / 20.74
        out.append(mag * np.where((s + b) % 2, -1.0, 1.0))
    return np.array(out).astype(_f32)


def scale_of(kind, gate):
    if gate in "ifozr":
        return NEG_LOG2E
    return TWO_LOG2E if kind == "gru" else _f32(1.0)


def kernel_weight(kind, gate, u):
    """the value a matrix-core form holds for the model's float32 weight u: ONE fp32 multiply by the row's scale"""
    return (scale_of(kind, gate) * np.asarray(u, _f32)).astype(_f32)


def tune_weight(kind, gate, held_mag, sign=1.0):
    """A float32 weight whose kernel value fl32(scale * u) lies within 9 % above `held_mag` — just above a power of two, where the low terms
    are largest against the value — and has the most substantial second and third bf16 terms of the 700 candidates: the one that maximises
    min(|t1| / 2^(e - 8), |t2| / 2^(e - 16)), 2^e <= |value| < 2^(e + 1) (each is at most 1). What is asked of it — |t1| >= 2^-10 |t0|,
    |t2| >= 2^-18 |t0| — is asserted by tests/test_term_probes_reference.py on every weight of every model."""
    sc = abs(float(scale_of(kind, gate)))
    cand = (_f32(sign * held_mag / sc) * (1.0 + np.arange(700) * 2.0 ** -13)).astype(_f32)
    v = kernel_weight(kind, gate, cand)
    t0, t1, t2 = split3(v)
    e = np.floor(np.log2(np.abs(v.astype(np.float64))))
    score = np.minimum(np.abs(t1) / 2.0 ** (e - 8), np.abs(t2) / 2.0 ** (e - 16))
    return cand[np.argmax(score)]


def _source_hbar(kind, b):
    return np.tanh(np.tanh(b)) if kind == "lstm" else np.tanh(b)


def _swing(kind, n_rnn, l, u, parity, rot):
    """GRU stacks: every fourth source below the top layer follows the SIGN of the held input, h = tanh(1.3 x) (above: of the swing
    source below it), for the candidates of the update-gate sinks above — an update gate shows only while h is on its way from one n
    to another, and the other sources hardly move (a sink's pre-activation is centred on them). No single product reads one."""
    return kind == "gru" and l < n_rnn - 1 and u % 2 == parity and (u // 2 + rot) % 4 == 3


def _column(kind, n_rnn, l_src, k, parity, rot, H):
    while _swing(kind, n_rnn, l_src, k, parity, rot):
        k = (k + 2) % H
    return k


def layout(kind, hidden, n_rnn, parity, shift, rot):
    """plan[l] = list over the units of layer l of dict(role='src'|'swing'|'sink', gate, seg ('U' | 'W' | None: a first-layer source),
    col, ncol: the swing source below an upper update-gate sink's candidate reads)"""
    H, gates = hidden, GATES[kind]
    G = len(gates)
    assert H % 2 == 0 and shift % 2 == 1
    cand = "g" if kind == "lstm" else "n"
    plan = []
    for l in range(n_rnn):
        units = []
        for u in range(H):
            if _swing(kind, n_rnn, l, u, parity, rot):
                units.append(dict(role="swing", gate=cand, seg=None if l == 0 else "W", col=0 if l == 0 else u, ncol=None))
            elif u % 2 == parity:
                units.append(dict(role="src", gate=cand, seg=None if l == 0 else "W", ncol=None,
                                  col=0 if l == 0 else _column(kind, n_rnn, l - 1, (u + shift + 1) % H, parity, rot, H)))
            else:
                turn = u // 2 + rot
                g = gates[turn % G]
                seg = "W" if (l > 0 and (turn // G) % 2 == 0) else "U"
                k = _column(kind, n_rnn, l - 1 if seg == "W" else l, (u + shift) % H, parity, rot, H)
                ncol = None
                if g == "z" and l > 0:
                    ncol = (u + 1) % H
                    while not _swing(kind, n_rnn, l - 1, ncol, parity, rot):
                        ncol = (ncol + 2) % H
                units.append(dict(role="sink", gate=g, seg=seg, col=k, ncol=ncol))
        plan.append(units)
    return plan


def make(kind, hidden, n_rnn, parity, shift, rot):
    """-> (json dict in the schema of workloads.make_model, plan: see `layout`)"""
    H, gates = hidden, GATES[kind]
    G = len(gates)
    plan = layout(kind, hidden, n_rnn, parity, shift, rot)
    cand = "g" if kind == "lstm" else "n"
    layers = []
    src_b_below = None
    for l in range(n_rnn):
        I = 1 if l == 0 else H
        W = np.zeros((I, G * H), _f32)
        U = np.zeros((H, G * H), _f32)
        b = np.zeros((2, G * H), _f32)                   # GRU: [input bias, recurrent bias]; LSTM: row 0
        col = {g: gi * H + np.arange(H) for gi, g in enumerate(gates)}
        j = np.arange(H)
        # the sources' candidate bias: |h| a little above 0.5 (0.50 .. 0.61 with what the input adds: +-0.025 below, +-0.08 above) — just above a
        # power of two, where h's second and third bf16 terms are largest against h: |h2| reaches 2^-17 |h| there, 2^-18 |h| just below 1 —,
        # the sign by the unit
        src_b = ((0.70 + 0.06 * ((5 * j + 3 * l) % 11) / 10.0) if kind == "lstm" else (0.61 + 0.04 * ((5 * j + 3 * l) % 11) / 10.0)) * np.where((j // 2 + l) % 2, -1.0, 1.0)
        for u, d in enumerate(plan[l]):
            fix = dict(i=ONE, f=ZERO, o=ONE) if kind == "lstm" else dict(z=ZERO, r=0.0)
            if d["role"] == "swing":
                for g, v in fix.items():
                    b[0, col[g][u]] = v
                W[d["col"], col[cand][u]] = (1.3 if u % 4 < 2 else -1.3) if l == 0 else 1.6
                continue
            if d["role"] == "src":
                for g, v in fix.items():
                    b[0, col[g][u]] = v
                if l == 0:
                    W[0, col[cand][u]] = 0.025 * np.sin(1.0 + u)
                    b[0, col[cand][u]] = src_b[u]
                else:                                    # reads ONE source below: z = w h_k + b around src_b[u]
                    k = d["col"]
                    hbar = _source_hbar(kind, src_b_below[k])
                    w = tune_weight(kind, cand, 4.15 if kind == "lstm" else 8.3, np.sign(hbar))
                    W[k, col[cand][u]] = w
                    b[0, col[cand][u]] = src_b[u] - float(w) * hbar
                continue
            # ---- a sink: gate g from one product
            g, seg, k = d["gate"], d["seg"], d["col"]
            hbar = _source_hbar(kind, (src_b_below if seg == "W" else src_b)[k])
            # the held value a little above 16 (the LSTM's candidate, unscaled: 4): |u h| is 3.2 on a GRU's candidate, 2.3 on the LSTM's and
            # 6.3 on the sigmoid rows — beyond the 2 .. 4 that keeps the pre-activation's own rounding small, because a sigmoid gate shows a
            # term only through a state whose OTHER factors carry their activations' relative errors (tanh(c) behind o, b1 behind r): at
            # |u h| = 3.2 the third h term of the o and r rows stayed inside three bars on every stream, at 6.3 it does not
            w = tune_weight(kind, g, dict(g=4.15).get(g, 16.6), (1.0 if (g in "gn" or (u // 2) % 2 == 0) else -1.0) * np.sign(hbar))
            (W if seg == "W" else U)[k, col[g][u]] = w
            centre = -float(w) * hbar
            if kind == "lstm":
                # z of g and i around 0, of o around 0.5, of f around -0.6 (sigmoid(z) <= 0.6 wherever the sources go)
                off = dict(g=0.25 * np.sin(u), i=0.3 * np.cos(u), o=0.3 * np.sin(u), f=-0.5)[g]
                bias = dict(i=ONE, f=ZERO, g=(0.9 if u % 4 < 2 else -0.9), o=ONE)
                if g == "f":
                    bias["g"] = 0.3 if u % 4 < 2 else -0.3          # c = tanh(b_g) / (1 - f) stays below 0.75
                bias[g] = centre + off
                for gg, v in bias.items():
                    b[0, col[gg][u]] = v
            else:
                off = dict(n=0.25 * np.sin(u), r=0.3 * np.cos(u), z=0.2 * np.sin(u))[g]
                if g == "n":                             # r = 1: h = tanh(b0 + (u h + b1))
                    b[0, col["z"][u]], b[0, col["r"][u]] = ZERO, ONE
                    if seg == "U":
                        b[0, col["n"][u]], b[1, col["n"][u]] = off, centre
                    else:                                # (through W the product sits in the candidate's input half)
                        b[0, col["n"][u]], b[1, col["n"][u]] = centre, off
                elif g == "r":                           # h = tanh(b0 + r b1)
                    b[0, col["z"][u]], b[0, col["r"][u]] = ZERO, centre + off
                    b1n = (2.0 + ((u // 2) % 5) / 4.0) * (1.0 if u % 4 < 2 else -1.0)
                    b[0, col["n"][u]], b[1, col["n"][u]] = 0.2 * np.cos(u) - 0.5 * b1n, b1n      # (around r = 0.5 the candidate sits near 0.2 cos u)
                else:                                    # z: n = tanh(+-2.5 x) / tanh(2 h of a swing source below) follows the input's sign
                    b[0, col["z"][u]], b[0, col["r"][u]] = centre + off, 0.0
                    if l == 0:
                        W[0, col["n"][u]] = 2.5 if u % 4 < 2 else -2.5
                    else:
                        W[d["ncol"], col["n"][u]] = 2.0
        src_b_below = src_b
        bias = b[0] if kind == "lstm" else b
        layers.append({"type": kind, "activation": "", "shape": [None, None, H], "weights": [W.tolist(), U.tolist(), bias.tolist()]})
    jj = np.arange(H)
    d = (np.where(jj % 2, -1.0, 1.0) * (0.25 + 0.75 * ((7 * jj) % H) / H) / np.sqrt(H)).astype(_f32)
    layers.append({"type": "dense", "activation": "", "shape": [None, None, 1], "weights": [d[:, None].tolist(), [0.125]]})
    j = {"in_shape": [None, None, 1], "layers": layers,
         "metadata": {"name": f"term_{kind}{H}x{n_rnn}_p{parity}s{shift}r{rot}", "samplerate": "48000"}}
    return j, plan


def classes_of(plan, hidden):
    """the (layer, segment, row tile, gate, k-step of 32) combinations a model's single products sit in, and the columns it reads"""
    cls, cols = set(), set()
    for l, units in enumerate(plan):
        for u, d in enumerate(units):
            if d["seg"] is not None and d["role"] != "swing":
                cls.add((l, d["seg"], u // 16, d["gate"], d["col"] // 32))
                cols.add((l, d["seg"], d["col"]))
    return cls, cols


def wanted_classes(kind, hidden, n_rnn):
    """every (row tile, gate, k-step) of every layer's U; of the upper layers' W as well"""
    T, KS = (hidden + 15) // 16, (hidden + 31) // 32
    return {(l, seg, t, g, ks) for l in range(n_rnn) for seg in (("U",) if l == 0 else ("U", "W"))
            for t in range(T) for g in GATES[kind] for ks in range(KS)}


_MODELS = {}


def models(kind, hidden, n_rnn):
    """The models of one (cell, H, layers): both parities, every rotation — every (row, gate) of every 16-row tile is probed —, then odd
    shifts added greedily until every (layer, segment, row tile, gate, k-step) occurs in two rows; every column is read.
    -> list of (json, plan, (parity, shift, rot)), computed once."""
    key = (kind, hidden, n_rnn)
    if key in _MODELS:
        return _MODELS[key]
    G = len(GATES[kind])
    rots = range(G if n_rnn == 1 else 2 * G)
    want = wanted_classes(kind, hidden, n_rnn)
    chosen, count = [], {}

    def units_of(plan):
        """(class, unit) pairs: a class counts as reached once TWO different rows hold a product of it (one row alone can sit on a
        source whose low terms happen to be small on most streams)"""
        return {(unit_class(d, l, u), u) for l, units in enumerate(plan) for u, d in enumerate(units) if d["seg"] is not None and d["role"] != "swing"}

    def short():
        return {c for c in want if len(count.get(c, ())) < 2}

    def add(p, s, r):
        j, plan = make(kind, hidden, n_rnn, p, s, r)
        for c, u in units_of(plan):
            count.setdefault(c, set()).add(u)
        chosen.append((j, plan, (p, s, r)))
    for p in (0, 1):
        for r in rots:
            add(p, 1, r)
    while short():
        need = short()
        best, gain = None, 0
        for s in range(3, hidden, 2):
            for p in (0, 1):
                for r in rots:
                    g = len({(c, u) for c, u in units_of(layout(kind, hidden, n_rnn, p, s, r)) if c in need and u not in count.get(c, ())})
                    if g > gain:
                        best, gain = (p, s, r), g
        assert best is not None, sorted(need)
        add(*best)
    _MODELS[key] = chosen
    return chosen


# ------------------------------------------------------------------------------------------------ the reference step and its bar
def _sigm(v):
    with np.errstate(over="ignore"):
        return 1.0 / (1.0 + np.exp(-v))


def sigmoid_bound(s):
    return 2.0 ** -23 * (1.5 * s + s * (1.0 - s))


def tanh_exp_bound(y):
    return 2.0 ** -23 * (1.5 * (1.0 - y) + 0.5 * (1.0 - y * y)) + EPS * np.abs(y)


def _sig_with_bar(pre, ez, act):
    s = _sigm(pre)
    sat = np.abs(pre) >= 30.0                        # a gate on a +-40 bias: 1 / 4e-18 to the bit
    return s, np.where(sat, 0.0, act * sigmoid_bound(s) + s * (1.0 - s) * ez)


class Layer:
    """one recurrent layer of a probe model as float32 matrices, with the fp64 step, its bar and the bf16 term-product emulation"""

    def __init__(self, j, l):
        L = j["layers"][l]
        self.kind = L["type"]
        self.gates = GATES[self.kind]
        self.W, self.U = (np.asarray(a, _f32) for a in L["weights"][:2])
        b = np.asarray(L["weights"][2], _f32)
        self.H = self.U.shape[0]
        self.b = b if self.kind == "gru" else np.stack([b, np.zeros_like(b)])

    def _cols(self, g):
        gi = self.gates.index(g)
        return slice(gi * self.H, (gi + 1) * self.H)

    def pre_exact(self, x_in, h_prev):
        """fp64 pre-activations from the float32 weights: {gate: (value, magnitude sum)}; GRU: 'n' is (input half, recurrent half) twice"""
        x, h = np.asarray(x_in, np.float64), np.asarray(h_prev, np.float64)
        W, U, b = (a.astype(np.float64) for a in (self.W, self.U, self.b))
        out = {}
        for g in self.gates:
            c = self._cols(g)
            a_in, a_rec = x @ W[:, c], h @ U[:, c]
            m_in, m_rec = np.abs(x) @ np.abs(W[:, c]), np.abs(h) @ np.abs(U[:, c])
            if self.kind == "gru" and g == "n":
                out[g] = ((a_in + b[0, c], a_rec + b[1, c]), (m_in + np.abs(b[0, c]), m_rec + np.abs(b[1, c])))
            else:
                out[g] = (a_in + a_rec + (b[0, c] + b[1, c]), m_in + m_rec + np.abs(b[0, c]) + np.abs(b[1, c]))
        return out

    def terms(self, x_in, h_prev):
        """What pre_emulated accumulates, computed once per (input, h) and shared by every mutation: {gate: dict(inp=[S][H] the first layer's
        fp32 input product or None, W / U = {(a, b, ks): [S][H]} the bf16 term products (weight term a, operand term b) of the columns of
        k-step ks)} — from the values a matrix-core form holds: weights times the row's scale, one fp32 multiply, split into three bf16
        terms; a bf16 x bf16 product is exact in fp32, and a row has one non-zero, so every entry is one exact product."""
        x32, h32 = np.asarray(x_in, _f32), np.asarray(h_prev, _f32)
        first = self.W.shape[0] == 1
        out = {}
        for g in self.gates:
            c = self._cols(g)
            sc = scale_of(self.kind, g)
            d = dict(inp=None, W={}, U={})
            for seg, M, v in (("W", self.W, x32), ("U", self.U, h32)):
                if seg == "W" and first:
                    d["inp"] = x32.astype(np.float64) @ (sc * M[:, c]).astype(_f32).astype(np.float64)
                    continue
                Ws = [w.astype(np.float64) for w in split3((sc * M[:, c]).astype(_f32))]
                Vs = [t.astype(np.float64) for t in split3(v)]
                for ks in range((M.shape[0] + 31) // 32):
                    rows = slice(32 * ks, min(32 * ks + 32, M.shape[0]))
                    if not np.any(Ws[0][rows]):
                        continue
                    for a in range(3):
                        for bb in range(3):
                            d[seg][(a, bb, ks)] = Vs[bb][:, rows] @ Ws[a][rows]
            out[g] = d
        return out

    def pre_emulated(self, x_in, h_prev, order=PRODUCTS6, mutate=None, terms=None):
        """The pre-activations as a matrix-core form accumulates them: in fp32 onto the scaled bias, the first layer's input product
        first, then the term products of `order` (every k-step of a product in turn), one rounding each. Returned UNSCALED (divided by
        the scale in fp64), in pre_exact's shape, magnitudes None.
        mutate = (kind, seg, k-step or None, a, b): on the columns of that k-step of that segment, 'drop' / 'double' the product (a, b),
        'swap_h' (h1 where h2 belongs and the reverse) or 'swap_w'."""
        T = self.terms(x_in, h_prev) if terms is None else terms
        swap = {0: 0, 1: 2, 2: 1}
        out = {}
        for g in self.gates:
            c = self._cols(g)
            sc = scale_of(self.kind, g)
            d = T[g]

            def accumulate(bias, segs):
                acc = None
                for seg in segs:
                    if seg == "inp":
                        if d["inp"] is not None:
                            acc = (np.float64(1.0) * (sc * bias).astype(_f32) + d["inp"]).astype(_f32)
                        continue
                    kss = sorted({k[2] for k in d[seg]})
                    for (a, bb) in order:
                        for ks in kss:
                            a2, b2, rep = a, bb, 1
                            if mutate is not None and mutate[1] == seg and mutate[2] in (None, ks):
                                if mutate[0] in ("drop", "double") and (a, bb) == (mutate[3], mutate[4]):
                                    rep = 0 if mutate[0] == "drop" else 2
                                elif mutate[0] == "swap_h":
                                    b2 = swap[bb]
                                elif mutate[0] == "swap_w":
                                    a2 = swap[a]
                            for _ in range(rep):
                                base = (sc * bias).astype(_f32) if acc is None else acc
                                acc = (base.astype(np.float64) + d[seg][(a2, b2, ks)]).astype(_f32)
                if acc is None:
                    acc = np.broadcast_to((sc * bias).astype(_f32), (np.asarray(h_prev).shape[0], self.H))
                return acc.astype(np.float64) / np.float64(sc)

            if self.kind == "gru" and g == "n":
                out[g] = ((accumulate(self.b[0, c], ("inp", "W")), accumulate(self.b[1, c], ("U",))), None)
            else:
                out[g] = (accumulate((self.b[0, c] + self.b[1, c]).astype(_f32), ("inp", "W", "U")), None)
        return out

    def cell(self, pre, h_prev, c_prev, e_h_prev, e_c_prev, mags=None, act=1.0, rat=False):
        """the cell update in fp64 from pre-activations `pre` -> h, c, bar_h, bar_c. mags None: the pre-activations carry no error term
        (C_Z = 0). act = 0: the activations and the cell's own roundings carry none either. rat: a GRU candidate on tanh_rat (k_stack)."""
        ez = (lambda g, part=None: 0.0) if mags is None else \
             (lambda g, part=None: C_Z * EPS * (pre[g][1] if part is None else pre[g][1][part]))
        rnd = act * EPS
        if self.kind == "lstm":
            i, ei = _sig_with_bar(pre["i"][0], ez("i"), act)
            f, ef = _sig_with_bar(pre["f"][0], ez("f"), act)
            o, eo = _sig_with_bar(pre["o"][0], ez("o"), act)
            gg = np.tanh(pre["g"][0])
            eg = act * TANH_RAT_REL * np.abs(gg) + (1.0 - gg * gg) * ez("g")
            c = f * c_prev + i * gg
            ec = np.abs(c_prev) * ef + f * e_c_prev + np.abs(gg) * ei + i * eg + rnd * (np.abs(i * gg) + np.abs(c))
            tc = np.tanh(c)
            etc = act * TANH_RAT_REL * np.abs(tc) + (1.0 - tc * tc) * ec
            h = o * tc
            return h, c, np.abs(tc) * eo + o * etc + rnd * np.abs(h), ec
        z, e_z = _sig_with_bar(pre["z"][0], ez("z"), act)
        r, e_r = _sig_with_bar(pre["r"][0], ez("r"), act)
        (n_in, n_rec) = pre["n"][0]
        pn = n_in + r * n_rec
        e_pn = ez("n", 0) + np.abs(n_rec) * e_r + r * ez("n", 1) + rnd * np.abs(pn)
        n = np.tanh(pn)
        e_n = act * (TANH_RAT_REL * np.abs(n) if rat else tanh_exp_bound(n)) + (1.0 - n * n) * e_pn
        d = h_prev - n
        h = n + z * d
        e_h = np.abs(d) * e_z + (1.0 - z) * e_n + z * e_h_prev + rnd * (z * np.abs(d) + np.abs(h))
        return h, np.zeros_like(h), e_h, np.zeros_like(h)

    def run(self, n, x_first, x_rest, hk_first, hk_rest, h0, c0, emulate=None, act=1.0, with_z=True, memo=None):
        """n frames of a block. x_*: this layer's input (the held value [S][1], or the read-back bits of the layer below [S][H]) in
        frame 1 / frames 2 .. n; hk_*: the h the U products multiply with in frame 1 (read back BEFORE the block) and in frames 2 .. n
        (read back after it: the sources rest); h0, c0: the units' own state before the block, what the elementwise recurrences start from.
        emulate = dict(order=..., mutate=...): the pre-activations from the bf16 term-product emulation instead of fp64 (memo: a dict
        that keeps the term products between calls on the same bits).
        -> h, c, bar_h, bar_c after the block"""
        h, c = np.asarray(h0, np.float64), np.asarray(c0, np.float64)
        eh, ec = np.zeros_like(h), np.zeros_like(h)
        if emulate is None:
            pre_first = self.pre_exact(x_first, hk_first)
            pre_rest = self.pre_exact(x_rest, hk_rest) if n > 1 else None
        else:
            memo = {} if memo is None else memo
            if "first" not in memo:
                memo["first"] = self.terms(x_first, hk_first)
                memo["rest"] = self.terms(x_rest, hk_rest) if n > 1 else None
            pre_first = self.pre_emulated(x_first, hk_first, terms=memo["first"], **emulate)
            pre_rest = self.pre_emulated(x_rest, hk_rest, terms=memo["rest"], **emulate) if n > 1 else None
        return self.run_pre(n, pre_first, pre_rest, h, c, mags=(True if (with_z and emulate is None) else None), act=act)

    def run_pre(self, n, pre_first, pre_rest, h, c, mags=None, act=1.0):
        eh, ec = np.zeros_like(h), np.zeros_like(h)
        for t in range(n):
            h, c, eh, ec = self.cell(pre_first if t == 0 else pre_rest, h, c, eh, ec, mags=mags, act=act)
        return h, c, eh, ec


_LAYERS = {}


def layer_of(j, l):
    key = (j["metadata"]["name"], len(j["layers"]), l)
    if key not in _LAYERS:
        _LAYERS[key] = Layer(j, l)
    return _LAYERS[key]


def source_mask(plan_l):
    return np.array([d["role"] != "sink" for d in plan_l])


def reference_block(j, plan, n, x_new, state_before, state_after, emulate=None, act=1.0, with_z=True, layers=None, memo=None):
    """Every layer's units after a block of n frames holding x_new ([S]), from read-back bits: state_before / state_after =
    [layer] (h [S][H], c [S][H]) before and after the block. A layer above reads the SOURCES below, which rest on the held input from
    frame 1 on: their bits after the block. -> [layer] (h, c, bar_h, bar_c) (layers: only those, None elsewhere)."""
    out = []
    for l in range(len(plan)):
        if layers is not None and l not in layers:
            out.append(None)
            continue
        L = layer_of(j, l)
        x_in = np.asarray(x_new, _f32)[:, None] if l == 0 else state_after[l - 1][0]
        out.append(L.run(n, x_in, x_in, state_before[l][0], state_after[l][0], state_before[l][0], state_before[l][1],
                         emulate=emulate, act=act, with_z=with_z, memo=None if memo is None else memo.setdefault(l, {})))
    return out


def closed_form_sources(j, plan, x):
    """the SOURCES of every layer on the held value x [S], fp64 from the model's float32 weights: [layer] h [S][H] (sinks: nan)"""
    out, below = [], None
    for l in range(len(plan)):
        L = layer_of(j, l)
        src = source_mask(plan[l])
        x_in = np.asarray(x, np.float64)[:, None] if l == 0 else np.where(np.isnan(below), 0.0, below)
        z = np.zeros((x_in.shape[0], L.H))
        h, _, _, _ = L.cell(L.pre_exact(x_in, z), z, z, z, z, mags=None, act=0.0)
        h = np.where(src[None, :], h, np.nan)
        out.append(h)
        below = h
    return out


# ------------------------------------------------------------------------------------------------ judging a block from read-back bits
MUTATIONS = [("drop", a, b) for a, b in PRODUCTS6] + [("double", a, b) for a, b in PRODUCTS6] + [("swap_h", None, None), ("swap_w", None, None)]
SEEN_FACTOR = 3.0                               # an observation SEES a mutation that moves it by this many bars


def judged(plan_l, l):
    """the units of a layer that hold one term-product family alone: the sinks, and above the first layer the sources"""
    return np.array([d["seg"] is not None and d["role"] != "swing" for d in plan_l])


def unit_class(d, l, u):
    return (l, d["seg"], u // 16, d["gate"], d["col"] // 32)


def moved_by(j, plan, n, x_new, before, after, mutations, order=PRODUCTS6, ks=None):
    """{mutation: [layer] (|h(mutated) - h(as designed)|, the same of c) [S][H]} at the given bits: the emulation with the mutation on
    the segment that holds the unit's product (ks: on one k-step only) against the emulation without. (The mutations of a layer run
    through the cell update side by side, stacked in front of the stream axis.)"""
    out = {m: [] for m in mutations}
    for l in range(len(plan)):
        L = layer_of(j, l)
        x_in = np.asarray(x_new, _f32)[:, None] if l == 0 else after[l - 1][0]
        t_first = L.terms(x_in, before[l][0])
        t_rest = L.terms(x_in, after[l][0]) if n > 1 else None
        segs = ("U",) if l == 0 else ("U", "W")
        specs = [None] + [(m[0], seg, ks, m[1], m[2]) for m in mutations for seg in segs]

        def stacked(terms, hk):
            pres = [L.pre_emulated(x_in, hk, terms=terms, order=order, mutate=sp) for sp in specs]
            return {g: ((tuple(np.stack([p[g][0][i] for p in pres]) for i in (0, 1)) if isinstance(pres[0][g][0], tuple)
                         else np.stack([p[g][0] for p in pres])), None) for g in L.gates}
        h0 = np.broadcast_to(np.asarray(before[l][0], np.float64), (len(specs),) + before[l][0].shape)
        c0 = np.broadcast_to(np.asarray(before[l][1], np.float64), h0.shape)
        h, c, _, _ = L.run_pre(n, stacked(t_first, before[l][0]), stacked(t_rest, after[l][0]) if n > 1 else None, h0, c0, mags=None, act=0.0)
        own = np.array([segs.index(d["seg"]) if d["seg"] in segs else 0 for d in plan[l]])
        for mi, m in enumerate(mutations):
            pick = 1 + mi * len(segs) + own                       # per unit: the row of the stack with the mutation on its own segment
            hm = np.take_along_axis(h, pick[None, None, :].repeat(h.shape[1], 1), 0)[0]
            cm = np.take_along_axis(c, pick[None, None, :].repeat(h.shape[1], 1), 0)[0]
            out[m].append((np.abs(hm - h[0]), np.abs(cm - c[0])))
    return out


def emulated_run(j, plan, order=PRODUCTS6, mutate=None, x=None):
    """The blocks of `held` through the emulation from a zero state, block by block: -> [block] [layer] (h, c) as float32 — the bits a
    kernel that does what the emulation does would hand to read_state —, and the same in fp64 before that rounding."""
    X = held() if x is None else x
    S = X.shape[1]
    H = len(plan[0])
    state = [(np.zeros((S, H), _f32), np.zeros((S, H), _f32)) for _ in plan]
    bits, exact = [state], []
    for bi, n in enumerate(BLOCKS):
        after = [None] * len(plan)
        ex = [None] * len(plan)
        for l in range(len(plan)):
            # the sources do not read U: a first pass gives them, the second gives the sinks that multiply with them
            guess = list(after)
            guess[l] = state[l]
            for _ in range(2):
                r = reference_block(j, plan, n, X[bi], state, guess, emulate=dict(order=order, mutate=mutate), layers=(l,))
                guess[l] = (r[l][0].astype(_f32), r[l][1].astype(_f32))
            after[l], ex[l] = guess[l], (r[l][0], r[l][1])
        bits.append(after)
        exact.append(ex)
        state = after
    return bits, exact


def tally(j, plan, bits, mutations, seen, tot, order=PRODUCTS6):
    """One model's blocks judged from `bits` ([block + 1][layer] (h, c): the read-back before the first block and after each):
    -> [block] [layer] (h, c, bar_h, bar_c), the reference with its bars; and per (unit class, mutation) the number of (stream, unit,
    block) observations that SEE the mutation — it moves h or c by SEEN_FACTOR bars — added into `seen`, all of them into `tot`."""
    X = held(bits[0][0][0].shape[0])
    refs = []
    for bi, n in enumerate(BLOCKS):
        ref = reference_block(j, plan, n, X[bi], bits[bi], bits[bi + 1])
        refs.append(ref)
        if not mutations:
            continue
        for m, per in moved_by(j, plan, n, X[bi], bits[bi], bits[bi + 1], mutations, order=order).items():
            for l in range(len(plan)):
                hit = (per[l][0] >= SEEN_FACTOR * ref[l][2]) | ((per[l][1] >= SEEN_FACTOR * ref[l][3]) & (ref[l][3] > 0.0))
                n_hit = hit.sum(0)
                for u, d in enumerate(plan[l]):
                    if d["seg"] is not None and d["role"] != "swing":
                        k = (unit_class(d, l, u), m)
                        seen[k] = seen.get(k, 0) + int(n_hit[u])
                        tot[k] = tot.get(k, 0) + hit.shape[0]
    return refs


def unseen(kind, hidden, n_rnn, seen, mutations):
    """the (class, mutation) pairs no observation saw"""
    return sorted(str((c, m)) for c in wanted_classes(kind, hidden, n_rnn) for m in mutations if seen.get((c, m), 0) == 0)


KEPT = [("drop", a, b) for a, b in PRODUCTS6]       # what the GPU test asks its own read-backs for: every kept product of every class
