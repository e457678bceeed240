"""The cell activations of every kernel form on saturating models (run with -m gpu on an MI355X).

The sigmoid and tanh of the recurrent kernels exist in many hand-written copies (aidax_device.h: fast_sigmoid, sigmoid_pre,
tanh_rat with its clamp at 7.9, tanh_exp / tanh_exp_pre, and the tanh-form sigmoid 0.5 tanh_rat(z / 2) + 0.5 of the one-wave
LSTM's shared lane maps and of k_lstm_q4; aidax_tick.hip and aidax_mfmals.h deal the same operations out by hand between MFMA groups), and the
random models of the parity tests keep every pre-activation within about +-3. Here the diagonal probe models of tests/probes.py
(U = 0: each unit its own (w, b) per gate, an fp64 closed form — established as a reference, together with its conditioning, by
tests/test_probes_reference.py) drive them to exactly 0 and 1, through the overflow of exp (|z| up to 200), down to |x| = 1e-6
where only relative accuracy counts, and take the cell state across the clamp — on every kernel form that serves the cell, with
`pool.kernel_name` asserted so that a change of the pool's table cannot quietly move a case to another kernel. The cases that
set no switch run on the shipped library too and join the ship leg's bit-identity digest.

Bars — from the header's own numbers and an fp32 emulation of its functions, not from what the kernels measured:
  * per-unit state, h and c where |c| <= 8: 1e-6 absolute (tanh_rat <= 3.6e-7 relative, tanh_exp 1.2e-7 and the tanh-form sigmoid
    1.9e-7 absolute, exp2 and rcp an ulp each; the emulated LSTM cell ended at 4.8e-7 / 2.5e-7); |c| > 8: 4e-7 |c|;
  * Dense output: 1e-6 sum|d_j| for the bare network, times max(1, downstream linear gain) — 1 under these controls — for a pool
    (the rule of tests/test_gpu_parity.py's docstring); the pools of every family but `clamp` measured 5e-8 and are held to 5e-7;
  * the tanh family's held blocks, state read back after >= 16 equal samples: every unit with |ref| >= 1e-5 within 2e-6 |ref| —
    on EVERY LSTM form and on k_stack's GRU, which evaluate the candidate with tanh_rat; this is the check that fails if a tanh_exp
    gets into an LSTM. The other GRU forms use tanh_exp BY DESIGN (a GRU has no cell state that integrates the error): they are
    held to ITS bound instead, which is absolute — aidax_device.h derives it from the one ulp each of v_exp_f32 and v_rcp_f32:
    2^-23 (1.5 (1 - y) + (1 - y^2) / 2) + 2^-24 |y|, 2.4e-7 at the small end, where the two forms differ by orders of magnitude (the
    header used to say "~1.2e-7": a typical figure, the first run of this test found a unit of the 64-wide forms at 1.22e-7 plus
    roundings) — plus what the number format puts around the function: the rounding of the pre-activation z it is given,
    6 * 2^-24 |z| tanh'(z) (a weight and a bias that the packer scaled by 2 log2 e and rounded, |w x| + |b| <= 5 |z| on the held
    values — tests/test_probes_reference.py —, and one FMA), which vanishes with |h|.
Every comparison goes through errlog.bound with a tag per family and form; the maxima measured on an MI355X are in
profiles/activation_probe_errors.json.
"""
import importlib
import json

import numpy as np
import pytest

from tests import errlog, probes

pytestmark = pytest.mark.gpu

ax = importlib.import_module("aidadsp-lv2_amd")

STATE_BAR = 1.0e-6            # h, and c where |c| <= 8
C_REL_BAR = 4.0e-7            # c where |c| > 8, relative
OUT_BAR = 1.0e-6              # times sum|d_j|: the bare network, and the clamp family's pools (measured up to 2.5e-7 / 1.7e-7)
POOL_OUT_BAR = 5.0e-7         # ... the other families' pools: ten times the 5.0e-8 measured, as tests/errlog.py prescribes
REL_BAR = 2.0e-6              # tanh family, held blocks, tanh_rat forms: relative, for |ref| >= 1e-5


def _tanh_exp_bound(y):
    """aidax_device.h, tanh_exp: |error| at the true value y, the argument taken as exact"""
    return 2.0 ** -23 * (1.5 * (1.0 - y) + 0.5 * (1.0 - y * y)) + 2.0 ** -24 * np.abs(y)


K = "AIDAX_KERNEL"
# id: (cell, hidden, layers, switches, kernel name, candidate on tanh_rat?). The name is what a block of the pool's full length runs: a pool
# on k_*_pipe4 passes its ragged blocks (37 and 1 frames here) through k_*_pipe on the same state.
FORMS = {
    # one-layer LSTM
    "lstm-wave12": ("lstm", 12, 1, {K: "wave"}, "k_lstm<12>", True),                   # lane map S = 4: i, f, o on the tanh-form sigmoid
    "lstm-wave32": ("lstm", 32, 1, {K: "wave"}, "k_lstm<32>", True),                   # S = 2: o on the tanh-form sigmoid
    "lstm-wave64": ("lstm", 64, 1, {K: "wave"}, "k_lstm<64>", True),                   # S = 1
    "lstm-pipe32": ("lstm", 32, 1, {K: "pipe", "AIDAX_PIPE4": "0"}, "k_lstm_pipe<32>", True),
    "lstm-pipe4-32": ("lstm", 32, 1, {}, "k_lstm_pipe4<32>", True),
    "lstm-pipe4-12": ("lstm", 12, 1, {}, "k_lstm_pipe4<12>", True),
    "lstm-pipe40": ("lstm", 40, 1, {}, "k_lstm_pipe<40>", True),
    "lstm-split32": ("lstm", 32, 1, {K: "split"}, "k_chain+k_nn<lstm32>", True),
    "lstm-quad32": ("lstm", 32, 1, {K: "quad"}, "k_chain+k_quad", True),
    "lstm-quad64": ("lstm", 64, 1, {}, "k_chain+k_quad", True),                        # what a small LSTM-64 pool gets
    "lstm-valu32": ("lstm", 32, 1, {K: "valu"}, "k_lstm_pipe<32>", True),
    "lstm-q4": ("lstm", 32, 1, {K: "q4"}, "k_lstm_q4<32>", True),
    "lstm-mfma32": ("lstm", 32, 1, {K: "mfma", "AIDAX_LS1": "0"}, "k_mfma_lp", True),
    "lstm-ls1-32": ("lstm", 32, 1, {K: "mfma", "AIDAX_LS1": "1"}, "k_mfma_ls1", True),
    "lstm-ls1-40": ("lstm", 40, 1, {K: "mfma", "AIDAX_LS1": "1"}, "k_mfma_ls1", True),
    "lstm-gs40": ("lstm", 40, 1, {K: "mfma", "AIDAX_LSTM_GS": "1"}, "k_lstm_gs", True),
    "lstm-gs64": ("lstm", 64, 1, {K: "mfma", "AIDAX_LSTM_GS": "1"}, "k_lstm_gs", True),
    "lstm-gs9-40": ("lstm", 40, 1, {K: "mfma", "AIDAX_LSTM_GS": "1", "AIDAX_GS_PRODUCTS": "9"}, "k_lstm_gs", True),
    "lstm-gs9-64": ("lstm", 64, 1, {K: "mfma", "AIDAX_LSTM_GS": "1", "AIDAX_GS_PRODUCTS": "9"}, "k_lstm_gs", True),
    # one-layer GRU
    "gru-wave16": ("gru", 16, 1, {K: "wave"}, "k_gru<16>", False),
    "gru-pipe16": ("gru", 16, 1, {K: "pipe", "AIDAX_PIPE4": "0"}, "k_gru_pipe<16>", False),
    "gru-pipe4-16": ("gru", 16, 1, {}, "k_gru_pipe4<16>", False),
    "gru-pipe32": ("gru", 32, 1, {}, "k_gru_pipe<32>", False),
    "gru-quad80": ("gru", 80, 1, {}, "k_chain+k_quad", False),
    "gru-quad16": ("gru", 16, 1, {K: "quad"}, "k_chain+k_quad", False),
    "gru-valu16": ("gru", 16, 1, {K: "valu"}, "k_gru_pipe<16>", False),
    "gru-mfma64": ("gru", 64, 1, {K: "mfma", "AIDAX_GRU_GM": "0"}, "k_mfma_lp", False),
    "gru-gm64": ("gru", 64, 1, {K: "mfma", "AIDAX_GRU_GM": "f32"}, "k_gru_gm", False),
    "gru-gs64": ("gru", 64, 1, {}, "k_gru_gs", False),
    "gru-gs80": ("gru", 80, 1, {K: "mfma"}, "k_gru_gs", False),
    "gru-ls1-16": ("gru", 16, 1, {K: "mfma", "AIDAX_LS1": "1", "AIDAX_GRU_GM": "0"}, "k_mfma_ls1", False),
    # stacked: the smallest widths k_mfma_ls takes (test_split_stack_geometries_match_the_oracle: LSTM-16 x 2, GRU-40 x 3 run as 48)
    "lstm16x2-ls": ("lstm", 16, 2, {}, "k_mfma_ls", True),
    "lstm16x2-lp": ("lstm", 16, 2, {"AIDAX_LP_SPLIT": "0"}, "k_mfma_lp", True),
    "lstm16x2-mfma": ("lstm", 16, 2, {"AIDAX_MFMA_LP": "0"}, "k_chain+k_mfma", True),
    "lstm16x2-valu": ("lstm", 16, 2, {K: "valu"}, "k_stack", True),
    "gru40x3-ls": ("gru", 40, 3, {}, "k_mfma_ls", False),
    "gru40x3-lp": ("gru", 40, 3, {"AIDAX_LP_SPLIT": "0"}, "k_mfma_lp", False),
    "gru40x3-mfma": ("gru", 40, 3, {"AIDAX_MFMA_LP": "0"}, "k_chain+k_mfma", False),
    "gru40x3-valu": ("gru", 40, 3, {K: "valu"}, "k_stack", True),                      # k_stack's GRU candidate is a tanh_rat
}
CASES = [(form, family) for form, f in FORMS.items() for family in probes.FAMILIES[f[0]]]


class _Bars:
    """errlog.bound for every comparison of a test, the misses raised together at its end: one run shows every figure of a form"""

    def __init__(self):
        self.missed = []

    def __call__(self, err, tol, tag):
        try:
            errlog.bound(err, tol, tag)
        except AssertionError as e:
            self.missed.append(e.args[0])

    def done(self):
        assert not self.missed, self.missed


def _check_state(bound, tag, h, c, rh, rc, lstm):
    bound(np.abs(h - rh).max(), STATE_BAR, tag + ":h")
    if lstm:
        big = np.abs(rc) > 8.0
        bound(np.abs(c - rc)[~big].max(initial=0.0), STATE_BAR, tag + ":c")
        if big.any():
            bound((np.abs(c - rc)[big] / np.abs(rc)[big]).max(), C_REL_BAR, tag + ":c_rel")


@pytest.mark.parametrize("form,family", CASES)
def test_pool_on_a_probe_matches_the_fp64_oracle_per_unit(form, family, monkeypatch):
    """20 streams (a full 16-stream group and a ragged one, five 4-stream groups), each at another input phase, blocks of 256, 256,
    37 and 1 frames, the whole chain in circuit: output and per-unit h / c after every block against the oracle's plugin mirror
    around the fp64 network."""
    cell, hidden, n_rnn, env, name, rat = FORMS[form]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    ref = probes.pool_reference(cell, family, hidden, n_rnn)
    tag = f"probe:{family}:{form}"
    S, bound = probes.STREAMS, _Bars()
    pool = ax.Pool(S, 256)
    pool.set_model(ax.Model(text=json.dumps(ref["j"])))
    pool.set_controls(ax.default_controls(**probes.pool_controls(family)))
    pos = 0
    for bi, n in enumerate(probes.BLOCKS):
        got = pool.process(np.ascontiguousarray(ref["x"][:, pos:pos + n]))
        assert pool.kernel_name == name, (bi, pool.kernel_name)
        assert np.all(np.isfinite(got)), (tag, bi)
        bound(np.abs(got - ref["y"][:, pos:pos + n]).max(), (OUT_BAR if family == "clamp" else POOL_OUT_BAR) * ref["l1"], tag + ":out")
        pos += n
        for l in range(n_rnn):
            st = [pool.read_state(s, l) for s in range(S)]
            h, c = np.array([a for a, _ in st]), np.array([b for _, b in st])
            assert h.shape == (S, hidden) and np.all(np.isfinite(h)) and np.all(np.isfinite(c))
            _check_state(bound, tag, h, c, ref["h"][bi, l], ref["c"][bi, l], cell == "lstm")
            if family == "tanh" and l == 0 and bi in (1, 2):
                # the block held one input value for n >= 16 samples (what the input low-pass makes of it has settled): h is the
                # candidate of that value alone
                r = ref["h"][bi, 0].astype(np.float64)
                if rat:
                    big = np.abs(r) >= 1e-5
                    assert big.sum() >= S * hidden // 2
                    bound((np.abs(h - r)[big] / np.abs(r)[big]).max(), REL_BAR, tag + ":held_rel")
                else:
                    ra = np.minimum(np.abs(r), 1.0 - 2.0 ** -24)          # (a reference that rounded to 1: the last float below, z tanh'(z) is 1e-6 there)
                    allowed = _tanh_exp_bound(r) + 2.0 ** -24 * 6.0 * np.arctanh(ra) * (1.0 - ra * ra)
                    bound((np.abs(h - r) / allowed).max(), 1.0, tag + ":held_abs_over_bound")
                    bound(np.abs(h - r)[np.abs(r) < 1e-2].max(), 2.0 ** -22, tag + ":held_abs_small")
    pool.close()
    bound.done()


@pytest.mark.parametrize("form,family", CASES)
def test_bare_network_on_a_probe_matches_the_closed_form(form, family, monkeypatch):
    """Model.forward (reset state, unit gains, no chain) under the same switches against the numpy closed form."""
    cell, hidden, n_rnn, env, _, _ = FORMS[form]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    j = probes.make_probe(cell, family, hidden, n_rnn)
    X = probes.probe_input(family, 6)
    m = ax.Model(text=json.dumps(j))
    for s in (0, 5):
        y = m.forward(X[s][:, None], unit_gains=True)
        assert np.all(np.isfinite(y))
        errlog.bound(np.abs(y - probes.closed_form(j, X[s])["y"]).max(), OUT_BAR * probes.dense_l1(j), f"probe:{family}:{form}:bare")
