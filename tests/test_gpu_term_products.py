"""Every kept bf16 term product of the recurrent matrix-core kernels, one product family alone in a pre-activation (run with -m gpu on
an MI355X).

k_gru_gs, k_lstm_gs, k_mfma_ls and k_mfma_ls1 compute every contraction as six (or all nine) of the nine bf16 term products of operands
split into three bf16 terms. The activation probes (tests/test_gpu_activations.py) have U = 0, and the random models of
tests/test_gpu_parity.py bury a lost w0 h2, w1 h1 or w2 h0 — 2^-17 of one product — under a dense row's sum at 2e-6 of full scale. The
sparse-recurrent probe models of tests/termprobes.py put ONE such product family into a pre-activation and read h back; the reference
is the block's frames in fp64 from the read-back bits, the bar is composed from aidax_device.h's stated bounds (there; established with
an emulation, and with what a lost, doubled or misplaced term does to it, by tests/test_term_probes_reference.py). Per form:

  * 20 streams, blocks of 64, 37, 1, 1, 2, 3, 5 and 4 frames, each holding one value per stream, the input low-pass off: the pre-chain
    is the identity; read_state of every stream and layer before the first block and after each. The long blocks end in a steady
    state — the in-loop path —, the one-frame blocks multiply with h as it came from HBM, the short ones show a GRU's update gate
    while h is on its way;
  * pool.kernel_name asserted on the full-length block;
  * the layer-0 sources against their closed form at tests/test_gpu_activations.py's STATE_BAR; every unit that holds one product —
    the sinks, and above the first layer the sources — against the reference within ITS bar: errlog.bound of the largest error / bar
    per form and gate, bar 1;
  * before the sinks are judged: from the bits that were read back, every (layer, segment, row tile, gate, k-step, kept product) is
    SEEN — dropping the product would move h or c by three bars — by at least one (stream, unit, block). A run that could not have
    noticed a lost term fails instead of passing.
The fp32 forms (k_gru_gm, k_mfma_lp, k_chain+k_mfma) have no terms; they meet the same bars, and this is the first test of their U
routing row by row. Maxima measured on an MI355X: profiles/term_probe_errors.json; what the test does to a library that loses a term:
profiles/term_probes.txt.
"""
import importlib
import json

import numpy as np
import pytest

from tests import errlog
from tests import termprobes as T
from tests.test_gpu_activations import STATE_BAR, _Bars

pytestmark = pytest.mark.gpu

ax = importlib.import_module("aidadsp-lv2_amd")

K = "AIDAX_KERNEL"
_GS, _LS1 = {K: "mfma", "AIDAX_LSTM_GS": "1"}, {K: "mfma", "AIDAX_LS1": "1"}
# id: (cell, hidden, layers, switches, kernel name of a full-length block)
FORMS = {
    "gru-gs64": ("gru", 64, 1, {}, "k_gru_gs"),
    "gru-gs80": ("gru", 80, 1, {K: "mfma"}, "k_gru_gs"),
    "lstm-gs40": ("lstm", 40, 1, _GS, "k_lstm_gs"),
    "lstm-gs64": ("lstm", 64, 1, _GS, "k_lstm_gs"),
    "lstm-gs9-40": ("lstm", 40, 1, dict(_GS, AIDAX_GS_PRODUCTS="9"), "k_lstm_gs"),
    "lstm-gs9-64": ("lstm", 64, 1, dict(_GS, AIDAX_GS_PRODUCTS="9"), "k_lstm_gs"),
    "lstm-ls1-32": ("lstm", 32, 1, _LS1, "k_mfma_ls1"),
    "lstm-ls1-40": ("lstm", 40, 1, _LS1, "k_mfma_ls1"),
    "lstm-ls1-80": ("lstm", 80, 1, _LS1, "k_mfma_ls1"),                              # the four-wave geometry
    "gru-ls1-16": ("gru", 16, 1, dict(_LS1, AIDAX_GRU_GM="0"), "k_mfma_ls1"),
    "lstm16x2-ls": ("lstm", 16, 2, {}, "k_mfma_ls"),
    "gru40x3-ls": ("gru", 40, 3, {}, "k_mfma_ls"),
    "lstm96x2-ls": ("lstm", 96, 2, {}, "k_mfma_ls"),                                 # cfg5's geometry: three k-steps, K = 192 above
    # (under AIDAX_LP_SPLIT=9 the 512-register geometries still issue six products — nine spill, aidax_mfmals.h: ls_fn_for —, so the state bits
    # of this case are those of the one above; the small stack below is where k_mfma_ls issues all nine)
    "lstm96x2-ls9": ("lstm", 96, 2, {"AIDAX_LP_SPLIT": "9"}, "k_mfma_ls"),
    "lstm16x2-ls9": ("lstm", 16, 2, {"AIDAX_LP_SPLIT": "9"}, "k_mfma_ls"),
    # fp32 controls
    "gru-gm64": ("gru", 64, 1, {K: "mfma", "AIDAX_GRU_GM": "f32"}, "k_gru_gm"),
    "gru-mfma64": ("gru", 64, 1, {K: "mfma", "AIDAX_GRU_GM": "0"}, "k_mfma_lp"),
    "lstm-mfma32": ("lstm", 32, 1, {K: "mfma", "AIDAX_LS1": "0"}, "k_mfma_lp"),
    "lstm16x2-lp": ("lstm", 16, 2, {"AIDAX_LP_SPLIT": "0"}, "k_mfma_lp"),
    "gru40x3-lp": ("gru", 40, 3, {"AIDAX_LP_SPLIT": "0"}, "k_mfma_lp"),
    "lstm16x2-mfma": ("lstm", 16, 2, {"AIDAX_MFMA_LP": "0"}, "k_chain+k_mfma"),
    "gru40x3-mfma": ("gru", 40, 3, {"AIDAX_MFMA_LP": "0"}, "k_chain+k_mfma"),
}


def _read(pool, S, n_rnn):
    out = []
    for l in range(n_rnn):
        st = [pool.read_state(s, l) for s in range(S)]
        out.append((np.array([a for a, _ in st]), np.array([b for _, b in st])))
    return out


@pytest.mark.parametrize("form", list(FORMS))
def test_every_unit_with_one_product_matches_its_fp64_step(form, monkeypatch):
    cell, hidden, n_rnn, env, name = FORMS[form]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    S, bound = T.STREAMS, _Bars()
    X = T.held(S)
    pool = ax.Pool(S, T.BLOCKS[0])
    runs = []
    for j, plan, key in T.models(cell, hidden, n_rnn):
        pool.set_model(ax.Model(text=json.dumps(j)))
        pool.set_controls(ax.default_controls(**T.pool_controls()))
        bits = [_read(pool, S, n_rnn)]
        for bi, n in enumerate(T.BLOCKS):
            got = pool.process(np.ascontiguousarray(np.repeat(X[bi][:, None], n, axis=1)))
            if bi == 0:
                assert pool.kernel_name == name, (key, pool.kernel_name)
            assert np.all(np.isfinite(got)), (form, key, bi)
            bits.append(_read(pool, S, n_rnn))
        for b in bits:
            for h, c in b:
                assert h.shape == (S, hidden) and np.all(np.isfinite(h)) and np.all(np.isfinite(c))
        runs.append((j, plan, key, bits))
    pool.close()
    # could this run have seen a lost term? — from the bits it read back, before any sink is judged
    seen, tot, refs = {}, {}, []
    for j, plan, key, bits in runs:
        refs.append(T.tally(j, plan, bits, T.KEPT, seen, tot))
    assert not T.unseen(cell, hidden, n_rnn, seen, T.KEPT)
    for (j, plan, key, bits), ref in zip(runs, refs):
        for bi in range(len(T.BLOCKS)):
            want = T.closed_form_sources(j, plan, X[bi])
            for l in range(n_rnn):
                h, c = bits[bi + 1][l]
                plain = np.array([d["seg"] is None or d["role"] == "swing" for d in plan[l]])       # the sources that hold no product (of the probed kind)
                if plain.any():
                    bound(np.abs(h - want[l])[:, plain].max(), STATE_BAR, f"term:{form}:src")
                rh, rc, bh, bc = ref[bi][l]
                for g in T.GATES[cell]:
                    m = np.array([d["seg"] is not None and d["role"] != "swing" and d["gate"] == g for d in plan[l]])
                    if not m.any():
                        continue
                    bound((np.abs(h - rh) / bh)[:, m].max(), 1.0, f"term:{form}:{g}:h_over_bar")
                    if cell == "lstm":
                        bound((np.abs(c - rc) / bc)[:, m].max(), 1.0, f"term:{form}:{g}:c_over_bar")
    bound.done()
