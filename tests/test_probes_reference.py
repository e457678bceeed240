"""The diagonal probe models (tests/probes.py) as a REFERENCE, established on the CPU before any kernel is judged by them
(tests/test_gpu_activations.py): for every probe of every family

  * the numpy closed form and the fp64 C oracle agree after rounding to float32 — two independent statements of the cell;
  * the plain fp32 oracle stays within 2.5e-7 * sum|d_j| of the closed form (d the Dense row): a probe that misses this is
    ill-conditioned — a forget gate left near but not at 1, say — and no kernel can be held to 1e-6 on it;
  * the probes reach what they are for: the sigmoid family has a quarter of its swept gate evaluations beyond |z| = 16 and a
    twentieth beyond 88 (exp overflows fp32 there), the clamp family takes every unit's |c| across 7.9 at least four times,
    the tanh family's held blocks are well-conditioned in RELATIVE terms down to |h| = 1e-5.
"""
import numpy as np
import pytest

from oracle import oracle as O
from tests import probes

WIDTHS = (12, 32, 40)
CASES = [(kind, fam, H, 1) for kind in ("lstm", "gru") for fam in probes.FAMILIES[kind] for H in WIDTHS] + \
        [("lstm", fam, 16, 2) for fam in probes.FAMILIES["lstm"]] + [("gru", fam, 16, 3) for fam in probes.FAMILIES["gru"]]
STREAMS = (0, 3, 5)


def _same(got32, ref64):
    """equal after rounding to float32 — or, where the clamp family's integrator comes back to zero and leaves 1e-15 of its own
    fp64 rounding behind, within 1e-12: two fp64 evaluations with different libm's agree on nothing about such a residue"""
    return bool(np.all((got32 == ref64.astype(np.float32)) | (np.abs(got32 - ref64) <= 1e-12)))


def _states_f64(spec, x, n_rnn):
    """h, c of every layer after every sample, from the fp64 oracle (as float32: what orc_net_state hands out)"""
    m = O.OracleModel(spec, warmup=False, f64=True)
    hs = [[] for _ in range(n_rnn)]
    cs = [[] for _ in range(n_rnn)]
    y = np.empty_like(x)
    for t in range(x.size):
        y[t] = m.apply(x[t:t + 1])[0]
        for l in range(n_rnn):
            h, c = m.state(l)
            hs[l].append(h)
            cs[l].append(c)
    return y, [np.array(a) for a in hs], [np.array(a) for a in cs]


@pytest.mark.parametrize("kind,family,hidden,n_rnn", CASES)
def test_closed_form_is_the_fp64_oracle_and_the_fp32_oracle_is_near(kind, family, hidden, n_rnn):
    j = probes.make_probe(kind, family, hidden, n_rnn)
    spec = O.parse_model(j)
    X = probes.probe_input(family, max(STREAMS) + 1)
    l1 = probes.dense_l1(j)
    for s in STREAMS:
        ref = probes.closed_form(j, X[s])
        assert np.all(np.isfinite(ref["y"]))
        y64 = O.net_run(spec, X[s], f64=True)
        assert np.array_equal(y64, ref["y"].astype(np.float32)), (s, np.abs(y64 - ref["y"]).max())
        y32 = O.net_run(spec, X[s])
        err = np.abs(y32 - ref["y"]).max()
        assert err <= 2.5e-7 * l1, (s, err / l1)
    yb, hs, cs = _states_f64(spec, X[1][:300], n_rnn)
    ref = probes.closed_form(j, X[1][:300])
    assert _same(yb, ref["y"])
    for l in range(n_rnn):
        assert _same(hs[l], ref["h"][l]), l
        if kind == "lstm":
            assert _same(cs[l], ref["c"][l]), l


@pytest.mark.parametrize("kind", ["lstm", "gru"])
@pytest.mark.parametrize("hidden", (12, 16, 32, 40, 64, 80))
def test_sigmoid_family_reaches_past_the_overflow_of_exp(kind, hidden):
    j = probes.make_probe(kind, "sigmoid", hidden)
    X = probes.probe_input("sigmoid", 20)
    swept = ("i", "o") if kind == "lstm" else ("z", "r")
    z = np.concatenate([np.abs(probes.closed_form(j, X[s])["pre"][0][g]).ravel() for s in range(20) for g in swept])
    assert z.max() > 190.0
    assert np.mean(z > 16.0) >= 0.25, np.mean(z > 16.0)
    assert np.mean(z > 88.0) >= 0.05, np.mean(z > 88.0)


def test_reset_family_sweeps_r_through_overflow_under_a_large_recurrent_bias():
    j = probes.make_probe("gru", "reset", 40)
    X = probes.probe_input("reset", 20)
    pr = np.concatenate([np.abs(probes.closed_form(j, X[s])["pre"][0]["r"]).ravel() for s in range(20)])
    assert np.mean(pr > 16.0) >= 0.25 and np.mean(pr > 88.0) >= 0.05
    b1n = np.abs(np.asarray(j["layers"][0]["weights"][2])[1, 80:])
    assert 2.9 < b1n.max() <= 3.0


@pytest.mark.parametrize("hidden", (12, 32, 40, 64))
def test_clamp_family_takes_every_cell_across_the_tanh_clamp(hidden):
    j = probes.make_probe("lstm", "clamp", hidden)
    X = probes.probe_input("clamp", 20)
    for s in (0, 7, 19):
        c = np.abs(probes.closed_form(j, X[s])["c"][0])
        assert c.max() > 39.0
        crossings = np.sum((c[1:] > 7.9) != (c[:-1] > 7.9), axis=0)
        assert crossings.min() >= 4, crossings.min()


@pytest.mark.parametrize("kind", ["lstm", "gru"])
def test_tanh_family_covers_the_small_end_and_its_held_blocks_are_well_conditioned(kind):
    """the relative bar of the GPU test (2e-6 of |h| down to |h| = 1e-5) asks nothing the fp32 oracle itself does not deliver
    with room to spare on the held blocks: 5e-7"""
    j = probes.make_probe(kind, "tanh", 40)
    spec = O.parse_model(j)
    X = probes.probe_input("tanh", 8)
    # no cancellation to speak of in w x + b on the held values: |w x| + |b| <= 5 |w x + b| (the GPU test's allowance for the rounding
    # of a pre-activation whose weight and bias the packer scaled counts on it)
    w, b = (np.asarray(a, np.float64) for a in (j["layers"][0]["weights"][0], j["layers"][0]["weights"][2]))
    w, b = w[0, -40:] if kind == "gru" else w[0, 80:120], b[0, -40:] if kind == "gru" else b[80:120]
    for xh in np.unique(X[:, 256:549]):
        assert np.all(np.abs(w * xh) + np.abs(b) <= 5.0 * np.abs(w * xh + b) + 1e-12), xh
    small = 0
    for s in range(8):
        ref = probes.closed_form(j, X[s])["h"][0]
        m = O.OracleModel(spec, warmup=False)
        for b0, n in zip(np.cumsum((0,) + probes.BLOCKS[:-1]), probes.BLOCKS):
            m.apply(X[s, b0:b0 + n])
            if n in (256, 37) and b0 > 0:
                h, r = m.state(0)[0].astype(np.float64), ref[b0 + n - 1]
                big = np.abs(r) >= 1e-5
                small += int(np.sum(big & (np.abs(r) < 1e-2)))
                assert np.all(np.abs(h - r)[big] <= 5e-7 * np.abs(r)[big]), (s, b0)
    assert small >= 40          # the probes reach the range where only a RELATIVELY accurate tanh passes
