"""The sparse-recurrent probe models (tests/termprobes.py) as a REFERENCE with bars, established on the CPU before any kernel is
judged by them (tests/test_gpu_term_products.py):

  * under the probes' controls the pre-chain is the identity on a held block: the input low-pass is skipped, the pre-gain ramp rests
    at exactly 1, and the fp64 oracle's sources sit on the closed form of the held value itself from a block's first frame on;
  * the reference step — n frames in fp64 from read-back bits — is the fp64 C oracle's cell: started from the oracle's own states
    it lands on the oracle's next states (two independent statements of the cell);
  * every probing weight has three substantial bf16 terms IN THE VALUE THE KERNELS HOLD (one fp32 multiply by the row's scale), the
    sources' |h| (0.25 .. 0.9) and the products |u h| (1.3 .. 8) are where the design puts them, a probed forget gate stays below 0.6; the models of a form
    reach every (layer, segment, row tile, gate, k-step), every (row, gate) of every tile and every column;
  * an fp32 emulation of the term-product accumulation — six products in either kernel's order, or all nine —, with the activation
    errors put at their header bounds in the worst direction, stays inside the bars on every unit: SHARE_USED of the room the bar
    leaves for the pre-activation is the most it took;
  * every single mutation — one kept product dropped or doubled, h1 and h2 swapped, w1 and w2 swapped — moves the sinks it touches
    by three bars or more at the emulation's source bits, for a share of the observations that is measured (profiles/term_probes.txt);
    not every observation can see the smallest products (h's low terms are what the bits are), so the condition is per CLASS: every
    (layer, segment, row tile, gate, k-step, mutation) is seen by at least one (stream, unit, block) among the 20 streams; a mutation
    confined to one k-step moves nothing in another.
The bars are tests/termprobes.py's, from aidax_device.h's stated bounds; nothing here or there is taken from what a kernel measured.
"""
import numpy as np
import pytest

from oracle import oracle as O
from tests import termprobes as T
from tests.test_split_arith import split3

# the geometries of tests/test_gpu_term_products.py
GEOS = [("gru", 64, 1), ("gru", 80, 1), ("lstm", 40, 1), ("lstm", 64, 1), ("lstm", 32, 1), ("lstm", 80, 1), ("gru", 16, 1),
        ("lstm", 16, 2), ("gru", 40, 3), ("lstm", 96, 2)]
SMALL = [("gru", 16, 1), ("lstm", 32, 1), ("lstm", 16, 2), ("gru", 40, 3)]
SHARE_USED = 0.35          # of the pre-activation's room; measured 0.07 .. 0.29 (profiles/term_probes.txt)
PRODUCTS9 = ((2, 2), (1, 2), (2, 1)) + T.PRODUCTS6


def _oracle_blocks(j, n_rnn, x_blocks, per_frame=False):
    """one stream through the fp64 oracle's plugin mirror under the probes' controls: [block + 1][layer] (h, c) (per_frame: after every frame)"""
    spec = O.parse_model(j)
    m = O.OracleModel(spec, f64=True)
    plug = O.OraclePlugin()
    plug.set_model(m)
    ctl = O.default_controls(**T.pool_controls())
    out = [[m.state(l) for l in range(n_rnn)]]
    for n, v in x_blocks:
        x = np.full(n, v, np.float32)
        if per_frame:
            for t in range(n):
                plug.run(ctl, x[t:t + 1])
                out.append([m.state(l) for l in range(n_rnn)])
        else:
            plug.run(ctl, x)
            out.append([m.state(l) for l in range(n_rnn)])
    return out, plug


@pytest.mark.parametrize("kind,hidden,n_rnn", [("lstm", 16, 2), ("gru", 40, 3)])
def test_the_pre_chain_is_the_identity_on_a_held_block(kind, hidden, n_rnn):
    j, plan, _ = T.models(kind, hidden, n_rnn)[3]
    X = T.held()
    for s in (0, 7, 19):
        blocks = [(5, X[0, s]), (4, X[1, s]), (1, X[2, s])]
        states, plug = _oracle_blocks(j, n_rnn, blocks, per_frame=True)
        assert plug.p.in_lpf_pc_old == 0.0                                   # (run() copies the input when the control is 0)
        assert plug.p.preGain.mem == 1.0 and plug.p.preGain.target == 1.0
        t = 1
        for n, v in blocks:
            want = T.closed_form_sources(j, plan, np.array([v]))
            for _ in range(n):                                               # from the block's FIRST frame on
                for l in range(n_rnn):
                    src = T.source_mask(plan[l])
                    assert np.array_equal(states[t][l][0][src], want[l][0][src].astype(np.float32)), (s, t, l)
                t += 1


@pytest.mark.parametrize("kind,hidden,n_rnn", SMALL)
def test_the_reference_step_is_the_fp64_oracle(kind, hidden, n_rnn):
    """... to what the float32 read-back of a source leaves open: 2^-25 |h| times |u| = 11.5 in a pre-activation, 2e-7, and the float32
    rounding of the state that is compared"""
    X = T.held()
    for j, plan, _ in T.models(kind, hidden, n_rnn)[::3]:
        for s in (1, 12):
            states, _ = _oracle_blocks(j, n_rnn, [(n, X[bi, s]) for bi, n in enumerate(T.BLOCKS)])
            for bi, n in enumerate(T.BLOCKS):
                before = [(h[None, :], c[None, :]) for h, c in states[bi]]
                after = [(h[None, :], c[None, :]) for h, c in states[bi + 1]]
                ref = T.reference_block(j, plan, n, X[bi, s:s + 1], before, after)
                for l in range(n_rnn):
                    assert np.abs(ref[l][0] - after[l][0]).max() < 4e-7, (bi, l)
                    if kind == "lstm":
                        assert np.abs(ref[l][1] - after[l][1]).max() < 4e-7, (bi, l)


@pytest.mark.parametrize("kind,hidden,n_rnn", GEOS)
def test_weights_magnitudes_and_coverage(kind, hidden, n_rnn):
    ms = T.models(kind, hidden, n_rnn)
    assert len(ms) <= 24
    X = T.held()
    classes, cols, rows = set(), set(), set()
    for j, plan, _ in ms:
        c, k = T.classes_of(plan, hidden)
        classes |= c
        cols |= k
        bits, _ = T.emulated_run(j, plan)
        for l in range(n_rnn):
            L = T.layer_of(j, l)
            src = T.source_mask(plan[l])
            for bi in range(len(T.BLOCKS)):
                ah = np.abs(bits[bi + 1][l][0][:, src])
                assert 0.25 <= ah.min() and ah.max() <= 0.9, (l, bi, ah.min(), ah.max())
            for u, d in enumerate(plan[l]):
                if d["seg"] is None or d["role"] == "swing":
                    continue
                rows.add((l, d["seg"], u, d["gate"]))
                M = L.W if d["seg"] == "W" else L.U
                colw = M[:, L._cols(d["gate"])][:, u]
                assert np.count_nonzero(colw) == 1 and colw[d["col"]] != 0.0                # ONE product in the probed pre-activation
                if d["role"] == "sink":
                    other = (L.U if d["seg"] == "W" else L.W)[:, L._cols(d["gate"])][:, u]
                    assert not np.any(other)
                t0, t1, t2 = (float(t[0]) for t in split3(T.kernel_weight(kind, d["gate"], colw[d["col"]:d["col"] + 1])))
                assert abs(t1) >= 2.0 ** -10 * abs(t0) and abs(t2) >= 2.0 ** -18 * abs(t0), (l, u, t0, t1, t2)
                below = l - 1 if d["seg"] == "W" else l
                uh = np.abs(float(colw[d["col"]]) * np.stack([bits[bi + 1][below][0][:, d["col"]] for bi in range(len(T.BLOCKS))]))
                assert 1.3 <= uh.min() and uh.max() <= 8.0, (l, u, uh.min(), uh.max())
                if d["gate"] == "f":
                    pre = float(colw[d["col"]]) * bits[2][below][0][:, d["col"]].astype(np.float64) + float(L.b[0, L._cols("f")][u])
                    assert np.all(1.0 / (1.0 + np.exp(-pre)) <= 0.6)
    assert classes >= T.wanted_classes(kind, hidden, n_rnn)
    for l in range(n_rnn):
        for seg in (("U",) if l == 0 else ("U", "W")):
            assert {c for (ll, sg, c) in cols if (ll, sg) == (l, seg)} == set(range(hidden)), (l, seg)      # every column is read
            for g in T.GATES[kind]:
                assert {u for (ll, sg, u, gg) in rows if (ll, sg, gg) == (l, seg, g)} == set(range(hidden)), (l, seg, g)   # every row of every gate


@pytest.mark.parametrize("kind,hidden,n_rnn", GEOS)
@pytest.mark.parametrize("order", ["gs6", "ls6", "nine"])
def test_the_emulation_stays_inside_the_bars(kind, hidden, n_rnn, order):
    products = dict(gs6=T.PRODUCTS6, ls6=T.PRODUCTS6_LS, nine=PRODUCTS9)[order]
    X = T.held()
    worst = 0.0
    for j, plan, _ in T.models(kind, hidden, n_rnn)[::2]:
        bits, exact = T.emulated_run(j, plan, order=products)
        for bi, n in enumerate(T.BLOCKS):
            full = T.reference_block(j, plan, n, X[bi], bits[bi], bits[bi + 1])
            act = T.reference_block(j, plan, n, X[bi], bits[bi], bits[bi + 1], with_z=False)     # the activations' share of the bar: where the injected errors go
            for l in range(n_rnn):
                jm = T.judged(plan[l], l)
                for q in ((0, 2), (1, 3))[:2 if kind == "lstm" else 1]:
                    err = np.abs(exact[bi][l][q[0]] - full[l][q[0]])[:, jm]
                    room = (full[l][q[1]] - act[l][q[1]])[:, jm]
                    assert np.all(room > 0.0)
                    worst = max(worst, float((err / room).max()))
    print(f"term probes, {kind}{hidden}x{n_rnn} {order}: the emulation used {worst:.3f} of the pre-activation's room")
    assert worst <= SHARE_USED, worst


@pytest.mark.parametrize("kind,hidden,n_rnn", [g for g in GEOS if g != ("lstm", 96, 2)] + [pytest.param("lstm", 96, 2, id="lstm-96-2")])
def test_every_mutation_is_seen_in_every_class(kind, hidden, n_rnn):
    seen, tot = {}, {}
    ms = T.models(kind, hidden, n_rnn)
    for j, plan, _ in ms:
        bits, _ = T.emulated_run(j, plan)
        T.tally(j, plan, bits, T.MUTATIONS, seen, tot)
    assert not T.unseen(kind, hidden, n_rnn, seen, T.MUTATIONS)
    for m in T.MUTATIONS:
        share = [seen[k] / tot[k] for k in seen if k[1] == m]
        print(f"term probes, {kind}{hidden}x{n_rnn} {m}: seen by {min(share):.3f} .. {max(share):.3f} of a class's observations, {np.mean(share):.3f} overall")


def test_a_mutation_in_one_k_step_moves_nothing_in_another():
    j, plan, _ = T.models("lstm", 64, 1)[0]
    bits, _ = T.emulated_run(j, plan)
    X = T.held()
    ks_of = np.array([d["col"] // 32 for d in plan[0]])
    for ks in (0, 1):
        mv = T.moved_by(j, plan, 37, X[1], bits[1], bits[2], [("drop", 0, 0), ("swap_h", None, None)], ks=ks)
        for m, per in mv.items():
            sinks = ~T.source_mask(plan[0])
            assert np.all(per[0][0][:, sinks & (ks_of != ks)] == 0.0) and np.all(per[0][1][:, sinks & (ks_of != ks)] == 0.0)
            assert np.all(per[0][0][:, sinks & (ks_of == ks)].max(0) > 0.0)
