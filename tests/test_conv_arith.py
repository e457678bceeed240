"""The arithmetic behind the bit-exact conv tests (tests/test_gpu_conv_exact.py), checked in numpy and against the C oracle (CPU): on the
stacks of tests/convdata.py

  * layer 0 quantises: from the oracle's own pre-chain output — the warm-up's silence and the signal's stretches of zeros included — every
    pre-activation of layer 0 lies at least MARGIN = 127 from zero (nominally 128), where tanh and sigmoid are +-1 and 1 / 0 to the bit;
  * the oracle's network gives convdata.truth bit for bit, warmed up (what a pool runs) and from reset state on grid inputs (what
    Model.forward runs), on every stack and family;
  * on the mixed families the three dropped term products are zero at every layer, the products a family claims (convdata.EXERCISES) are
    non-zero at every tap of every layer, and every sum a kernel can form stays inside fp32's 24 bits (convdata.budget);
  * a numpy emulation of the kernels' accumulation — per layer >= 1, tap, kept term product and half of the input channels one
    MFMA-sized sum, rounded to fp32 and added to an fp32 accumulator, in the kernels' order or in a shuffled one, the bias first or last —
    gives the truth bit for bit; and knocking out, doubling or swapping any single kept product at any single (layer >= 1, tap) changes
    output bits;
  * on the all-tanh family a tap that reads one frame off, at any (layer, tap), flips output signs.

Swapping a product (i, j) means w_j x_i in its place — for the diagonal products (0, 0) and (1, 1), whose swap is themselves, the product
taken at the neighbouring tap's delay instead."""
import numpy as np
import pytest

from oracle import oracle as O
from tests import convdata as cd
from tests.convdata import DROPPED, EXERCISES, EXERCISES_L1, KEPT, split3

S, T = 2, 700
CASES = [(st, f) for st in cd.STACKS for f in cd.FAMILIES]
MIXED_CASES = [(st, f) for st in cd.STACKS for f in cd.MIXED]
_DATA = {}
_PADDED = {}


def _data(stack, family):
    if (stack, family) not in _DATA:
        j, meta = cd.make_stack(stack, family)
        xg = cd.pre_chain(cd.signal(S, T, seed=11))
        y, acts = cd.truth(j, xg)
        # the same run with the warm-up's silence in it, from reset state: what the emulation below works on (every history inside the run)
        pad = cd.receptive_field(j)
        yp, actsp = cd.truth(j, np.concatenate([np.zeros((S, pad), np.float32), xg], axis=1), warm=False)
        assert np.array_equal(yp[:, pad:], y)
        _DATA[stack, family] = (j, meta, xg, y, acts)
        _PADDED[stack, family] = (yp, actsp)
    return _DATA[stack, family]


def test_the_pre_chain_emulation_is_the_plugins():
    """a plugin without a model under the exact tests' controls: out = (x * pre gain) * master gain, operation for operation"""
    x = cd.signal(1, 600, seed=5)[0]
    g, master = cd.gain_ramps(x.size)
    pl = O.OraclePlugin()
    pl.set_loading(False)
    got = pl.run(O.default_controls(in_lpf_pc=0.0, dc_blocker=0.0, eq_bypass=1.0), x)
    assert np.array_equal(got, cd.pre_chain(x)[0] * master)
    assert np.all(np.abs(g.astype(np.float64) - 1.0) <= 2.0 ** -22)


@pytest.mark.parametrize("stack,family", CASES)
def test_layer_0_quantises_with_margin(stack, family):
    j, meta, xg, y, acts = _data(stack, family)
    assert np.count_nonzero(xg == 0.0) >= S * 300 and np.count_nonzero(xg) >= S * T // 3       # silence and signal
    pad = cd.receptive_field(j)                                                                # (the warm-up's zeros in front)
    a = np.concatenate([np.zeros((S, pad)), xg.astype(np.float64)], axis=1)[:, None, :]
    z = cd.preactivation(j["layers"][0], a)
    assert np.abs(z).min() >= cd.MARGIN, np.abs(z).min()
    nominal = cd.preactivation(j["layers"][0], np.round(a / cd.LEVEL) * cd.LEVEL)
    assert np.abs(nominal).min() == cd.MARGIN_NOMINAL
    codes = acts[0]
    assert set(np.unique(codes)) == ({0.0, 1.0} if family == "T2" else {-1.0, 1.0})
    # fp32's own tanh / logistic function at the margin: the values the kernels must return to the bit
    m = np.float32(cd.MARGIN)
    assert np.tanh(m) == 1.0 and np.tanh(-m) == -1.0
    with np.errstate(over="ignore"):
        assert np.float32(1) / (np.float32(1) + np.exp(-m)) == 1.0 and np.float32(1) / (np.float32(1) + np.exp(m)) == 0.0


@pytest.mark.parametrize("stack,family", CASES)
def test_the_oracles_network_is_the_truth(stack, family):
    j, meta, xg, y, acts = _data(stack, family)
    spec = O.parse_model(j)
    assert spec.input_gain == 1.0 and spec.output_gain == 1.0 and spec.input_skip == 0
    for s in range(S):
        got = O.OracleModel(spec).apply(xg[s])                       # (warmed up, as a pool's model is)
        assert np.array_equal(got, y[s]), (s, np.count_nonzero(got != y[s]))
    assert np.unique(y).size >= 20


@pytest.mark.parametrize("stack", cd.STACKS)
def test_the_oracles_network_is_the_truth_from_reset_state_on_grid_inputs(stack):
    """the bare-model runs: layer 0 linear with one tap of +-1 per channel, inputs in {-1, 0, 1}, no quantiser"""
    j, meta = cd.make_stack(stack, "T3", quantiser=False)
    x = cd.grid_signal(500, seed=3)
    y, acts = cd.truth(j, x, warm=False)
    assert np.array_equal(O.net_run(O.parse_model(j), x), y[0])
    assert max(cd.budget(j, acts)) < 24.0


@pytest.mark.parametrize("stack,family", MIXED_CASES)
def test_budget_dropped_products_and_exercised_products(stack, family):
    j, meta, xg, y, acts = _data(stack, family)
    assert max(cd.budget(j, acts)) < 24.0, cd.budget(j, acts)
    for l in range(1, len(j["layers"]) - 1):
        w, b, k, dil, act = cd.layer_params(j["layers"][l])
        assert act == ("relu" if l % 2 else "")
        live = cd.term_activity(j, acts, l)
        for p in DROPPED:
            assert not any(live[p]), (l, p)
        claimed = EXERCISES_L1[family] if l == 1 else EXERCISES[family]
        for p in KEPT:
            if p in claimed:
                assert all(live[p]), (l, p, live[p])
            elif l == 1:
                assert not any(live[p]), (l, p)                      # layer 1 reads one-term codes
    assert cd.claims_hold(j, family, acts)


PLANE = 128          # frames of history k_conv_ms's activation plane holds (aidax_layout.h: kConvsHist); a tap further back is read from HBM


@pytest.mark.parametrize("stack", cd.MS_STACKS + ("StGeoA",))
def test_the_taps_beyond_the_plane_carry_all_six_products(stack):
    """the corners' deep layer (and StGeoA's last) sits behind a layer with multi-term outputs: between the two mixed families every kept
    product is non-zero at every tap that reaches beyond the plane — the packed k-step's (three taps), the plain k-step's one deep tap
    (two taps) and its two deep taps with per-lane sources (four taps at dilation 85)"""
    deep = [(l, tap) for l, (k, dil) in enumerate(cd.STACKS[stack][1]) if l >= 1 for tap in range(k) if (k - 1 - tap) * dil > PLANE]
    assert deep and all(l >= 2 for l, _ in deep), deep
    if stack == "four taps, two deep taps in one k-step":
        assert sorted((4 - 1 - tap) * 85 for _, tap in deep) == [170, 255]
    seen = {d: set() for d in deep}
    for family in cd.MIXED:
        j, meta, xg, y, acts = _data(stack, family)
        for l, tap in deep:
            live = cd.term_activity(j, acts, l)
            seen[l, tap] |= {p for p in KEPT if live[p][tap]}
            assert not any(live[p][tap] for p in DROPPED)
    for d in deep:
        assert seen[d] == set(KEPT), (d, seen[d])


def emulate_layer(layer, a, order=None, bias_last=False, mutate=None):
    """One layer >= 1 as k_conv_ms / k_conv_st accumulate it (see the module's docstring) on the activations a[s][c][t] below -> its
    activations, float64 holding float32 values. order: a permutation of the granules (tap, product, channel half); mutate = (tap,
    product, "drop" | "double" | "swap")."""
    w, b, k, dil, act = cd.layer_params(layer)
    ws = [t.astype(np.float64) for t in split3(w.astype(np.float32))]
    xs = [t.astype(np.float64) for t in split3(a.astype(np.float32))]
    Cin = w.shape[1]
    halves = [slice(0, 8), slice(8, Cin)] if Cin > 8 else [slice(0, Cin)]
    granules = []
    for tap in range(k):
        for p in KEPT:
            reps, q, back = 1, p, (k - 1 - tap) * dil
            if mutate is not None and mutate[0] == tap and mutate[1] == p:
                if mutate[2] == "drop":
                    reps = 0
                elif mutate[2] == "double":
                    reps = 2
                elif p[0] != p[1]:
                    q = (p[1], p[0])
                else:
                    back = (k - 1 - (tap + 1) % k) * dil
            granules += [(tap, q, back, h) for h in halves] * reps
    if order is not None:
        granules = [granules[i] for i in order.permutation(len(granules))]
    acc = np.zeros((a.shape[0], w.shape[2], a.shape[2]), np.float32)
    if not bias_last:
        acc += b.astype(np.float32)[None, :, None]
    for tap, (wi, xi), back, h in granules:
        d = cd.contract(cd.shifted(xs[xi][:, h, :], back), ws[wi][tap, h, :])
        acc = (acc + d.astype(np.float32)).astype(np.float32)
    if bias_last:
        acc = (acc + b.astype(np.float32)[None, :, None]).astype(np.float32)
    return cd.activate(acc.astype(np.float64), act)


@pytest.mark.parametrize("stack,family", MIXED_CASES)
def test_six_products_in_fp32_are_the_truth_in_any_order(stack, family):
    j = _data(stack, family)[0]
    y, acts = _PADDED[stack, family]
    rng = np.random.default_rng(7)
    for order, bias_last in ((None, False), (rng, False), (rng, True)):
        a = acts[0]
        for l in range(1, len(j["layers"]) - 1):
            a = emulate_layer(j["layers"][l], a, order, bias_last)
            assert np.array_equal(a, acts[l]), (l, order is not None, bias_last)
        # the Dense layer: sixteen fp32 FMAs in any order
        d, bd = (np.asarray(v, np.float32) for v in j["layers"][-1]["weights"])
        out = np.full(y.shape, bd[0], np.float32)
        for c in (rng.permutation(d.shape[0]) if order is not None else range(d.shape[0])):
            out = (out.astype(np.float64) + d[c, 0].astype(np.float64) * a[:, c, :]).astype(np.float32)
        assert np.array_equal(out, y)


@pytest.mark.parametrize("stack,family", MIXED_CASES)
def test_a_missing_doubled_or_swapped_product_changes_output_bits(stack, family):
    """what the bit-exact GPU tests see of a kernel that loses, doubles or misplaces ONE term product at ONE tap of ONE layer: the
    mutated layer's activations through the rest of the stack (exactly) differ from the truth in the OUTPUT"""
    j = _data(stack, family)[0]
    y, acts = _PADDED[stack, family]
    fewest = 1.0
    for l in range(1, len(j["layers"]) - 1):
        k = cd.layer_params(j["layers"][l])[2]
        for tap in range(k):
            for p in (EXERCISES_L1[family] if l == 1 else EXERCISES[family]):
                for how in ("drop", "double", "swap"):
                    a = emulate_layer(j["layers"][l], acts[l - 1], mutate=(tap, p, how))
                    got = cd.forward_from(j, a, l + 1, check=False)[0].astype(np.float32)
                    changed = np.count_nonzero(got != y) / y.size
                    assert changed > 0.0, (l, tap, p, how)
                    fewest = min(fewest, changed)
    assert fewest >= 0.01, fewest


@pytest.mark.parametrize("stack", cd.STACKS)
def test_a_tap_one_frame_off_flips_signs_of_the_all_tanh_family(stack):
    j, meta, xg, y, acts = _data(stack, "SIGN")
    for a in acts:
        assert set(np.unique(a)) == {-1.0, 1.0}
    a0 = np.concatenate([np.zeros((S, 1, cd.receptive_field(j) + 1)), xg.astype(np.float64)[:, None, :]], axis=2)
    pad = a0.shape[2] - T
    assert np.array_equal(cd.forward_from(j, a0, 0)[0][:, pad:].astype(np.float32), y)
    for l in range(1, len(j["layers"]) - 1):
        for tap in range(cd.layer_params(j["layers"][l])[2]):
            got = cd.forward_from(j, a0, 0, shift=(l, tap, 1))[0][:, pad:].astype(np.float32)
            assert np.count_nonzero(got != y) >= 0.01 * y.size, (l, tap)


def test_the_families_cover_every_kept_product():
    assert set(KEPT) == set().union(*EXERCISES.values())
    assert not set(DROPPED) & set(KEPT) and len(set(KEPT) | set(DROPPED)) == 9
    assert set(KEPT[:3]) == set().union(*EXERCISES_L1.values())
    for st in cd.ST_STACKS + cd.MS_STACKS:
        assert cd.STACKS[st][0] == 16
