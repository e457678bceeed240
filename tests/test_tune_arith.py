"""The arithmetic behind the bit-exact tuner tests (tests/test_gpu_tuner_exact.py), checked in numpy (CPU): on the families of
tests/tunedata.py, k_tune's six term products accumulated in fp32 give the true autocorrelation at lags 1 .. tmax + 1 bit for bit in
either order, and a kernel that drops any one of them, reads a low term's plane one frame early or late, or splits the window into two
bf16 terms instead of three, does not. Also: the pick cases sit on the edges they state.

The emulation follows the kernel (aidax_tune.hip). Per K step of 32 frames at j0 and lag t = i + 16 nn + 256 tile, one MFMA sums the 32
products a[j0 + k - i] b[j0 + k - i + t] of one pair of terms (exact here in fp64, rounded once to fp32) onto the wave's fp32 accumulator;
wave w takes the steps w, w + 4, .., each with the products in the kernel's order (a0 a1 a2) b0, (a0 a1) b1, a0 b2; the four waves'
partial sums are added in wave order. The reversed order (a wave's last step first, the products backwards) must give the same bits."""
import numpy as np
import pytest

from tests import tunedata, tunehelp as th
from tests.test_split_arith import split3
from tests.tunedata import DROPPED, EXERCISES, KEPT

CONFIGS = [("A", 1024, 511), ("B", 1024, 511), ("C", 1024, 511), ("C", 2048, 1023)]
IDS = [f"{f}-{W}" for f, W, _ in CONFIGS]


def _terms(x, n=3):
    """the kernel's three bf16 terms of the windows; n = 2: a two-term split (the third term lost)"""
    t = list(split3(x))
    for k in range(n, 3):
        t[k] = np.zeros_like(t[k])
    return t


def _shift(plane, by):
    """the plane read `by` frames late (by = 1: frame j gives what frame j - 1 holds) or early (by = -1)"""
    out = np.zeros_like(plane)
    if by > 0:
        out[:, by:] = plane[:, :-by]
    else:
        out[:, :by] = plane[:, -by:]
    return out


def step_sums(a, b, tmax):
    """[step][stream][lag]: the 32-product sums of one pair of term planes a (the earlier frames), b (the later ones), in fp64"""
    S, W = a.shape
    T = tmax + 2
    if not a.any() or not b.any():
        return np.zeros((W // 32, S, T))
    lo, hi = 16, T + 32
    A = np.zeros((S, lo + W + hi))
    B = np.zeros((S, lo + W + hi))
    A[:, lo:lo + W], B[:, lo:lo + W] = a, b
    t = np.arange(T)
    k = np.arange(32)
    out = np.zeros((W // 32, S, T))
    for st in range(W // 32):
        P = 32 * st - (t % 16)[:, None] + k[None, :] + lo                 # frames j0 + k - i, zeros outside the window
        seg = A[:, P]
        live = np.flatnonzero(seg.any(axis=(1, 2)))                       # (sparse windows: most streams have nothing in a step)
        if live.size:
            out[st, live] = np.einsum("stk,stk->st", seg[live], B[live][:, P + t[:, None]])
    return out


def emulate(sums, products=KEPT, reverse=False):
    """sums: {(term of a, term of b): step_sums}; the kernel's fp32 accumulation of `products`: [stream][lag] float32"""
    steps = next(iter(sums.values())).shape[0]
    order = list(products)[::-1] if reverse else list(products)
    part = []
    for w in range(4):
        acc = np.zeros(next(iter(sums.values())).shape[1:], np.float32)
        mine = list(range(w, steps, 4))
        for st in (mine[::-1] if reverse else mine):
            for p in order:
                acc = (acc + sums[p][st].astype(np.float32)).astype(np.float32)
        part.append(acc)
    r = part[0]
    for w in (1, 2, 3):
        r = (r + part[w]).astype(np.float32)
    return r


_DATA = {}


def _data(cfg):
    """(the family, the truth at lags 1 .. tmax + 1 as float32, the step sums of all nine term products)"""
    if cfg not in _DATA:
        f, W, tmax = cfg
        fam = tunedata.family(f, W, tmax)
        ts = _terms(fam["x"])
        sums = {(i, j): step_sums(ts[i], ts[j], tmax) for i in range(3) for j in range(3)}
        _DATA[cfg] = fam, fam["r"][:, 1:].astype(np.float32), sums
    return _DATA[cfg]


def _every_lag_changes(got, truth, what, allow=0):
    """a mutant must show on every lag, in some stream: no lag of the GPU comparison is blind to it (but for `allow` of them)"""
    blind = np.flatnonzero(~(got[:, 1:] != truth).any(axis=0)) + 1
    assert blind.size <= allow, (what, "lags that do not see it", blind[:16])


@pytest.mark.parametrize("cfg", CONFIGS, ids=IDS)
def test_truth_is_the_fp64_autocorrelation(cfg):
    fam, truth, _ = _data(cfg)
    assert fam["x"].shape[0] <= 64 and fam["x"].shape[1] == cfg[1]
    for s, x in enumerate(fam["x"]):
        r = th.autocorr(x, cfg[2])
        assert np.array_equal(r[1:], fam["r"][s, 1:]) and r[0] == fam["r"][s, 0], s
    assert np.array_equal(truth.astype(np.float64), fam["r"][:, 1:])
    assert (np.count_nonzero(truth, axis=0) > 0).all(), "a lag without a product"
    print(f"{cfg}: {fam['x'].shape[0]} streams")


@pytest.mark.parametrize("cfg", CONFIGS, ids=IDS)
def test_six_products_in_fp32_are_exact_in_either_order(cfg):
    _, truth, sums = _data(cfg)
    assert np.array_equal(emulate(sums)[:, 1:], truth)
    assert np.array_equal(emulate(sums, reverse=True)[:, 1:], truth)


@pytest.mark.parametrize("cfg", CONFIGS, ids=IDS)
def test_the_dropped_products_are_zero_and_the_claimed_ones_are_on_every_lag(cfg):
    fam, _, sums = _data(cfg)
    for p in DROPPED:
        assert not sums[p][:, :, 1:].any(), p
    for p in EXERCISES[cfg[0]]:
        live = np.abs(sums[p]).sum(axis=0) > 0                            # [stream][lag]
        for s, cover in enumerate(fam["covers"]):
            assert live[s, sorted(cover)].all(), (p, s)
        assert live[:, 1:].any(axis=0).all(), p


@pytest.mark.parametrize("cfg", CONFIGS[:3], ids=IDS[:3])
def test_a_missing_or_misplaced_product_changes_bits(cfg):
    """what the bit-exact GPU tests would see from a kernel that lost one product, read a plane of term 1 or 2 one frame off (as either
    operand), or split the window in two terms"""
    f, W, tmax = cfg
    fam, truth, sums = _data(cfg)
    for p in EXERCISES[f]:
        _every_lag_changes(emulate(sums, [q for q in KEPT if q != p]), truth, ("dropped", p))
    ts = _terms(fam["x"])
    low = sorted({(side, p[side]) for p in EXERCISES[f] for side in (0, 1) if p[side] > 0})
    assert low
    # A plane read one frame off moves a product to the next lag. A lag can miss that only where the frame next to the pair's other mark
    # holds a mark that gives the same product: the distances of a stream's marks are all different, so it has at most one pair of
    # neighbours (distance 1), which stands in one pair of lags per other mark: one mark in A and B (the rich one), N_MARKS - 2 in C
    allow = fam["x"].shape[0] * (1 if f in "AB" else tunedata.N_MARKS - 2)
    assert allow < (tmax + 1) // 4
    for side, term in low:
        for by in (-1, 1):
            moved = dict(sums)
            plane = _shift(ts[term], by)
            for p in KEPT:
                if p[side] == term:
                    moved[p] = step_sums(plane, ts[p[1]], tmax) if side == 0 else step_sums(ts[p[0]], plane, tmax)
            _every_lag_changes(emulate(moved), truth, ("operand", side, "term", term, "read off by", by), allow)
    if f in "AB":
        t2 = _terms(fam["x"], 2)
        two = {p: step_sums(t2[p[0]], t2[p[1]], tmax) if 2 in p else sums[p] for p in KEPT}
        _every_lag_changes(emulate(two), truth, "two-term split")


def test_the_families_claim_every_kept_product():
    assert set(KEPT) == set().union(*EXERCISES.values())
    assert not set(DROPPED) & set(KEPT) and len(set(KEPT) | set(DROPPED)) == 9
    # the kernel's order: b's term outermost, a's terms 0 .. 2 - b's
    assert list(KEPT) == [(tw, th_) for th_ in range(3) for tw in range(3 - th_)]


def test_the_rich_marks_keep_their_distance():
    for f in "AB":
        fam = tunedata.family(f)
        for s, marks in enumerate(fam["marks"]):
            ts = split3(fam["x"][s])
            rich = [q for q in marks if ts[1][q] != 0 or ts[2][q] != 0]
            assert rich == [fam["rich"][s]] and ts[2][rich[0]] != 0
    fam = tunedata.family("C")
    ts = split3(fam["x"])
    assert not ts[2].any() and ((ts[1] != 0) == (fam["x"] != 0)).all()


@pytest.mark.parametrize("name", list(tunedata.PICK_CASES))
def test_pick_cases_sit_on_their_edges(name):
    tunedata.check_case(tunedata.PICK_CASES[name])


def test_pick_designs():
    want = {"std": (4, 0.93, 0.0), "half": (4, 0.5, 0.0), "one": (4, 1.0, 0.0), "tmin2": (2, 0.93, 0.0), "gates": (4, 0.93, 0.5)}
    for name, (tmin, k, cl) in want.items():
        rec = th.design(tunedata.SR, **tunedata.pick_design(name))
        assert (rec["tmin"], rec["tmax"], rec["threshold"], rec["clarity_min"]) == (tmin, 299, np.float32(k), np.float32(cl))
        assert tunedata.cases_of(name)
    assert th.design(tunedata.SR, **tunedata.pick_design("gates"))["level_min"] == np.float32(0.1)
