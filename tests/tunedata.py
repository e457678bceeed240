"""Windows on which the stream tuners (k_tune, aidax_tune.hip) must be exact to the last bit: sparse windows that reach the low bf16 terms
of the autocorrelation, and windows of integers / 8 that sit on the edges of the peak pick (rules 5 and 6 of include/aidax.h, "Stream
tuners"). Every claim made here is asserted here, on the CPU; tests/test_tune_arith.py runs the assertions and the emulation of the
kernel's arithmetic, tests/test_gpu_tuner_exact.py holds the kernel to these windows.

A window is a few non-zero frames, its MARKS. For a pair (x[a], x[a + t]) the earlier frame is the kernel's A operand and the later one
its B operand; it keeps the term products (a0 a1 a2) b0, (a0 a1) b1, a0 b2. A RICH value is an odd mantissa of the stated number of bits
times a power of two, of magnitude in [1/8, 1); a PLAIN value is +-2^k, k in [-3, 0].

    family  window                                                                      term products that carry bits
    A       one rich mark of 22 bits, all three of its terms non-zero, up to 14 plain    a0 b0, a1 b0, a2 b0
            marks behind it (later), none farther than tmax + 1
    B       the same with the plain marks ahead of the rich one                           a0 b0, a0 b1, a0 b2
    C       up to 15 rich marks of 11 bits: a non-zero second term, no third one          a0 b0, a1 b0, a0 b1, a1 b1

In every window the distances of the marks that are at most tmax + 1 apart are all different, so a lag 1 .. tmax + 1 carries at most one
product: 22 bits by a power of two, or 11 bits by 11 bits — an fp32 number, like every partial sum of its term products. A and B hold one
rich mark, so the three dropped products (a1 b2, a2 b1, a2 b2) are zero on every lag but lag 0, which is the sum of the squares (not an
fp32 number: outside the bit comparison). Every frame is a multiple of 2^-24 and the squares of a window add up to less than 2^5, so any
partial sum of the squares, in any order, is exact in fp64: m[t] is exact and the NSDF at lags 1 .. tmax + 1 is ONE correctly rounded
value. A family is a set of streams drawn greedily until every lag 1 .. tmax + 1 has a rich-by-plain (C: rich-by-rich) product in some
stream: both copies of a plane, every row and column of the fragment and every lag tile are reached, and the rich mark's position varies
over the streams (the K step, the position inside it and the wave vary with it).

The pick cases (PICK_CASES) are windows of integers / 8 with W = 1024 and tmax = 299 whose marks all lie in [tmax + 1, W - tmax - 1): then
m[t] = 2 c[W] for every lag, so equal r[t] give equal NSDF bits. tests/tunehelp.py's analyse(exact=True) is their reference, and every case
states its key maxima, its chosen lag and the edge it sits on; check_case() holds the restatement to them."""
import functools
import math

import numpy as np

from tests import tunehelp as th
from tests.test_split_arith import split3

F32 = np.float32
SR = 48000.0
# the kernel's six term products as (term of A: the earlier frame, term of B: the later frame), in the order it issues them per step
KEPT = ((0, 0), (1, 0), (2, 0), (0, 1), (1, 1), (0, 2))
DROPPED = ((2, 1), (1, 2), (2, 2))
EXERCISES = {"A": ((0, 0), (1, 0), (2, 0)),
             "B": ((0, 0), (0, 1), (0, 2)),
             "C": ((0, 0), (1, 0), (0, 1), (1, 1))}
N_MARKS = 15
MAX_STREAMS = 64


def f_min_for(tmax):
    """an f_min whose design has this tmax at 48 kHz"""
    return SR / (tmax - 0.5)


def _rich(rng, bits):
    """+-m 2^(e - bits), m odd of exactly `bits` bits, e in [-2, 0]: redrawn until the split has the terms the family claims"""
    want = (True, True, True) if bits == 22 else (True, True, False)
    while True:
        m = 2 * int(rng.integers(1 << (bits - 2), 1 << (bits - 1))) + 1
        v = F32(math.ldexp(-m if rng.random() < 0.5 else m, int(rng.integers(-2, 1)) - bits))
        if tuple(bool(t[0] != 0) for t in split3(np.array([v]))) == want:
            return v


def _plain(rng):
    return F32(math.ldexp(-1.0 if rng.random() < 0.5 else 1.0, int(rng.integers(-3, 1))))


def _draw_marks(rng, fam, W, last, unc):
    """one stream's marks, drawn greedily: (positions, the rich mark's position or None). unc[t]: no stream covers lag t yet; cleared here"""
    t = int(rng.choice(np.flatnonzero(unc)))
    if fam == "C":
        a = int(rng.integers(0, W - t))
    else:
        # the rich mark: half of the draws leave room for every lag on its plain side, the other half go anywhere the first pair fits
        lo, hi = (0, W - 1 - t) if fam == "A" else (t, W - 1)
        if rng.random() < 0.5:
            lo, hi = (lo, min(hi, W - 1 - last)) if fam == "A" else (max(lo, last), hi)
        rich = int(rng.integers(lo, hi + 1))
        a = rich if fam == "A" else rich - t
    marks = [a, a + t]
    rich = None if fam == "C" else (a if fam == "A" else a + t)
    used = np.zeros(W, bool)                                              # distances (<= last) between two marks of this stream
    used[0] = used[t] = True
    unc[t] = False
    p = np.arange(W)
    while len(marks) < N_MARKS:
        d = np.abs(p[:, None] - np.array(marks)[None, :])                 # [candidate][mark]
        near = d <= last
        ds = np.sort(np.where(near, d, W + np.arange(len(marks))[None, :]), axis=1)
        ok = ~(used[d] & near).any(axis=1) & ~(ds[:, 1:] == ds[:, :-1]).any(axis=1)
        if fam == "C":
            gain = (unc[np.minimum(d, last)] & near).sum(axis=1)
        else:
            side = p - rich if fam == "A" else rich - p
            ok &= (side >= 1) & (side <= last)
            gain = unc[np.clip(side, 0, last)].astype(np.int64)
        gain = np.where(ok, gain, -1)
        if gain.max() <= 0:
            break
        q = int(rng.choice(np.flatnonzero(gain == gain.max())))
        for m in marks:
            dd = abs(q - m)
            if dd <= last:
                used[dd] = True
                if fam == "C" or m == rich:
                    unc[dd] = False
        marks.append(q)
    return sorted(marks), rich


@functools.lru_cache(maxsize=None)
def family(fam, W=1024, tmax=511, seed=0, streams=None):
    """the streams of a family: a dict with x [S][W] float32, marks (per stream, ascending), rich (per stream: the rich mark's position,
    None in C), covers (per stream: the lags its rich products fall on) and r [S][tmax + 2] float64, the exact autocorrelation.
    streams=None draws until every lag 1 .. tmax + 1 is covered (at most MAX_STREAMS); streams=n stops after n."""
    assert fam in EXERCISES
    rng = np.random.default_rng([ord(fam), W, tmax, seed])
    last = tmax + 1
    unc = np.zeros(last + 1, bool)
    unc[1:] = True
    xs, all_marks, riches, covers, rs = [], [], [], [], []
    while unc.any() and (streams is None or len(xs) < streams):
        marks, rich = _draw_marks(rng, fam, W, last, unc)
        x = np.zeros(W, np.float32)
        for q in marks:
            x[q] = _rich(rng, 11) if fam == "C" else _rich(rng, 22) if q == rich else _plain(rng)
        # r from the pairs: at most one per lag, each one exact product
        r = np.zeros(last + 1)
        r[0] = math.fsum(float(x[q]) ** 2 for q in marks)
        count = np.zeros(last + 1, np.int64)
        cover = set()
        for i, qa in enumerate(marks):
            for qb in marks[i + 1:]:
                t = qb - qa
                if t > last:
                    continue
                count[t] += 1
                r[t] = float(x[qa]) * float(x[qb])
                if fam == "C" or rich in (qa, qb):
                    cover.add(t)
        assert count.max() == 1, "two pairs of marks on one lag"
        assert np.array_equal(r[1:].astype(np.float32).astype(np.float64), r[1:]), "a lag that is no fp32 number"
        if fam != "C":
            assert all((q > rich) == (fam == "A") for q in marks if q != rich) and all(abs(q - rich) <= last for q in marks)
        # every partial sum of the squares, in any order: multiples of 2^-48 that stay below 2^53 of them
        xi = [int(float(x[q]) * 2.0 ** 24) for q in marks]
        assert all(v * 2.0 ** -24 == float(x[q]) for v, q in zip(xi, marks)) and sum(v * v for v in xi) < 1 << 53
        assert r[0] == sum(v * v for v in xi) * 2.0 ** -48
        xs.append(x)
        all_marks.append(tuple(marks))
        riches.append(rich)
        covers.append(frozenset(cover))
        rs.append(r)
    S = len(xs)
    assert S <= MAX_STREAMS, S
    if streams is None:
        covered = set().union(*covers)
        assert covered == set(range(1, last + 1)), sorted(set(range(1, last + 1)) - covered)
        if fam != "C":                                                    # the rich mark moves: every wave's steps, most positions in a step
            assert len({(q // 32) % 4 for q in riches}) == 4 and len({q % 32 for q in riches}) >= 12
    return dict(fam=fam, W=W, tmax=tmax, x=np.array(xs), marks=all_marks, rich=riches, covers=covers, r=np.array(rs))


# ---------------------------------------------------------------------------------------------------------------------------------------
# the pick's edges

PICK_W, PICK_TMAX = 1024, 299
PICK_LO, PICK_HI = PICK_TMAX + 1, PICK_W - PICK_TMAX - 1                   # marks in [PICK_LO, PICK_HI): m[t] = 2 c[W] on every lag
# one pool per design; clarity_min = 0 except where the gates are the subject, so that a reading shows the lag the pick chose
DESIGNS = {
    "std": dict(clarity_min=0.0),
    "half": dict(clarity_min=0.0, threshold=0.5),
    "one": dict(clarity_min=0.0, threshold=1.0),
    "tmin2": dict(clarity_min=0.0, f_max=24000.0),
    "gates": dict(clarity_min=0.5, level_min_db=-20.0),
}


def pick_design(name):
    """the keyword arguments of a pick design (tunehelp.design and the binding's tuner_params take the same)"""
    kw = dict(window=PICK_W, hop=PICK_W, f_min=f_min_for(PICK_TMAX), f_max=12000.0)
    kw.update(DESIGNS[name])
    return kw


def _bits(v):
    return np.asarray(v, np.float32).view(np.uint32)


def _window(marks):
    """{position: integer}: the window of integers / 8, every mark where m[t] does not depend on t"""
    x = np.zeros(PICK_W, np.float32)
    for q, v in marks.items():
        assert PICK_LO <= q < PICK_HI and v == int(v), (q, v)
        x[q] = v / 8.0
    return x


PICK_CASES = {}


def _case(name, design, marks, keys, choice, edge, lag=None, x=None):
    """keys: the key maxima in lag order; choice: the lag rules 5 and 6 choose (0: none); lag: the reading's (choice unless a gate of
    rule 8 closes); edge(n, rec, rd): asserts, on the restatement's row and reading, that the window sits on its edge"""
    assert name not in PICK_CASES
    PICK_CASES[name] = dict(name=name, design=design, x=_window(marks) if x is None else x, keys=list(keys), choice=choice,
                            lag=choice if lag is None else lag, edge=edge, flat=x is None)


def _eq(n, a, b):
    return _bits(n[a]) == _bits(n[b])


def _edge_equal_keys(n, rec, rd):
    assert _eq(n, 130, 260) and n[130] > 0


def _edge_small_in_front(n, rec, rd):
    assert _eq(n, 130, 260) and 0 < n[50] < rec["threshold"] * n[130] and 0 < n[180] < n[50]


def _edge_lobe_tie(n, rec, rd):
    assert _eq(n, 100, 102) and _bits(n[101]) == _bits(n[100] / F32(2)) and not n[99] > 0 and not n[103] > 0


def _edge_plateau(n, rec, rd):
    assert _eq(n, 99, 100) and n[100] > n[101] and not n[98] > 0


def _edge_at_the_bar(n, rec, rd):
    assert rec["threshold"] == F32(0.5) and _bits(F32(0.5) * n[250]) == _bits(n[100]) and n[150] < n[100]


def _edge_under_the_bar(n, rec, rd):
    assert rec["threshold"] == F32(0.5) and _bits(F32(0.25) * n[250]) == _bits(n[100]) and n[150] < n[100]


def _edge_threshold_one(n, rec, rd):
    assert rec["threshold"] == F32(1.0) and _eq(n, 130, 260) and 0 < n[50] < n[130]


_EQUAL = {300: 16, 430: 8, 560: 16}                                        # r[130] = 16 8 + 8 16 = r[260] = 16 16
_case("equal_keys", "std", _EQUAL, [130, 260], 130, _edge_equal_keys)
_case("equal_keys_small_in_front", "std", {**_EQUAL, 610: 1}, [50, 130, 180, 260], 130, _edge_small_in_front)
_case("lobe_tie_v_half_v", "std", {300: 8, 400: 2, 401: 1, 402: 2}, [100], 100, _edge_lobe_tie)
_case("plateau", "std", {300: 8, 399: 2, 400: 2}, [100], 100, _edge_plateau)
_case("key_at_the_bar", "half", {300: 8, 400: 1, 550: 2}, [100, 150, 250], 100, _edge_at_the_bar)
_case("key_under_the_bar", "half", {300: 8, 400: 1, 550: 4}, [100, 150, 250], 250, _edge_under_the_bar)
_case("threshold_one", "one", {**_EQUAL, 610: 1}, [50, 130, 180, 260], 130, _edge_threshold_one)


def _straddles():
    """lobes of two and three lags over the chunk edges 63|64 and 127|128 and the tile edge 255|256, the maximum on either side"""
    for e in (64, 128, 256):
        for tag, first, vals in (("two_max_below", e - 1, (2, 1)), ("two_max_above", e - 1, (1, 2)),
                                 ("three_up_to_edge", e - 2, (1, 2, 3)), ("three_down_to_edge", e - 2, (3, 2, 1)),
                                 ("three_up_from_edge", e - 1, (1, 2, 3)), ("three_down_from_edge", e - 1, (3, 2, 1)),
                                 ("three_max_on_edge", e - 1, (1, 3, 1))):
            key = first + int(np.argmax(vals))
            marks = {300: 8, **{300 + first + k: v for k, v in enumerate(vals)}}

            def edge(n, rec, rd, first=first, vals=vals, e=e):
                lobe = n[first:first + len(vals)]
                assert not n[first - 1] > 0 and not n[first + len(vals)] > 0 and (lobe > 0).all() and first < e <= first + len(vals) - 1
                assert all(np.sign(float(lobe[i]) - float(lobe[j])) == np.sign(vals[i] - vals[j]) for i in range(len(vals)) for j in range(i))
            _case(f"straddle_{e}_{tag}", "std", marks, [key], key, edge)


_straddles()


def _edge_wide(n, rec, rd):
    assert (n[120:201] > 0).all() and not (n[81:120] > 0).any() and not n[201] > 0          # chunk 128 .. 191 lies inside the lobe
    assert (_bits(n[120:200]) == _bits(n[120])).all() and n[200] > n[199]


def _edge_wide_tie(n, rec, rd):
    assert (n[120:201] > 0).all() and not (n[81:120] > 0).any() and not n[201] > 0
    assert _eq(n, 125, 200) and n[125] > n[124] and n[125] > n[126]


_RUN = {300: 8, **{300 + t: 1 for t in range(120, 200)}, 500: 2}
_case("wide_lobe_max_in_last_chunk", "std", _RUN, [200], 200, _edge_wide)
_case("wide_lobe_tie_across_chunks", "std", {**_RUN, 425: 2}, [125], 125, _edge_wide_tie)


def _edge_tmin2(n, rec, rd):
    assert rec["tmin"] == 2 and not n[1] > 0 and n[2] > 0 and not n[3] > 0


def _edge_below_tmin(n, rec, rd):
    assert rec["tmin"] == 4 and not n[1] > 0 and n[3] > n[20] > n[40] > 0 and rec["threshold"] * n[3] > n[20]


def _edge_at_tmax(n, rec, rd):
    assert rec["tmax"] == 299 and n[299] > 0 and not n[298] > 0 and not n[300] > 0


def _edge_past_tmax(n, rec, rd):
    assert n[300] > n[299] > 0 and not n[298] > 0 and not (n[3:298] > 0).any() and rd["clarity"] == 0


def _edge_open_end(n, rec, rd):
    assert (n[295:301] > 0).all() and not n[294] > 0 and n[297] > n[296] and n[297] > n[298]


def _edge_constant(n, rec, rd):
    assert (_bits(n[1:]) == _bits(F32(1.0))).all() and rd["clarity"] == 0 and rd["level"] == F32(1.0)


_case("tmin_two", "tmin2", {300: 8, 302: 8}, [2], 2, _edge_tmin2)
_case("peak_below_tmin", "std", {300: 64, 303: 64, 660: 2, 680: 8, 700: 16}, [20, 40], 20, _edge_below_tmin)
_case("key_at_tmax", "std", {300: 8, 599: 8}, [299], 299, _edge_at_tmax)
_case("only_maximum_past_tmax", "std", {300: 8, 599: 1, 600: 2}, [], 0, _edge_past_tmax)
_case("lobe_open_at_the_end", "std", {300: 8, 595: 1, 596: 2, 597: 3, 598: 2, 599: 1, 600: 1}, [297], 297, _edge_open_end)
_case("constant_window", "std", None, [], 0, _edge_constant, x=np.ones(PICK_W, np.float32))


def _edge_clarity_equal(n, rec, rd):
    assert _bits(rd["clarity"]) == _bits(rec["clarity_min"]) == _bits(F32(0.5)) and not rd["level"] < rec["level_min"]


def _edge_clarity_under(n, rec, rd):
    assert 0 < rd["clarity"] < rec["clarity_min"] and not rd["level"] < rec["level_min"] and rd["hz"] == 0 and rd["period"] == 0


def _edge_level_under(n, rec, rd):
    assert 0 < rd["level"] < rec["level_min"] and _bits(rd["clarity"]) == _bits(F32(0.5)) and rd["hz"] == 0 and rd["period"] == 0


_case("clarity_at_the_floor", "gates", {300: 32, 400: 32}, [100], 100, _edge_clarity_equal)
_case("clarity_under_the_floor", "gates", {300: 28, 400: 32}, [100], 100, _edge_clarity_under, lag=0)
_case("level_under_the_floor", "gates", {300: 8, 400: 8}, [100], 100, _edge_level_under, lag=0)


def check_case(case):
    """hold the restatement to what the case states; returns (the reading, the NSDF row)"""
    rec = th.design(SR, **pick_design(case["design"]))
    assert rec is not None and (rec["window"], rec["tmax"]) == (PICK_W, PICK_TMAX)
    rd, n = th.analyse(case["x"], rec, exact=True)
    q, keys = th.pick(n, rec["tmin"], rec["tmax"], rec["threshold"])
    assert keys == case["keys"], (case["name"], keys)
    assert q == case["choice"], (case["name"], q)
    assert rd["lag"] == case["lag"], (case["name"], rd)
    if case["flat"]:                                                      # equal r, equal bits
        xs = case["x"].astype(np.float64)
        c = np.concatenate([[0.0], np.cumsum(xs * xs)])
        t = np.arange(PICK_TMAX + 2)
        assert (c[PICK_W - t] + (c[PICK_W] - c[t]) == 2.0 * c[PICK_W]).all()
    case["edge"](n, rec, rd)
    return rd, n


def cases_of(design):
    return [c for c in PICK_CASES.values() if c["design"] == design]
