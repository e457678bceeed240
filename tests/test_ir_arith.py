"""The arithmetic behind the bit-exact IR tests (tests/test_gpu_ir_exact.py), checked in numpy (CPU): on the exact-arithmetic families of
tests/irdata.py, k_ir_conv's six term products accumulated in fp32 give the true convolution bit for bit in any order, and a kernel that
drops or misplaces any one of them, or splits either operand into two bf16 terms instead of three, does not.

The emulation follows the kernel (aidax_ir_mfma.hip): per 32-frame input window and term product, one MFMA-sized sum (exact here in fp64,
rounded once to fp32), added to an fp32 accumulator window after window (the newest first) and, per window, product after product in the
kernel's order: (h0 h1 h2) x0, (h0 h1) x1, h0 x2. The reversed order (oldest window first, products backwards) must give the same bits."""
import numpy as np
import pytest

from tests import irdata
from tests.irdata import DROPPED, EXERCISES, KEPT, split3

CASES = [(f, L) for f in "ABC" for L in (1, 33, 8192)] + [("D", L) for L in (1, 5, 12)]
_DATA = {}


def _data(f, L):
    if (f, L) not in _DATA:
        _DATA[f, L] = irdata.FAMILIES[f](L, 2, max(4096, L + L // 2), seed=7)
    return _DATA[f, L]


def _terms(v, n=3):
    """the kernel's three bf16 terms of v; n = 2: a two-term split (the third term lost)"""
    t = list(split3(v))
    for k in range(n, 3):
        t[k] = np.zeros_like(t[k])
    return t


def emulate(hs, xs, products=KEPT, reverse=False, acc=np.float32):
    """sum over `products` (term of h, term of x) of hs[i] * xs[j], causally, as k_ir_conv adds them (see the module's docstring).
    hs: three tap vectors (their lengths may differ), xs: three [S][T] arrays. acc=np.float64: plain fp64 sums (for |.| activity)."""
    S, T = xs[0].shape
    U = -(-T // 32)
    Lh = max(h.size for h in hs)
    h64 = [np.pad(h.astype(np.float64), (0, Lh - h.size)) for h in hs]
    xb = [np.pad(x.astype(np.float64), ((0, 0), (0, 32 * U - T))).reshape(S, U, 32) for x in xs]
    M = (Lh + 30) // 32 + 1                                            # windows that reach an output: taps v + 32 m - r, r, v in [0, 32)
    y = np.zeros((S, U, 32), acc)
    r, v = np.arange(32)[:, None], np.arange(32)[None, :]
    order = list(products)[::-1] if reverse else list(products)
    for m in (range(M - 1, -1, -1) if reverse else range(M)):
        if m >= U:
            continue
        tap = v + 32 * m - r
        ok = (tap >= 0) & (tap < Lh)
        H = [np.where(ok, hv[np.clip(tap, 0, Lh - 1)], 0.0) for hv in h64]
        for i, j in order:
            d = np.zeros((S, U, 32))
            d[:, m:] = xb[j][:, :U - m] @ H[i]                          # one MFMA's sum per (window, output frame)
            y = (y + d.astype(acc)).astype(acc)
    return y.reshape(S, 32 * U)[:, :T]


def _active(h, x, p):
    """outputs where some term product of p = (term of h, term of x) is non-zero"""
    hs, xs = _terms(h), _terms(x)
    return emulate([np.abs(t) for t in hs], [np.abs(t) for t in xs], [p], acc=np.float64) > 0


def _changed(got, truth):
    return np.count_nonzero(got != truth) / got.size


@pytest.mark.parametrize("f,L", CASES)
def test_truth_is_the_fp64_convolution(f, L):
    h, x, truth = _data(f, L)
    assert h.size == L and truth.shape == x.shape
    for s in range(x.shape[0]):
        ref = np.convolve(h.astype(np.float64), x[s].astype(np.float64))[:x.shape[1]]
        assert np.array_equal(truth[s].astype(np.float64), ref)
    assert np.count_nonzero(truth) > 0.3 * truth.size


@pytest.mark.parametrize("f,L", CASES)
def test_six_products_in_fp32_are_exact_in_either_order(f, L):
    h, x, truth = _data(f, L)
    hs, xs = _terms(h), _terms(x)
    assert np.array_equal(emulate(hs, xs), truth)
    assert np.array_equal(emulate(hs, xs, reverse=True), truth)


@pytest.mark.parametrize("f,L", CASES)
def test_the_dropped_products_are_zero_and_the_claimed_ones_are_exercised(f, L):
    h, x, truth = _data(f, L)
    for p in DROPPED:
        assert not _active(h, x, p).any(), p
    live = truth != 0
    for p in EXERCISES[f]:
        share = np.count_nonzero(_active(h, x, p) & live) / np.count_nonzero(live)
        assert share > 0.3, (p, share)


@pytest.mark.parametrize("f,L", CASES)
def test_a_missing_or_misplaced_product_changes_the_output(f, L):
    """what the bit-exact GPU tests would see from a kernel that lost one product, split an operand in two, or a packer that put the
    IR's third term one diagonal (16 taps) late: at least 1 % of the outputs differ from the truth"""
    h, x, truth = _data(f, L)
    hs, xs = _terms(h), _terms(x)
    for p in EXERCISES[f]:
        assert _changed(emulate(hs, xs, [q for q in KEPT if q != p]), truth) >= 0.01, ("dropped", p)
    if (2, 0) in EXERCISES[f]:
        assert _changed(emulate(_terms(h, 2), xs), truth) >= 0.01, "two-term split of h"
        late = hs[:2] + [np.concatenate([np.zeros(16, np.float32), hs[2]])]
        assert _changed(emulate(late, xs), truth) >= 0.01, "h's third term on the next diagonal"
    if (0, 2) in EXERCISES[f]:
        assert _changed(emulate(hs, _terms(x, 2)), truth) >= 0.01, "two-term split of x"


def test_the_families_cover_every_kept_product_and_both_splits():
    assert set(KEPT) == set().union(*EXERCISES.values())
    assert not set(DROPPED) & set(KEPT) and len(set(KEPT) | set(DROPPED)) == 9
    assert any((2, 0) in e for e in EXERCISES.values()) and any((0, 2) in e for e in EXERCISES.values())
