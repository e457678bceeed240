"""The IR fade, the parts that need no device: the two entry points' exports from both builds of the library, the argument checks made
before any device is touched, and the fp64 helper the GPU tests hold the fade pass against (tests/irfade.py), on cases small enough to
work out by hand."""
import ctypes as C
import importlib

import numpy as np

from tests import conftest, irfade

ax = importlib.import_module("aidadsp-lv2_amd")
ERR_ARG = -1
NEW = ("aidax_pool_set_ir_fade", "aidax_pool_ir_fade")


def test_both_libraries_export_the_entry_points():
    names = ax.declared_symbols()
    for path in (conftest.SHIP_LIB, conftest.HOOKS_LIB):
        L = C.CDLL(path)
        for n in NEW:
            assert n in names, n
            assert hasattr(L, n), (path, n)
    with open(f"{conftest.ROOT}/include/aidax.h") as f:
        threads = f.read().split("/* Threads.")[1].split("*/")[0]
    assert "set_ir_fade" in threads.split("plus, concurrently")[0]       # an audio-side call


def test_argument_checks_without_a_pool():
    L = ax.lib()
    assert L.aidax_pool_set_ir_fade(None, 64) == ERR_ARG
    assert "null pool" in L.aidax_last_error().decode()
    assert L.aidax_pool_set_ir_fade(None, 8193) == ERR_ARG
    assert "fade length" in L.aidax_last_error().decode()
    assert L.aidax_pool_set_ir_fade(None, 0xffffffff) == ERR_ARG
    assert L.aidax_pool_ir_fade(None) == 0
    assert hasattr(ax.Pool, "set_ir_fade") and hasattr(ax.Pool, "ir_fade")


def test_weights():
    assert irfade.weights(4, 6).tolist() == [0.25, 0.5, 0.75, 1.0, 1.0, 1.0]
    assert irfade.weights(8, 2).tolist() == [0.5, 1.0]                   # Lf = min(F, n)
    assert irfade.weights(3, 3).tolist() == [1 / 3, 2 / 3, 1.0]
    assert irfade.weights(1, 3).tolist() == [1.0, 1.0, 1.0]              # a fade of one frame is the abrupt switch


def test_conv64_by_hand():
    x = np.array([[1.0, 2.0, 3.0, 4.0], [0.0, -1.0, 0.0, 2.0]])
    assert irfade.conv64(x, np.array([2.0])).tolist() == [[2, 4, 6, 8], [0, -2, 0, 4]]
    assert irfade.conv64(x, np.array([1.0, -1.0])).tolist() == [[1, 1, 1, 1], [0, -1, 1, 2]]
    assert irfade.conv64(x, np.array([0.0, 0.0, 0.5])).tolist() == [[0, 0, 0.5, 1], [0, 0, 0, -0.5]]
    assert irfade.conv64(x, None).tolist() == x.tolist()
    # the FFT path against the tap-by-tap one
    rng = np.random.default_rng(1)
    xs, h = rng.standard_normal((3, 300)), rng.standard_normal(100)
    direct = np.array([np.convolve(r, h)[:300] for r in xs])
    assert np.abs(irfade.conv64(xs, h) - direct).max() < 1e-12


def test_expected_block_by_hand():
    # history 1 2 | block 3 4 5 6; old = a gain of 2, new = [1, -1] (the first difference); F = 4 of n = 4
    x = np.array([[1.0, 2.0, 3.0, 4.0, 5.0, 6.0]])
    y, E = irfade.expected(x, np.array([2.0]), np.array([1.0, -1.0]), 4, 4)
    # old 6 8 10 12, new 1 1 1 1, w = 1/4 1/2 3/4 1
    assert np.allclose(y, [[0.75 * 6 + 0.25, 0.5 * 8 + 0.5, 0.25 * 10 + 0.75, 1.0]], rtol=0, atol=1e-15)
    # |old| * |x| = 6 8 10 12, |new| * |x| = 5 7 9 11
    assert np.allclose(E, [[0.75 * 6 + 0.25 * 5, 0.5 * 8 + 0.5 * 7, 0.25 * 10 + 0.75 * 9, 11.0]], rtol=0, atol=1e-15)
    # F = 2: the fade ends inside the block, the rest is the new side
    y, E = irfade.expected(x, np.array([2.0]), np.array([1.0, -1.0]), 2, 4)
    assert np.allclose(y, [[0.5 * 6 + 0.5, 1.0, 1.0, 1.0]], rtol=0, atol=1e-15)
    assert np.allclose(E, [[0.5 * 6 + 0.5 * 5, 7.0, 9.0, 11.0]], rtol=0, atol=1e-15)
    # F above n: Lf = n
    y8, _ = irfade.expected(x, np.array([2.0]), np.array([1.0, -1.0]), 8, 4)
    y4, _ = irfade.expected(x, np.array([2.0]), np.array([1.0, -1.0]), 4, 4)
    assert np.array_equal(y8, y4)


def test_nothing_is_the_unit_impulse():
    x = np.array([[1.0, -2.0, 3.0, -4.0]])
    # from no IR to a delay of one frame with gain 3, over the whole block of 2
    y, E = irfade.expected(x, None, np.array([0.0, 3.0]), 2, 2)
    assert np.allclose(y, [[0.5 * 3 + 0.5 * -6, 9.0]], rtol=0, atol=1e-15)
    assert np.allclose(E, [[0.5 * 3 + 0.5 * 6, 9.0]], rtol=0, atol=1e-15)
    # ... and back
    y, E = irfade.expected(x, np.array([0.0, 3.0]), None, 2, 2)
    assert np.allclose(y, [[0.5 * -6 + 0.5 * 3, -4.0]], rtol=0, atol=1e-15)
    assert np.allclose(E, [[0.5 * 6 + 0.5 * 3, 4.0]], rtol=0, atol=1e-15)
    # the same IR on both sides is that IR, whatever the weights
    h = np.array([0.5, 0.25])
    y, _ = irfade.expected(x, h, h, 2, 2)
    assert np.allclose(y, irfade.conv64(x, h)[:, -2:], rtol=0, atol=1e-15)
