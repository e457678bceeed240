"""The IR blend on the GPU (-m gpu): aidax_pool_assign_ir_b, aidax_pool_set_ir_mix, the plan's blend section and k_ir_mix (include/aidax.h,
"IR blend").

As in tests/test_gpu_ir_fade.py the pools run a real LSTM-16 model with every stream disabled, so the stage's input is the test's input
bit for bit. On the exact-arithmetic data of tests/irdata.py (family C: every convolution output is one exact product) both sides of a
blend are known to the last bit, and every output is held with np.array_equal to tests/irblend.py's mix32 of them under the weights of
irblend.weights. On random data each sample is held to TAU * E[t], TAU = 4e-6 being tests/test_gpu_ir.py's bound for one convolution: the
two sides enter with weights that sum to one (to a rounding of u), and the mix adds three fp32 roundings (u, the product, the fmaf), below
2e-7 * E together: the argument of tests/test_gpu_ir_fade.py's header. Blocks are cut as CUT, repeated, and at every frame a mix changes."""
import importlib

import numpy as np
import pytest

from tests import errlog, irblend, irdata, irfade, modelgen
from tests.test_gpu_ir import TAU
from tests.test_gpu_ir_bank_rt import _Device, _quiet, calls          # noqa: F401  (calls: a fixture)

pytestmark = pytest.mark.gpu
ax = importlib.import_module("aidadsp-lv2_amd")
ERR_ARG = -1
S7 = 7
CUT = [1, 17, 0, 64, 33, 256, 16]
NONE = ax.IR_NONE


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    p = str(tmp_path_factory.mktemp("ir_blend") / "lstm16.json")
    modelgen.write_model(modelgen.make_model(kind="lstm", hidden=16, input_size=1, seed=5), p)
    return ax.Model(p)


def _ir(L, seed, sign=1.0):
    rng = np.random.default_rng(seed)
    return (sign * rng.standard_normal(L) * np.exp(-np.arange(L) / max(L / 6.0, 1.0))).astype(np.float32)


def _pool(model, S, irs, A, B, F=0, max_frames=256):
    """a pool of disabled streams with bank slot k = irs[k], stream s on A[s] and with the second IR B[s]"""
    p = ax.Pool(S, max_frames)
    p.set_model(model)
    p.set_controls(ax.default_controls(enabled=0.0))
    if F:
        p.set_ir_fade(F)
    for k, h in enumerate(irs):
        p.set_ir_slot(k, h)
    for s in range(S):
        p.assign_ir(s, A[s])
        if B is not None:
            p.assign_ir_b(s, B[s])
    return p


def _process(p, blk):
    return p.process(np.ascontiguousarray(blk))


def _drive(pool, x, pattern, actions=(), via=_process, after=None):
    """x through the pool in blocks of `pattern` (repeated), cut short where an action is due. actions: (frame, stream, mix, R) for
    set_ir_mix, or (frame, callable) — applied at the block boundary at that frame. after(frame, n): called behind every pass."""
    due = sorted(actions, key=lambda a: a[0])
    out, pos, i, T = [], 0, 0, x.shape[1]
    while pos < T:
        while due and due[0][0] == pos:
            a = due.pop(0)
            if callable(a[1]):
                a[1](pool)
            else:
                pool.set_ir_mix(a[1], a[2], a[3])
        n = min(pattern[i % len(pattern)], (due[0][0] if due else T) - pos, T - pos)
        i += 1
        out.append(via(pool, x[:, pos:pos + n]))
        pos += n
        if after:
            after(pos, n)
    assert not due
    return np.concatenate(out, axis=1)


def _weights(S, T, actions):
    """(W, U, ramps): the weights of every stream's frames 0 .. T - 1 under the set_ir_mix actions, by irblend.Ramp"""
    W, U = np.zeros((S, T), np.float32), np.zeros((S, T), np.float32)
    ramps = [irblend.Ramp() for _ in range(S)]
    marks = sorted({a[0] for a in actions} | {0, T})
    for lo, hi in zip(marks[:-1], marks[1:]):
        for a in actions:
            if a[0] == lo:
                for s in (range(S) if a[1] == ax.ALL_STREAMS else [a[1]]):
                    ramps[s].set(a[2], a[3])
        for s in range(S):
            W[s, lo:hi], U[s, lo:hi] = ramps[s].take(hi - lo)
    return W, U, ramps


@pytest.fixture(scope="module")
def exact():
    """two family-C IRs (33 and 600 taps) on one impulse train spaced beyond the longer one, 7 streams x 4 rounds of CUT, with their
    exact convolutions: (hA, hB, x, yA, yB). Every stream's first impulse lies before frame BASE, where the ramps of the tests start"""
    T = 4 * sum(CUT)
    hB, x, yB = irdata.family_c(600, S7, T, seed=1)
    hA = irdata._taps(np.random.default_rng([0xC, 33, 2]), 33, 11)
    return hA, hB, x, irdata.exact_conv(hA, x), yB


def _sides(exact, A, B):
    """per stream the exact A and B sides of the layout (slot 0: hA, slot 1: hB, none: the dry block)"""
    _, _, x, yA, yB = exact
    side = {0: yA, 1: yB, NONE: x}
    return np.stack([side[a][s] for s, a in enumerate(A)]), np.stack([side[b][s] for s, b in enumerate(B)])


# ---- 1. rest mixes

def test_rest_mixes_are_exact_to_the_bit(model, exact):
    hA, hB, x, _, _ = exact
    A = [0, 0, 0, 0, 0, 0, NONE]
    B = [1, 1, 1, 1, 1, NONE, 1]
    mixes = [0.0, 0.25, 0.5, 0.75, 1.0, 0.5, 0.5]
    p = _pool(model, S7, [hA, hB], A, B)
    actions = [(0, s, m, 0) for s, m in enumerate(mixes)]
    got = _drive(p, x, CUT, actions)
    W, U, _ = _weights(S7, x.shape[1], actions)
    assert np.array_equal(W, np.repeat(np.float32(mixes)[:, None], x.shape[1], axis=1))
    ya, yb = _sides(exact, A, B)
    want = irblend.mix32(W, U, ya, yb)
    for s in range(S7):
        assert (want[s] != 0).sum() > 50
        assert np.array_equal(got[s], want[s]), (s, mixes[s], int((got[s] != want[s]).sum()))
    assert np.array_equal(got[0], ya[0]) and np.array_equal(got[4], yb[4])
    assert [p.stream_ir_mix(s) for s in (0, 2, 5)] == [(1, 0.0, 0.0, 0), (1, 0.5, 0.5, 0), (NONE, 0.5, 0.5, 0)]
    p.close()


# ---- 2. ramps

RAMP_A = [0, 0, 0, 0, 0, 0, NONE]
RAMP_B = [1, 1, 1, 1, 1, NONE, 1]
BASE = 650
# 0 -> 1 over 1, 8 and 512 frames from frame BASE; stream 3 jumps to 1, ramps to 0.25 over 300 frames and is interrupted after 100 by a
# ramp to 0.9 over 7; stream 4 stays at rest on 0; wet -> dry over 512 on stream 5; dry -> wet over 8 on stream 6, and back over 200
RAMP_ACTIONS = [(BASE, 0, 1.0, 1), (BASE, 1, 1.0, 8), (BASE, 2, 1.0, 512), (0, 3, 1.0, 0), (BASE, 3, 0.25, 300), (BASE + 100, 3, 0.9, 7),
                (BASE, 5, 1.0, 512), (BASE, 6, 1.0, 8), (BASE + 450, 6, 0.0, 200)]


def _ramp_run(model, exact, pattern, via=_process, check_state=True, actions=RAMP_ACTIONS):
    hA, hB, x, _, _ = exact
    p = _pool(model, S7, [hA, hB], RAMP_A, RAMP_B)
    _, _, ramps = _weights(S7, 0, [])
    due = sorted(actions, key=lambda a: a[0])
    state = {"pos": 0}

    def after(pos, n):
        # the host model moves on by the frames of the pass (the actions due at its start first), and the pool must report the same
        while due and due[0][0] == state["pos"]:
            a = due.pop(0)
            ramps[a[1]].set(a[2], a[3])
        before = [(r.now, r.left) for r in ramps]
        for r in ramps:
            r.take(n)
        state["pos"] = pos
        if n == 0:
            assert before == [(r.now, r.left) for r in ramps]
        if check_state:
            for s, r in enumerate(ramps):
                assert p.stream_ir_mix(s) == (RAMP_B[s], float(r.now), float(r.m1), r.left), (pos, s)
    got = _drive(p, x, pattern, actions, via, after)
    p.close()
    return got


@pytest.fixture(scope="module")
def ramp_truth(model, exact):
    """the ramps of test 2 through aidax_pool_process in blocks of CUT, checked against mix32: what every other way of issuing is held to"""
    x = exact[2]
    W, U, _ = _weights(S7, x.shape[1], RAMP_ACTIONS)
    ya, yb = _sides(exact, RAMP_A, RAMP_B)
    want = irblend.mix32(W, U, ya, yb)
    got = _ramp_run(model, exact, CUT)
    return got, want, W


def test_ramps_are_exact_to_the_bit_and_reported(model, exact, ramp_truth):
    got, want, W = ramp_truth
    # the weights are what the issue spells out: R = 1 jumps, R = 8 moves by eighths, the interrupted ramp starts from the weight of frame 99
    b = BASE
    assert W[0, b - 1:b + 2].tolist() == [0, 1, 1] and W[1, b - 1:b + 9].tolist() == [0, .125, .25, .375, .5, .625, .75, .875, 1, 1]
    assert W[3, b + 99] == np.float32(1.0 + (0.25 - 1.0) * 100 / 300) and W[3, b + 105] != W[3, b + 106] == np.float32(0.9) == W[3, b + 107]
    assert 0 < W[2, b + 300] < 1 and W[2, b + 511] == 1 and W[2, b + 510] < 1
    assert exact[2][:, :b].any(axis=1).all()
    for s in range(S7):
        assert np.array_equal(got[s], want[s]), (s, np.flatnonzero(got[s] != want[s])[:8])
    assert not np.array_equal(got[2], exact[3][2]) and not np.array_equal(got[2], exact[4][2])


def test_ramps_do_not_depend_on_the_cut(model, exact, ramp_truth):
    got = _ramp_run(model, exact, [256])
    assert np.array_equal(got, ramp_truth[0])


# ---- 3. random data against fp64

def test_random_data_matches_fp64(model):
    hs = [_ir(1, 1), _ir(100, 2), _ir(8192, 3, sign=-1.0)]
    A = [0, 1, 2, 2, NONE, 1, 2]
    B = [1, 2, 0, NONE, 1, 2, 1]
    T = 3 * sum(CUT)
    x = modelgen.signal(S7, T, seed=7)
    actions = [(0, 0, 0.3, 0), (0, 1, 0.62, 0), (18, 2, 1.0, 1000), (18, 3, 0.62, 1000), (0, 4, 0.3, 0), (0, 5, 1.0, 0), (18, 5, 0.0, 1000),
               (0, 6, 0.62, 0), (99, 6, 0.3, 1000)]
    p = _pool(model, S7, hs, A, B)
    got = _drive(p, x, CUT, actions)
    p.close()
    W, U, _ = _weights(S7, T, actions)
    worst = 0.0
    for s in range(S7):
        hA, hB = (None if k == NONE else hs[k] for k in (A[s], B[s]))
        y64, E = irblend.expected(x[s:s + 1], hA, hB, W[s], U[s])
        err = np.abs(got[s:s + 1].astype(np.float64) - y64)
        over = np.maximum(err - 1e-12 * E.max(), 0.0)                 # (the FFT's noise on near-silent samples, as in test_gpu_ir.py)
        assert not over[E <= 0].any(), s
        ratio = (over / np.where(E > 0, E, 1.0)).max()
        print(f"ir_blend random: stream {s} max |y - y64| / E = {ratio:.3e}")
        worst = max(worst, ratio)
        # the blend is really there: far from either side alone on most frames of a stream that rests inside (0, 1)
        if s in (0, 1, 4):
            a64, b64 = irfade.conv64(x[s:s + 1], hA), irfade.conv64(x[s:s + 1], hB)
            assert (np.abs(got[s] - a64[0]) > 10 * TAU * E[0]).mean() > 0.8 and (np.abs(got[s] - b64[0]) > 10 * TAU * E[0]).mean() > 0.8
    errlog.bound(worst, TAU, "ir_blend:random")


# ---- 4. hand-over

@pytest.mark.parametrize("F", [0, 64])
def test_hand_over_at_the_end_of_a_ramp(model, F):
    """after a ramp has ended on 1 (stream 0) and on 0 (stream 1), three more passes against a twin without a fade length that assigned
    the streams those IRs at the boundary behind the pass in which the ramps ended; then the recipe's last step"""
    hs = [_ir(600, 11), _ir(33, 12, sign=-1.0)]
    S = S7
    A = [0, 0, 0, 1, NONE, 0, 1]
    B = [1, 1, NONE, 0, 1, 1, 0]
    x = modelgen.signal(S, 64 + 64 + 64 + 17 + 256 + 64 + 64, seed=13)
    p = _pool(model, S, hs, A, B, F=F)
    twin = _pool(model, S, hs, A, None)
    p.set_ir_mix(1, 1.0, 0)                                            # stream 1 starts at rest on B ...
    twin.assign_ir(1, 1)
    p.set_ir_mix(5, 0.5, 0)                                            # (and two streams stay blended throughout)
    p.set_ir_mix(6, 0.25, 0)
    pos = 0

    def both(n):
        nonlocal pos
        blk = np.ascontiguousarray(x[:, pos:pos + n])
        pos += n
        return p.process(blk), twin.process(blk)
    a, b = both(64)
    assert np.array_equal(a[:5], b[:5]) and not np.array_equal(a[5], b[5])
    p.set_ir_mix(0, 1.0, 100)
    p.set_ir_mix(1, 0.0, 100)
    a, b = both(64)
    assert not np.array_equal(a[0], b[0]) and not np.array_equal(a[1], b[1]) and np.array_equal(a[2:5], b[2:5])
    assert p.stream_ir_mix(0)[3] == 36
    a, b = both(64)                                                    # the ramps end at frame 36 of this pass
    assert p.stream_ir_mix(0) == (1, 1.0, 1.0, 0) and p.stream_ir_mix(1) == (1, 0.0, 0.0, 0)
    twin.assign_ir(0, 1)
    twin.assign_ir(1, 0)
    for n in (17, 256, 64):
        a, b = both(n)
        assert np.array_equal(a[:5], b[:5]), (F, n, [s for s in range(5) if not np.array_equal(a[s], b[s])])
    # the recipe's last step: A takes the slot B plays, the mix jumps back to 0; the effective IR is the same slot content
    p.assign_ir(0, 1)
    p.set_ir_mix(0, 0.0, 0)
    a, b = both(64)
    assert np.array_equal(a[:5], b[:5])
    assert p.stream_ir_mix(0) == (1, 0.0, 0.0, 0) and p.stream_ir(0) == 1
    p.close()
    twin.close()


# ---- 5. plan geometry

def test_plan_geometry_with_fade_out_and_blend_sections_in_one_pass(model):
    S, n, F = 130, 256, 32
    hs = [_ir(600, 21), _ir(33, 22, sign=-1.0), _ir(100, 23), _ir(4097, 24)]
    A = [0] * 70 + [2] * 10 + [3] * 10 + [NONE] * 10 + [0] * 10 + [2] * 10 + [NONE] * 5 + [3] * 5
    B = [1] * 70 + [3] * 10 + [NONE] * 10 + [2] * 10 + [NONE] * 30
    mixes = [0.5] * 70 + [0.25] * 10 + [0.75] * 10 + [0.0] * 40
    x = modelgen.signal(S, 3 * n, seed=25)
    p = _pool(model, S, hs, A, B, F=F)
    twin = _pool(model, S, hs, A, None)
    for s in range(90):
        p.set_ir_mix(s, mixes[s], 0)
    for s in range(90, 100):
        p.set_ir_mix(s, 1.0, 2 * n + 100)                             # a ramp that is still running in the pass looked at
    for i in range(2):
        p.process(np.ascontiguousarray(x[:, i * n:(i + 1) * n]))
        twin.process(np.ascontiguousarray(x[:, i * n:(i + 1) * n]))
    for q in (p, twin):                                                # unblended streams change their IR: slot 0 -> slot 2
        for s in range(100, 110):
            q.assign_ir(s, 2)
    blk = np.ascontiguousarray(x[:, 2 * n:])
    got, other = p.process(blk), twin.process(blk)
    p.close()
    twin.close()
    W, U, _ = _weights(S, 3 * n, [(0, s, mixes[s], 0) for s in range(90)] + [(0, s, 1.0, 2 * n + 100) for s in range(90, 100)])
    worst = 0.0
    for lo, hi in ((0, 70), (70, 80), (80, 90), (90, 100)):
        rows = list(range(lo, hi))
        hA, hB = (None if k == NONE else hs[k] for k in (A[lo], B[lo]))
        y64, E = irblend.expected(x[rows], hA, hB, W[lo, -n:], U[lo, -n:])
        over = np.maximum(np.abs(got[rows].astype(np.float64) - y64) - 1e-12 * E.max(), 0.0)
        assert not over[E <= 0].any(), lo
        worst = max(worst, (over / np.where(E > 0, E, 1.0)).max())
    errlog.bound(worst, TAU, "ir_blend:geometry")
    rows = list(range(100, 110))
    y64, E = irfade.expected(x[rows], hs[0], hs[2], F, n)
    over = np.maximum(np.abs(got[rows].astype(np.float64) - y64) - 1e-12 * E.max(), 0.0)
    errlog.bound((over / np.where(E > 0, E, 1.0)).max(), TAU, "ir_blend:geometry-fade")
    assert not np.array_equal(got[100:110, :F], other[100:110, :F]) and np.array_equal(got[100:110, F:], other[100:110, F:])
    assert np.array_equal(got[110:], other[110:])                     # untouched streams: the twin's bits


# ---- 6. every way a pass is issued

def test_submit_and_collect_with_three_blocks_in_flight(model, exact, ramp_truth):
    """ramps advance at issue: a set_ir_mix between two submits applies from the next submitted block, while earlier blocks are in flight"""
    hA, hB, x, _, _ = exact
    p = _pool(model, S7, [hA, hB], RAMP_A, RAMP_B)
    flight, out = [], []

    def via(pool, blk):
        if blk.shape[1]:
            pool.submit(np.ascontiguousarray(blk))
            flight.append(blk.shape[1])
        if len(flight) == 3:
            out.append(pool.collect(flight.pop(0)))
        return blk[:, :0]
    _drive(p, x, CUT, RAMP_ACTIONS, via)
    while flight:
        out.append(p.collect(flight.pop(0)))
    p.close()
    assert np.array_equal(np.concatenate(out, axis=1), ramp_truth[0])


def test_process_device_on_a_callers_stream(model, exact, ramp_truth):
    import torch
    dev = _Device(S7, 1, seed=0)

    def via(pool, blk):
        if blk.shape[1] == 0:
            pool.process_device(0, 0, 0, dev.s.cuda_stream)
            return blk
        dev.x = torch.from_numpy(np.ascontiguousarray(blk)).cuda()
        dev.y = torch.empty_like(dev.x)
        torch.cuda.synchronize()
        dev.pass_(pool)
        return dev.wait()
    got = _ramp_run(model, exact, CUT, via)
    assert np.array_equal(got, ramp_truth[0])


def test_reset_stream_keeps_the_blend_and_clears_the_history(model, exact):
    hA, hB, x, _, _ = exact
    T = x.shape[1]
    cutoff = BASE + 50
    actions = [(0, 1, 0.5, 0), (BASE, 2, 1.0, 512), (cutoff, lambda p: (p.reset_stream(1, ax.START_RESET), p.reset_stream(2, ax.START_RESET)))]
    p = _pool(model, S7, [hA, hB], RAMP_A, RAMP_B)
    seen = {}

    def after(pos, n):
        if pos == cutoff:
            seen["before"] = [p.stream_ir_mix(s) for s in range(S7)]
    got = _drive(p, x, CUT, actions, after=after)
    assert seen["before"][2][3] == BASE + 512 - cutoff and seen["before"][1] == (1, 0.5, 0.5, 0)
    W, U, _ = _weights(S7, T, actions[:2])
    ya, yb = _sides(exact, RAMP_A, RAMP_B)
    cleared = x.copy()
    cleared[1:3, :cutoff] = 0                                          # streams 1 and 2 have no past before the reset
    ya2, yb2 = irdata.exact_conv(hA, cleared), irdata.exact_conv(hB, cleared)
    ya[1:3, cutoff:], yb[1:3, cutoff:] = ya2[1:3, cutoff:], yb2[1:3, cutoff:]
    want = irblend.mix32(W, U, ya, yb)
    assert not np.array_equal(yb2[1:3, cutoff:], exact[4][1:3, cutoff:])          # (the cleared history is audible)
    assert np.array_equal(got, want)
    p.close()


# ---- 7. nothing else moves

def _counted_passes(p, dev, k, calls):
    out = []
    for _ in range(k):
        dev.pass_(p)
        out.append(calls())
        dev.wait()
        calls()
    return out


def test_launches_and_uploads(model, calls):
    S, n = 70, 64
    hs = [_ir(600, 31), _ir(33, 32)]
    dev = _Device(S, n, seed=33)
    plain = _pool(model, S, hs, [0] * S, None, F=32)
    withb = _pool(model, S, hs, [0] * S, [1] * S, F=32)
    withb.set_ir_mix(ax.ALL_STREAMS, 0.0, 0)
    runs = []
    for p in (plain, withb):
        _counted_passes(p, dev, 2, calls)
        steady = _counted_passes(p, dev, 2, calls)
        p.assign_ir(3, 1)                                              # a fade pass
        fade = _counted_passes(p, dev, 1, calls)[0]
        runs.append((steady, fade))
    (steady, fade), (steady_b, fade_b) = runs
    stage = lambda c: {k: v for k, v in c.items() if k.startswith("launch_ir")}
    assert stage(steady[0]) == stage(steady[1]) == {"launch_ir_append": 1, "launch_ir_conv": 1}
    assert stage(fade) == {"launch_ir_append": 1, "launch_ir_conv": 2, "launch_ir_fade": 1}
    assert "hipMemcpyAsync" not in steady[1] and fade.get("hipMemcpyAsync", 0) == 1
    assert steady_b == steady and fade_b == fade                       # a B assignment at rest on 0: every counted call the same
    # the three new calls are host records
    calls()
    withb.assign_ir_b(2, NONE)
    withb.assign_ir_b(ax.ALL_STREAMS, 1)
    withb.set_ir_mix(5, 0.5, 0)
    withb.set_ir_mix(6, 1.0, 10 * n)
    assert withb.stream_ir_mix(6) == (1, 0.0, 1.0, 10 * n)
    assert calls() == {}
    # blended passes: one more convolution launch and the mix, nothing else; only the first pass of the ramp uploads a plan
    ramp = _counted_passes(withb, dev, 10, calls)
    for i, c in enumerate(ramp):
        _quiet(c, f"ramp pass {i}")
        extra = {k: c.get(k, 0) - steady[1].get(k, 0) for k in set(c) | set(steady[1]) if c.get(k, 0) != steady[1].get(k, 0)}
        want = {"launch_ir_conv": 1, "launch_ir_mix": 1}
        if i == 0:
            assert extra.pop("hipMemcpyAsync") == 1 and extra.pop("hipEventRecord", 1) == 1, c
            extra.pop("hipEventQuery", None)
        assert extra == want, (i, c)
    assert withb.stream_ir_mix(6) == (1, 1.0, 1.0, 0)
    # the pass behind the ramp's end: stream 6 is a one-IR stream again (a new plan), stream 5 stays blended
    c = _counted_passes(withb, dev, 1, calls)[0]
    assert c.get("hipMemcpyAsync", 0) == 1 and c["launch_ir_mix"] == 1 and c["launch_ir_conv"] == 2, c
    c = _counted_passes(withb, dev, 1, calls)[0]
    assert "hipMemcpyAsync" not in c, c
    plain.close()
    withb.close()


# ---- 8. refused calls

def test_refused_calls_change_nothing(model, exact):
    hA, hB, x, _, _ = exact
    L = ax.lib()
    p = _pool(model, S7, [hA, hB], RAMP_A, RAMP_B)
    twin = _pool(model, S7, [hA, hB], RAMP_A, RAMP_B)
    for q in (p, twin):
        q.set_ir_mix(1, 0.5, 0)
        q.set_ir_mix(2, 1.0, 300)
    bad = [lambda: L.aidax_pool_set_ir_mix(p.h, 1, float("nan"), 0), lambda: L.aidax_pool_set_ir_mix(p.h, 1, -0.1, 0),
           lambda: L.aidax_pool_set_ir_mix(p.h, ax.ALL_STREAMS, 1.5, 0), lambda: L.aidax_pool_set_ir_mix(p.h, 2, 0.0, (1 << 24) + 1),
           lambda: L.aidax_pool_set_ir_mix(p.h, S7, 0.0, 0), lambda: L.aidax_pool_set_ir_mix(p.h, -2, 0.0, 0),
           lambda: L.aidax_pool_assign_ir_b(p.h, 1, 64), lambda: L.aidax_pool_assign_ir_b(p.h, ax.ALL_STREAMS, -3),
           lambda: L.aidax_pool_assign_ir_b(p.h, S7, 0), lambda: L.aidax_pool_assign_ir_b(p.h, -2, 0)]
    pos = 430
    for i, call in enumerate(bad):
        n = CUT[i % len(CUT)] or 5
        state = [p.stream_ir_mix(s) for s in range(S7)]
        assert call() == ERR_ARG, i
        assert state == [p.stream_ir_mix(s) for s in range(S7)] == [twin.stream_ir_mix(s) for s in range(S7)], i
        blk = np.ascontiguousarray(x[:, pos:pos + n])
        pos += n
        assert np.array_equal(p.process(blk), twin.process(blk)), i
    assert L.aidax_pool_stream_ir_mix(p.h, S7, None, None, None, None) == ERR_ARG
    p.close()
    twin.close()
