"""The noise gate on the GPU (-m gpu): a gated pool fed x returns, bit for bit, what a pool that never had a gate returns when fed the
reference's gated x (tests/gatehelp.py: the per-frame rule, sequentially, in numpy), and aidax_pool_read_gate returns the reference's
(hold_left, atten) after every pass: on every form that stages its input block differently, on every path a pass can take, across
parameter changes, resets and disabled streams. No tolerance anywhere.

Shapes: five streams (a lone wave in the second workgroup) and the ragged block plan of tests/test_gpu_meters.py (1, 3, 63, 65, 257:
unaligned rows, every tail around the wave width, several chunks); four parameter sets (gatehelp.SETS: short ramps; a hold and a release
that cross passes; attack 1, where up = P; hold 1)."""
import importlib

import numpy as np
import pytest

from tests import gatehelp as gh, modelgen, rateref as rr

pytestmark = pytest.mark.gpu
ax = importlib.import_module("aidadsp-lv2_amd")

ERR_ARG, ERR_STATE = -1, -6
P = gh.P
PLAN = [1, 3, 0, 63, 64, 65, 257, 4] * 2


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def _write(tmp_path_factory, name, **kw):
    p = str(tmp_path_factory.mktemp("gate") / f"{name}.json")
    modelgen.write_model(modelgen.make_model(**kw), p)
    return p


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    return ax.Model(_write(tmp_path_factory, "lstm16", kind="lstm", hidden=16, input_size=1, seed=5))


def _pool(model, S, max_frames, rate=48000.0, **controls):
    p = ax.Pool(S, max_frames, rate)
    p.set_model(model)
    if controls:
        p.set_controls(ax.default_controls(**controls))
    return p


def _cuts(x, plan):
    at = 0
    for n in plan:
        yield np.ascontiguousarray(x[:, at:at + n])
        at += n


def _rec(k, rate=48000.0, **kw):
    """(the GateParams of parameter set k, their record at `rate`)"""
    pr = gh.params(**dict(gh.SETS[k % len(gh.SETS)], **kw), rate=rate)
    return pr, ax.gate_design(pr, rate)


def _gate_all(pool, ref, S, **kw):
    """stream s on parameter set s mod 4, in the pool and in the reference"""
    for s in range(S):
        pr, rec = _rec(s, **kw)
        pool.set_gate(pr, s)
        ref.set(s, rec)


def _run(a, b, ref, blocks, what=""):
    """every block through the gated pool `a` and, gated by the reference, through the plain pool `b`: the same bits, the same state"""
    for k, blk in enumerate(blocks):
        want_in = ref.process(blk)
        ya, yb = a.process(blk), b.process(want_in)
        assert same(ya, yb), f"{what} pass {k} of {blk.shape[1]} frames"
        got, want = a.read_gate(), ref.state()
        assert got.tobytes() == want.tobytes(), (what, k, got, want)


def test_composition(model):
    S = 5
    a, b, ref = _pool(model, S, 257), _pool(model, S, 257), gh.Reference(S)
    _gate_all(a, ref, S)
    assert a.read_gate().tobytes() == bytes(8 * S)
    for s in range(S):
        pr, on = a.stream_gate(s)
        assert on and bytes(pr) == bytes(_rec(s)[0])
    assert a.kernel_name == b.kernel_name
    x = gh.signal(S, sum(PLAN), seed=41)
    _run(a, b, ref, _cuts(x, PLAN))
    ref.assert_covered()
    # the gate did something: some stream ended closed, and the gated input is not the input
    assert (a.read_gate()["atten"] == P).any() and not same(gh.Reference(S).process(x), ref.process(x))
    a.close()
    b.close()


FORMS = {
    # a table model on whole tiles with a full workgroup: k_lstm_pipe4 (the 37-frame block is k_lstm_pipe's, on the same state)
    "pipe4": (dict(kind="lstm", hidden=16, input_size=1, seed=5), 5, 64, [64, 48, 37, 64], "k_lstm_pipe4<16>"),
    "conv": (dict(kind="conv", hidden=16, input_size=1, seed=4), 5, 64, [64, 33, 64], "k_conv_st"),
    "stack": (dict(kind="lstm", hidden=12, input_size=1, seed=7, n_rnn=2), 5, 64, [64, 33, 64], None),
    # the LV2 instance's pool: one stream, the block read in pinned host memory, the completion word written by the model's kernel
    "one-stream": (dict(kind="lstm", hidden=16, input_size=1, seed=5), 1, 64, [64] * 8, None),
}


@pytest.mark.parametrize("form", sorted(FORMS))
def test_forms(tmp_path_factory, form):
    """(the two pools live one after the other: a stacked model's chained kernel is one pool's per device at a time)"""
    spec, S, max_frames, plan, kernel = FORMS[form]
    m = ax.Model(_write(tmp_path_factory, form, **spec))
    blocks = list(_cuts(gh.signal(S, sum(plan), seed=42), plan))
    a, ref = _pool(m, S, max_frames), gh.Reference(S)
    _gate_all(a, ref, S)
    name = a.kernel_name
    print(form, "runs", name)
    assert kernel is None or name == kernel
    got, want_in = [], []
    for k, blk in enumerate(blocks):
        want_in.append(ref.process(blk))
        got.append(a.process(blk))
        assert a.read_gate().tobytes() == ref.state().tobytes(), (form, k)
    assert a.kernel_name == name
    a.close()
    b = _pool(m, S, max_frames)
    assert b.kernel_name == name
    for k, (y, w) in enumerate(zip(got, want_in)):
        assert same(y, b.process(w)), f"{form} pass {k} of {w.shape[1]} frames"
    b.close()


def test_submit_and_collect_with_a_change_between_two_blocks_in_flight(model):
    """each block plays under the records in force when it was submitted: block 1 is in flight when stream 0's parameters change, stream 1
    goes off and stream 2 comes on (its state cleared behind block 1's pass, ahead of block 2's)"""
    S = 6
    a, b, ref = _pool(model, S, 64), _pool(model, S, 64), gh.Reference(S)
    for s in (0, 1, 3, 4, 5):
        pr, rec = _rec(s)
        a.set_gate(pr, s)
        ref.set(s, rec)
    blocks = list(_cuts(gh.signal(S, 64 * 3 + 37, seed=43), [64, 64, 37, 64]))
    want = [ref.process(blocks[0])]
    a.submit(blocks[0])
    pr, rec = _rec(1, hold=3)
    a.set_gate(pr, 0)
    ref.set(0, rec)
    a.set_gate(None, 1)
    ref.set(1, None)
    pr, rec = _rec(2)
    a.set_gate(pr, 2)
    ref.set(2, rec)
    want.append(ref.process(blocks[1]))
    a.submit(blocks[1])
    got = [a.collect(64)]
    pr, rec = _rec(3)
    a.set_gate(pr, 1)                                          # on again: from (0, 0)
    ref.set(1, rec)
    for blk in blocks[2:]:
        want.append(ref.process(blk))
        a.submit(blk)
    state = a.read_gate()                                       # behind every pass issued so far
    got += [a.collect(64), a.collect(37), a.collect(64)]
    assert state.tobytes() == ref.state().tobytes()
    for k, (y, w) in enumerate(zip(got, want)):
        assert same(y, b.process(w)), f"block {k}"
    a.close()
    b.close()


def test_process_device_in_place_and_on_a_callers_stream(model):
    import torch
    S, n = 5, 65
    a, b, ref = _pool(model, S, 65), _pool(model, S, 65), gh.Reference(S)
    _gate_all(a, ref, S)
    x = gh.signal(S, n * 4, seed=44)
    stream = torch.cuda.Stream()
    for k, blk in enumerate(_cuts(x, [n] * 4)):
        want = b.process(ref.process(blk))
        d_x = torch.from_numpy(blk).cuda()
        d_y = torch.empty_like(d_x)
        torch.cuda.synchronize()
        in_place, own = k % 2 == 1, k >= 2                      # out of place / in place, on the pool's stream / on the caller's
        with torch.cuda.stream(stream):
            a.process_device(d_x.data_ptr(), d_x.data_ptr() if in_place else d_y.data_ptr(), n, stream.cuda_stream if own else 0)
        if own:
            stream.synchronize()
        else:
            a.sync()
        got = (d_x if in_place else d_y).cpu().numpy()
        assert same(got, want), f"pass {k}"
        if not in_place:
            assert same(d_x.cpu().numpy(), blk)                 # the block the pass was handed is only read
        assert a.read_gate().tobytes() == ref.state().tobytes()
    a.close()
    b.close()


def test_under_a_rate_adapter(model):
    """44.1 kHz around a 48 kHz pool: the gate is designed at the pool's rate and sees the pool-rate block between the adapter's two
    stages; against the two stages by hand around a plain pool, with the reference's gate between the first stage and the pool"""
    S, host, rate = 3, 44100, 48000
    blocks = (64, 1, 255, 17, 256)
    a, b, ref = _pool(model, S, 288, float(rate)), _pool(model, S, 288, float(rate)), gh.Reference(S)
    _gate_all(a, ref, S, rate=float(rate))
    ad = ax.RateAdapter(a, float(host), 256)
    H_A, d_B = rr.delays(host, rate)
    A = ax.Resampler(S, float(host), float(rate), H_A, 0, 256)
    B = ax.Resampler(S, float(rate), float(host), 0, d_B, 288)
    x = gh.signal(S, sum(blocks), seed=45)
    for k, (blk, m) in enumerate(zip(_cuts(x, blocks), rr.pool_frames(blocks, host, rate))):
        got = ad.process(blk)
        ya = A.process(blk, m)
        yb = b.process(ref.process(ya))
        assert same(got, B.process(yb, blk.shape[1])), f"block {k}"
        assert a.read_gate().tobytes() == ref.state().tobytes()
    assert (a.read_gate()["hold_left"] != 0).any() or (a.read_gate()["atten"] != 0).any()
    ad.close()
    A.close()
    B.close()
    a.close()
    b.close()


def test_with_a_model_bank_assignment_in_force(model, tmp_path_factory):
    S = 8
    other = ax.Model(_write(tmp_path_factory, "lstm16_b", kind="lstm", hidden=16, input_size=1, seed=6))
    a, b, ref = _pool(model, S, 64), _pool(model, S, 64), gh.Reference(S)
    for p in (a, b):
        p.set_model_slot(1, other)
        p.assign_model(S - 1, 1, ax.START_RESET)
    _gate_all(a, ref, S)
    assert "bank" in a.kernel_name and a.kernel_name == b.kernel_name
    _run(a, b, ref, _cuts(gh.signal(S, 64 + 33 + 64, seed=46), [64, 33, 64]), what="bank")
    a.close()
    b.close()


def test_with_an_ir_and_the_meters_on(model):
    """the meters' input side describes the block the pass was handed, before the gate; everything behind the gate sees the gated block"""
    S = 5
    a, b, c, ref = _pool(model, S, 65), _pool(model, S, 65), _pool(model, S, 65), gh.Reference(S)
    for p in (a, b, c):
        p.set_ir(np.array([0.5, 0.25, -0.125], np.float32))
        p.set_metering(True)
    _gate_all(a, ref, S)
    for k, blk in enumerate(_cuts(gh.signal(S, 65 * 3, seed=47), [65, 64, 65])):
        gated = ref.process(blk)
        assert same(a.process(blk), b.process(gated)), f"pass {k}"
        c.process(blk)
    ma, mb, mc = a.read_meters(), b.read_meters(), c.read_meters()
    for f in ("in_peak", "in_energy", "in_nonfinite"):
        assert ma[f].tobytes() == mc[f].tobytes(), f
    for f in ("frames", "passes", "out_peak", "out_energy", "out_nonfinite", "out_over"):
        assert ma[f].tobytes() == mb[f].tobytes(), f
    assert (ma["in_energy"] != mb["in_energy"]).any()
    for p in (a, b, c):
        p.close()


def test_off_is_free(model):
    """a pool whose gate is allocated and off everywhere, a pool whose gate is on and transparent (every sample opens it: unity gain; and
    were it closed, floor_db = 0 is a gain of 1.0), and a pool without a gate: the same bits, the same kernel"""
    S = 5
    plain, off, clear = _pool(model, S, 257), _pool(model, S, 257), _pool(model, S, 257)
    off.set_gate(_rec(0)[0])
    off.set_gate(None)
    assert [off.stream_gate(s)[1] for s in range(S)] == [False] * S
    clear.set_gate(ax.GateParams(-120.0, -120.0, 0.0, 1.0, 1.0, 1.0))
    assert plain.kernel_name == off.kernel_name == clear.kernel_name
    for k, blk in enumerate(_cuts(modelgen.signal(S, sum(PLAN), seed=21), PLAN)):
        y = plain.process(blk)
        assert same(off.process(blk), y) and same(clear.process(blk), y), f"pass {k}"
    assert off.read_gate().tobytes() == bytes(8 * S)            # an off gate's state does not move
    assert plain.kernel_name == off.kernel_name == clear.kernel_name
    for p in (plain, off, clear):
        p.close()


def test_a_disabled_stream_returns_the_ungated_block(model):
    S = 5
    a, b, ref = _pool(model, S, 65), _pool(model, S, 65), gh.Reference(S)
    _gate_all(a, ref, S)
    blocks = list(_cuts(gh.signal(S, 65 * 3, seed=48), [65, 65, 65]))
    _run(a, b, ref, blocks[:1])
    for p in (a, b):
        p.set_controls(ax.default_controls(enabled=0.0), 1)
    before = a.read_gate()[1]
    assert (int(before["hold_left"]), int(before["atten"])) != (0, 0)
    want_in = ref.process(blocks[1], skip=(1,))
    ya = a.process(blocks[1])
    assert same(ya, b.process(want_in)) and same(ya[1], blocks[1][1])
    assert a.read_gate()[1] == before and a.read_gate().tobytes() == ref.state().tobytes()
    for p in (a, b):
        p.set_controls(ax.default_controls(), 1)
    _run(a, b, ref, blocks[2:])                                 # enabled again: the gate goes on from where it stood
    a.close()
    b.close()


def test_life_cycle(model):
    S = 5
    a, b, ref = _pool(model, S, 64), _pool(model, S, 64), gh.Reference(S)
    with pytest.raises(ax.AidaxError) as e:
        a.read_gate()
    assert e.value.code == ERR_STATE
    a.set_gate(None)                                            # off before it was ever on: still nothing to read
    with pytest.raises(ax.AidaxError) as e:
        a.read_gate()
    assert e.value.code == ERR_STATE
    assert a.stream_gate(0)[1] is False
    # AIDAX_ALL_STREAMS sets every stream
    pr, rec = _rec(1)                                           # hold 300, release 700: the state is in mid-flight after a block
    a.set_gate(pr)
    for s in range(S):
        ref.set(s, rec)
        got, on = a.stream_gate(s)
        assert on and bytes(got) == bytes(pr)
    blocks = list(_cuts(gh.signal(S, 64 * 6, seed=49), [64] * 6))
    _run(a, b, ref, blocks[:2])
    assert (a.read_gate()["hold_left"] > 7).any()
    # refused calls change nothing
    before = a.read_gate()
    for stream, params in ((S, pr), (-2, pr), (0, ax.GateParams(-30.0, -20.0, -40.0, 1.0, 1.0, 1.0)), (ax.ALL_STREAMS, ax.GateParams(0.0, 0.0, 1.0, 1.0, 1.0, 1.0)),
                           (1, ax.GateParams(-20.0, -30.0, -40.0, float("nan"), 1.0, 1.0))):
        with pytest.raises(ax.AidaxError) as e:
            a.set_gate(params, stream)
        assert e.value.code == ERR_ARG
    for first, count in ((0, 0), (4, 2), (5, 1), (0, 6), (0xFFFFFFFF, 2)):
        with pytest.raises(ax.AidaxError) as e:
            a.read_gate(first, count)
        assert e.value.code == ERR_ARG
    assert a.read_gate().tobytes() == before.tobytes() and all(bytes(a.stream_gate(s)[0]) == bytes(pr) for s in range(S))
    assert a.read_gate(1, 3).tobytes() == before[1:4].tobytes()
    # a parameter change keeps q and clips c (hold 300 -> 7): read back after the next pass, against the reference that does the same
    pr2, rec2 = _rec(0)
    a.set_gate(pr2, 0)
    ref.set(0, rec2)
    assert a.read_gate().tobytes() == before.tobytes()          # a host record: the state itself is clipped where it is used
    # reset_stream zeroes the state, and so does off -> on; on -> on does not
    a.reset_stream(1)
    b.reset_stream(1)
    ref.reset(1)
    a.set_gate(None, 2)
    a.set_gate(pr, 2)
    ref.set(2, None)
    ref.set(2, rec)
    a.set_gate(pr, 3)
    ref.set(3, rec)
    now = a.read_gate()
    assert now[[1, 2]].tobytes() == bytes(16) and now[[0, 3, 4]].tobytes() == before[[0, 3, 4]].tobytes()
    assert now.tobytes() == ref.state().tobytes()
    _run(a, b, ref, blocks[2:4])
    assert a.read_gate()["hold_left"][0] <= 7
    # off then on restarts at unity gain, (0, 0), whatever the state was; a stream that stays off keeps its state untouched
    a.set_gate(None)
    for s in range(S):
        ref.set(s, None)
    parked = a.read_gate()
    assert same(a.process(blocks[4]), b.process(blocks[4])) and a.read_gate().tobytes() == parked.tobytes()
    a.set_gate(pr, 4)
    ref.set(4, rec)
    assert a.read_gate()[4].tobytes() == bytes(8) and a.read_gate()[:4].tobytes() == parked[:4].tobytes()
    _run(a, b, ref, blocks[5:])
    a.close()
    b.close()


def test_non_finite_input(model):
    """a NaN is a quiet frame and comes out as a NaN (with q == 0: its own bits), +-Inf opens the gate. What the model makes of a NaN is
    its own business, so the comparison is again with a plain pool fed the reference's block, NaNs and all; where both outputs are NaN the
    payloads are not compared (a NaN times a gain: the payload is the hardware's)."""
    S = 2
    a, b, ref = _pool(model, S, 130), _pool(model, S, 130), gh.Reference(S)
    pr, rec = _rec(0, floor_db=-120.0)
    a.set_gate(pr)
    for s in range(S):
        ref.set(s, rec)
    x = gh.signal(S, 130, seed=50)
    x[0, :40] = np.float32(0.001)                               # stream 0 closes (release: 11 frames) ...
    x[0, 20] = np.nan                                           # ... a NaN in the closed stretch is a quiet frame: a NaN comes out, the state moves on
    x[0, 40] = np.inf                                           # +Inf opens the gate
    x[0, 41:60] = np.float32(0.2)
    bits(x)[0, 55] = 0x7FC12345                                 # q == 0 here (attack: 5 frames from frame 40): the NaN's own bits, and a quiet frame
    x[0, 56] = -np.inf
    assert bits(x)[0, 55] == 0x7FC12345
    quiet = x.copy()
    quiet[0, 20] = quiet[0, 55] = 0.0
    twin = gh.Reference(S)
    for s in range(S):
        twin.set(s, rec)
    want_in = ref.process(x)
    twin.process(quiet)
    assert ref.state().tobytes() == twin.state().tobytes()      # (on the reference alone: the NaNs moved the state as quiet frames do)
    assert np.isnan(want_in[0, 20]) and bits(want_in)[0, 55] == 0x7FC12345 and want_in[0, 40] == np.inf and want_in[0, 56] == -np.inf
    ya = a.process(x)
    assert a.read_gate().tobytes() == ref.state().tobytes()
    yb = b.process(want_in)
    assert gh.same_bits(ya, yb) and same(ya[1], yb[1])
    a.close()
    b.close()


def test_one_block_of_8192_frames(model):
    """128 chunks in one launch: the carry from chunk to chunk, a hold of 5000 frames counted down across them, and a release of 6000
    frames whose steps add up to far more than 2^31 / 64 per row"""
    a, b, ref = _pool(model, 1, 8192), _pool(model, 1, 8192), gh.Reference(1)
    pr = gh.params(hold=5000, attack=3, release=6000)
    rec = ax.gate_design(pr, 48000.0)
    assert rec.hold == 5000
    a.set_gate(pr)
    ref.set(0, rec)
    x = (np.random.RandomState(51).uniform(-0.004, 0.004, (1, 8192))).astype(np.float32)
    x[0, 700] = 0.5                                             # one trigger: open for 5000 frames, then the release ramp to the block's end
    x[0, 7900] = 0.05                                           # a close-level sample while closed: ignored
    want_in = ref.process(x)
    st = ref.state()
    assert st["hold_left"][0] == 0 and 0 < st["atten"][0] < P
    assert same(a.process(x), b.process(want_in))
    assert a.read_gate().tobytes() == st.tobytes()
    y2 = np.ascontiguousarray(x[:, ::-1])
    assert same(a.process(y2), b.process(ref.process(y2))) and a.read_gate().tobytes() == ref.state().tobytes()
    a.close()
    b.close()
