"""The mix buses on the GPU (-m gpu): after every pass aidax_pool_read_buses returns, bit for bit, what the numpy restatement
(tests/mixhelp.py: float32 products and sums in the normative order, fp64 ramp gains) makes of the stream block that same pass returned;
that stream block is a bus-less twin pool's; aidax_pool_stream_send answers as the restatement does. On buses around the group size of
32, on long ones around the rounds of the sixteen-wave launch shape, across block cuts, with a muted send of a stream that plays NaN, on
every path a pass can take, next to every other stage, and off. No tolerance anywhere.

Shapes: an LSTM-16 model and the ragged block plan of tests/test_gpu_gate.py (1, 3, 0, 63, 64, 65, 257, 4: unaligned rows, every tail
around the tile of 64 frames, several tiles); 5 streams where the sends matter, 70 where the entry count does, 128 to 257 where a bus
needs more than one round."""
import ctypes as C
import importlib

import numpy as np
import pytest

from tests import conftest, gatehelp as gh, mixhelp as mh, modelgen

pytestmark = pytest.mark.gpu
ax = importlib.import_module("aidadsp-lv2_amd")

ERR_ARG, ERR_STATE = -1, -6
NONE, ALL = mh.BUS_NONE, mh.ALL_STREAMS
PLAN = [1, 3, 0, 63, 64, 65, 257, 4] * 2
MAXF = 257


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    p = str(tmp_path_factory.mktemp("mix") / "lstm16.json")
    modelgen.write_model(modelgen.make_model(kind="lstm", hidden=16, input_size=1, seed=5), p)
    return ax.Model(p)


def _pool(model, S, max_frames=MAXF, buses=0):
    p = ax.Pool(S, max_frames)
    p.set_model(model)
    if buses:
        p.set_buses(buses)
    return p


def _cuts(x, plan):
    at = 0
    for n in plan:
        yield np.ascontiguousarray(x[:, at:at + n])
        at += n


class Both:
    """a pool with buses and the restatement, told the same things"""

    def __init__(self, model, S, B, max_frames=MAXF):
        self.pool, self.ref, self.S, self.B = _pool(model, S, max_frames, B), mh.Reference(S, B), S, B

    def send(self, stream, send, bus, gain=1.0, ramp=0):
        self.pool.set_send(stream, send, bus, gain, ramp)
        self.ref.set_send(stream, send, bus, gain, ramp)

    def check_sends(self, what=""):
        for s in range(self.S):
            for j in range(mh.SENDS):
                assert self.pool.stream_send(s, j) == self.ref.stream_send(s, j), (what, s, j)

    def process(self, blk, what=""):
        """one pass: (the stream block, the bus block), the bus block checked against the restatement over that stream block"""
        y = self.pool.process(blk)
        got = self.pool.read_buses()
        if blk.shape[1]:
            want = self.ref.mix(y)
            assert same(got, want), f"{what}: a pass of {blk.shape[1]} frames, buses {np.flatnonzero((bits(got) != bits(want)).any(axis=1))}"
        return y, got

    def close(self):
        self.pool.close()


def test_composition(model):
    """five streams, three buses: stream 0 on two buses (one at exactly 1), both sends of stream 1 on one bus, a negative gain, an empty
    bus, a stream without a send"""
    S, B = 5, 3
    m, twin = Both(model, S, B), _pool(model, S)
    assert m.pool.buses == B and twin.buses == 0 and m.pool.kernel_name == twin.kernel_name
    assert m.pool.read_buses().shape == (B, 0)                  # no pass mixed yet
    m.send(0, 0, 0, 0.5)
    m.send(0, 1, 1, 1.0)
    m.send(1, 0, 0, 0.25)
    m.send(1, 3, 0, 0.75)
    m.send(2, 2, 1, -0.5)
    m.send(3, 0, 0, 1.0)
    m.check_sends("set")
    assert m.pool.stream_send(0, 1) == (1, 0.0, 1.0, 1)         # a jump has one frame left until a frame is issued
    x = modelgen.signal(S, sum(PLAN), seed=31)
    last = None
    for k, blk in enumerate(_cuts(x, PLAN)):
        y, got = m.process(blk, f"pass {k}")
        assert same(y, twin.process(blk)), f"pass {k}: the stream block is a bus-less pool's"
        m.check_sends(f"pass {k}")
        if blk.shape[1] == 0:
            assert same(got, last)                              # a pass of no frames mixes nothing: the last block stands
        else:
            assert got.shape == (B, blk.shape[1]) and not got[2].any() and not np.signbit(got[2]).any()      # the empty bus is +0.0
        last = got
    assert m.pool.stream_send(0, 1) == (1, 1.0, 1.0, 0) and last[0].any() and last[1].any()
    assert same(m.pool.read_buses(1, 2), last[1:3]) and same(m.pool.read_buses(2), last[2:])
    m.close()
    twin.close()


def test_one_unity_send_carries_the_streams_bits_with_minus_zero_as_plus_zero(model):
    S = 2
    m = Both(model, S, 1, 64)
    m.pool.set_controls(ax.default_controls(enabled=0.0), 1)    # a disabled stream's row is its raw input, and that is what is summed
    m.send(1, 0, 0, 1.0)
    x = modelgen.signal(S, 64, seed=32)
    x[1, 5] = -0.0
    x[1, 6] = np.float32(1e-41)                                 # a denormal stays one
    y, got = m.process(x)
    assert same(y[1], x[1]) and np.signbit(y[1, 5])
    want = x[1].copy()
    want[5] = 0.0
    assert same(got[0], want)
    m.close()


# pools of 70 streams whose buses have 0, 1, 32, 33, 64, 65, 128, 129 and 140 entries between them (four sends per stream: 592 entries
# do not fit two pools). (bus, [(stream, send), ..]) per layout; 140: sends 0 and 1 of every stream on one bus.
LAYOUTS = {
    "140_128_1_0": [(0, [(s, j) for s in range(70) for j in (0, 1)]), (1, [(s, j) for s in range(64) for j in (2, 3)]), (2, [(69, 2)]), (3, [])],
    "129_65_64": [(0, [(s, j) for s in range(64) for j in (0, 1)] + [(64, 0)]), (1, [(s, 2) for s in range(65)]), (2, [(s, 3) for s in range(64)])],
    "32_33": [(0, [(s, 0) for s in range(32)]), (1, [(s, 1) for s in range(33)])],
    # (the launch shape goes by the longest bus: one wave up to 32 entries, four up to 128, sixteen beyond)
    "128_65_33": [(0, [(s, j) for s in range(64) for j in (0, 1)]), (1, [(s, 2) for s in range(65)]), (2, [(s, 3) for s in range(33)])],
    "32_1_0": [(0, [(s, 2) for s in range(38, 70)]), (1, [(0, 0)]), (2, [])],
}


@pytest.mark.parametrize("layout", sorted(LAYOUTS))
def test_group_edges(model, layout):
    S = 70
    spec = LAYOUTS[layout]
    m = Both(model, S, len(spec))
    i = 0
    for bus, sends in spec:
        for s, j in sends:
            m.send(s, j, bus, float(np.float32(2.0 ** -10 + 0.0067 * i)))      # distinct per entry, in [2^-10, 2]: a wrong order shows
            i += 1
    for bus, sends in spec:
        assert m.ref.entries(bus) == sorted(sends) and layout.split("_")[bus] == str(len(sends))
    x = modelgen.signal(S, sum(PLAN), seed=33)
    for k, blk in enumerate(_cuts(x, PLAN)):
        y, got = m.process(blk, f"{layout} pass {k}")
        if layout.startswith("140") and blk.shape[1] == 257:
            # the restatement on this very block: two entries of the 140-entry bus the other way round change the bus's bits (inside a
            # group, and across two groups), so the comparison above did test the order
            es = m.ref.entries(0)
            for a, b in ((5, 28), (31, 32), (100, 139)):
                swapped = list(es)
                swapped[a], swapped[b] = swapped[b], swapped[a]
                assert not same(m.ref.mix(y, order={0: swapped})[0], got[0]), (a, b)
    m.close()


# The sixteen-wave form's rounds. A plan with a bus of more than 128 entries runs sixteen waves per workgroup, one group each per round:
# 512 entries are 16 groups, the last round that is full; 513 and 516 are 17, a second round of one group, of 1 and of 4 entries (its
# sum goes through the other LDS buffer and meets the first round's behind a second barrier); 1028 are 33, a third round, which writes
# the first round's buffer again. One bus per pool: all four sends of every stream.
LONG = {512: 128, 513: 129, 516: 129, 1028: 257}


@pytest.mark.parametrize("n_entries", sorted(LONG))
def test_a_long_bus_crosses_rounds(model, n_entries):
    S = LONG[n_entries]
    m = Both(model, S, 2)
    sends = [(s, j) for s in range(S) for j in range(mh.SENDS)][:n_entries]
    for i, (s, j) in enumerate(sends):
        m.send(s, j, 0, float(np.float32(2.0 ** -10 + 0.0019 * i)))             # distinct per entry, in [2^-10, 2]
    if n_entries == 513:
        m.send(S - 1, 3, 1, 1.0)                                                # (a second, short bus in the same launch)
    assert m.ref.entries(0) == sends and len(sends) == n_entries
    x = modelgen.signal(S, sum(PLAN), seed=44)
    for k, blk in enumerate(_cuts(x, PLAN)):
        y, got = m.process(blk, f"{n_entries} entries, pass {k}")
        if blk.shape[1] == 257:
            # the restatement on this very block: two entries the other way round change the bus's bits: inside the first round, across
            # the edge of the rounds (the last entry of group 15 and the first of group 16), and inside what lies behind it
            es = m.ref.entries(0)
            for a, b in ((100, 480), (511, 512), (300, n_entries - 1)) + (((512, 1027), (1023, 1024)) if n_entries == 1028 else ()):
                if b >= n_entries or a == b:
                    continue
                swapped = list(es)
                swapped[a], swapped[b] = swapped[b], swapped[a]
                assert not same(m.ref.mix(y, order={0: swapped})[0], got[0]), (a, b)
    m.close()


def _schedule():
    """(frame, stream, send, bus, gain, ramp): a fade-in of 100 frames; a move to another bus; a ramp to 0, then BUS_NONE; a jump; a ramp
    re-targeted mid-way"""
    return [(0, 0, 0, 0, 1.0, 100), (0, 1, 0, 0, 0.5, 0), (150, 0, 0, 1, 0.8, 64), (300, 1, 0, 0, 0.0, 50), (400, 1, 0, NONE, 0.0, 0),
            (400, 2, 1, 1, -0.7, 0), (450, 2, 1, 1, 0.3, 200), (520, 2, 1, 1, 1.5, 30)]


def _run_schedule(model, x, pattern):
    """the schedule through a fresh pool, every stretch between two of its events cut by `pattern` (cyclically): the concatenated stream
    and bus rows, and stream_send's answers behind every event's first pass"""
    S, T = x.shape
    m = Both(model, S, 2)
    events = _schedule()
    marks = sorted({e[0] for e in events} | {T})
    ys, bs, at, i = [], [], 0, 0
    for lo, hi in zip(marks[:-1], marks[1:]):
        for e in events:
            if e[0] == lo:
                m.send(*e[1:])
        m.check_sends(f"events at {lo}")
        while at < hi:
            n = min(pattern[i % len(pattern)], hi - at)
            i += 1
            y, b = m.process(np.ascontiguousarray(x[:, at:at + n]), f"frames {at} .. {at + n}")
            m.check_sends(f"behind frame {at + n}")
            ys.append(y)
            bs.append(b)
            at += n
    m.close()
    return np.concatenate(ys, axis=1), np.concatenate(bs, axis=1)


def test_ramps_do_not_see_block_cuts(model):
    """(three streams: below a full workgroup of four every pass is k_lstm_pipe's, so the stream rows themselves do not depend on the cuts)"""
    x = modelgen.signal(3, 700, seed=34)
    ya, ba = _run_schedule(model, x, [64])
    yb, bb = _run_schedule(model, x, [1, 3, 63, 65, 257, 17])
    assert same(ya, yb), "the stream rows depend on the cuts: the bus rows cannot be compared"
    assert same(ba, bb)
    # the schedule did what it says: silence before the fade-in's first frame has a gain, bus 1 empty until frame 150, stream 1 gone from 349 on
    assert ba[1, :150].any() == False and ba[1, 150:].any() and ba[0, :100].any()      # noqa: E712
    ref = mh.Reference(3, 2)
    ref.set_send(1, 0, 0, 0.5, 0)
    ref.mix(ya[:, :300])
    ref.set_send(1, 0, 0, 0.0, 50)
    g = ref.gains(1, 0, 60)
    assert g[48] != 0 and not g[49:].any()


def test_a_muted_send_is_left_out(model):
    """stream 1 is disabled (its row is the raw input) and fed NaN and Inf; its send is on bus 0 next to stream 0's"""
    S = 3
    m = Both(model, S, 2, 64)
    m.pool.set_controls(ax.default_controls(enabled=0.0), 1)
    m.send(0, 0, 0, 0.5)
    m.send(1, 0, 0, 0.0)                                        # on the bus, muted
    m.send(1, 1, 1, 0.0)
    m.send(2, 0, 1, 1.0)
    x = modelgen.signal(S, 64 * 4, seed=35)
    x[1, 0::3] = np.nan
    x[1, 1::3] = np.inf
    x[1, 2::3] = -np.inf
    blocks = list(_cuts(x, [64] * 4))

    def run(blk, what):
        y = m.pool.process(blk)
        assert gh.same_bits(y[1], blk[1])
        got, want = m.pool.read_buses(), m.ref.mix(y)
        assert np.array_equal(np.isfinite(got), np.isfinite(want)), what
        assert np.array_equal(bits(got)[np.isfinite(want)], bits(want)[np.isfinite(want)]), what
        return got

    got = run(blocks[0], "muted")
    assert np.isfinite(got).all() and got[0].any()
    m.send(1, 0, 0, 1.0, 0)                                     # a jump to 1: non-finite from the first frame on
    got = run(blocks[1], "open")
    assert not np.isfinite(got[0]).any() and np.isfinite(got[1]).all()
    m.send(1, 0, 0, 0.0, 5)                                     # a ramp to 0 over 5 frames: frames 0 .. 3 still carry a gain, frame 4 is 0
    got = run(blocks[2], "closing")
    assert not np.isfinite(got[0, :4]).any() and np.isfinite(got[0, 4:]).all()
    m.send(1, 0, 0, 0.25, 8)                                    # ... and opening: the first frame whose gain is not 0 is the ramp's first
    got = run(blocks[3], "opening")
    assert not np.isfinite(got[0]).any()
    m.check_sends()
    m.close()


def _some_sends(m, S, B):
    for s in range(S):
        m.send(s, 0, s % B, 0.25 + 0.125 * s)
        m.send(s, 2, (s + 1) % B, -0.5 + 0.0625 * s, 1000)


def test_process_buses_is_process_and_read_buses(model):
    S, B = 5, 3
    a, b = Both(model, S, B), Both(model, S, B)
    for m in (a, b):
        _some_sends(m, S, B)
    x = modelgen.signal(S, sum(PLAN), seed=36)
    for k, blk in enumerate(_cuts(x, PLAN)):
        got = a.pool.process_buses(blk)
        _, want = b.process(blk, f"pass {k}")
        assert got.shape == (B, blk.shape[1])
        if blk.shape[1]:
            assert same(got, want), f"pass {k}"
            assert same(a.pool.read_buses(), want)
            a.ref.mix(np.zeros((S, blk.shape[1]), np.float32))  # (a's restatement only follows the ramps)
        a.check_sends(f"pass {k}")
    a.close()
    b.close()


class _DeviceBlock:
    """a view of device memory for torch.as_tensor (the bus block belongs to the pool)"""

    def __init__(self, ptr, shape):
        self.__cuda_array_interface__ = {"shape": shape, "typestr": "<f4", "data": (ptr, False), "version": 2}


def test_process_device_on_the_pools_stream_and_on_a_callers(model):
    import torch
    S, B, n = 5, 3, 65
    m, twin = Both(model, S, B, 65), Both(model, S, B, 65)
    for p in (m, twin):
        _some_sends(p, S, B)
    d_bus = m.pool.buses_device
    assert d_bus and d_bus == m.pool.buses_device
    stream = torch.cuda.Stream()
    x = modelgen.signal(S, n * 4, seed=37)
    for k, blk in enumerate(_cuts(x, [n, n, 33, n])):
        f = blk.shape[1]
        want_y, want_b = twin.process(blk, f"twin pass {k}")
        d_x = torch.from_numpy(blk).cuda()
        d_y = torch.empty_like(d_x)
        torch.cuda.synchronize()
        own = k >= 2                                            # on the pool's stream, then on the caller's
        with torch.cuda.stream(stream):
            m.pool.process_device(d_x.data_ptr(), d_y.data_ptr(), f, stream.cuda_stream if own else 0)
            if own:
                got_b = torch.as_tensor(_DeviceBlock(d_bus, (B, f)), device="cuda").clone()       # ordered on the stream the pass ran on
        if own:
            stream.synchronize()
        else:
            m.pool.sync()
            got_b = torch.as_tensor(_DeviceBlock(d_bus, (B, f)), device="cuda").clone()
            torch.cuda.synchronize()
        assert same(d_y.cpu().numpy(), want_y) and same(d_x.cpu().numpy(), blk), f"pass {k}"
        assert same(got_b.cpu().numpy(), want_b), f"pass {k}"
        assert same(m.pool.read_buses(), want_b), f"pass {k}"
        m.ref.mix(want_y)
        m.check_sends(f"pass {k}")
    m.close()
    twin.close()


def test_submit_and_collect_with_two_blocks_in_flight(model):
    """there is one bus block: after the last collect it holds the last block's mix, under the sends in force when that block was submitted"""
    S, B = 5, 3
    m = Both(model, S, B, 64)
    _some_sends(m, S, B)
    blocks = list(_cuts(modelgen.signal(S, 64 * 2 + 37, seed=38), [64, 64, 37]))
    m.pool.submit(blocks[0])
    m.send(0, 0, 2, 1.0, 10)                                    # between two blocks in flight
    m.pool.submit(blocks[1])
    y0 = m.pool.collect(64)
    m.pool.submit(blocks[2])
    y1, y2 = m.pool.collect(64), m.pool.collect(37)
    ref = mh.Reference(S, B)
    twin = Both(model, S, B, 64)
    twin.ref = ref
    _some_sends(twin, S, B)
    assert same(twin.process(blocks[0])[0], y0)
    twin.send(0, 0, 2, 1.0, 10)
    assert same(twin.process(blocks[1])[0], y1)
    y, want = twin.process(blocks[2])
    assert same(y, y2) and same(m.pool.read_buses(), want) and want.shape == (B, 37)
    m.ref = ref
    m.check_sends()
    m.close()
    twin.close()


def test_next_to_meters_a_gate_an_ir_blend_and_a_model_bank(model, tmp_path_factory):
    """the buses only read: audio and meter records are the bus-less twin's, and the bus block is the restatement's over that audio"""
    S, B = 8, 3
    path = str(tmp_path_factory.mktemp("mix") / "lstm16_b.json")
    modelgen.write_model(modelgen.make_model(kind="lstm", hidden=16, input_size=1, seed=6), path)
    other = ax.Model(path)
    m, twin = Both(model, S, B, 65), _pool(model, S, 65)
    for p in (m.pool, twin):
        p.set_model_slot(1, other)
        p.assign_model(S - 1, 1, ax.START_RESET)
        p.set_ir(np.array([0.5, 0.25, -0.125], np.float32))
        p.set_ir_slot(0, np.array([0.25, -0.5, 0.125, 0.0625], np.float32))
        p.assign_ir_b(2, 0)
        p.set_ir_mix(2, 0.75, 500)                              # mid-ramp through all three passes
        p.set_metering(True)
        p.set_gate(gh.params(**gh.SETS[0]), 1)
    assert "bank" in m.pool.kernel_name and m.pool.kernel_name == twin.kernel_name
    _some_sends(m, S, B)
    for k, blk in enumerate(_cuts(gh.signal(S, 65 + 64 + 65, seed=39), [65, 64, 65])):
        y, _ = m.process(blk, f"pass {k}")
        assert same(y, twin.process(blk)), f"pass {k}"
        assert 0 < m.pool.stream_ir_mix(2)[3] == twin.stream_ir_mix(2)[3]
    assert m.pool.read_meters().tobytes() == twin.read_meters().tobytes()
    assert m.pool.read_gate().tobytes() == twin.read_gate().tobytes()
    m.close()
    twin.close()


def test_off_is_off(model):
    """set_buses(0) after use: no pass is mixed, the bus block stays as it was and ramps do not advance; on again, it goes on from there.
    And a pool with its buses off, like one that never had any, returns a plain pool's bits from the same kernel."""
    S, B = 5, 3
    m, plain = Both(model, S, B), _pool(model, S)
    _some_sends(m, S, B)
    blocks = list(_cuts(modelgen.signal(S, sum(PLAN), seed=40), PLAN))
    for blk in blocks[:5]:
        m.process(blk)
        plain.process(blk)
    before, sends = m.pool.read_buses(), [m.pool.stream_send(s, 2) for s in range(S)]
    assert before.shape == (B, 64) and all(left > 0 for _, _, _, left in sends)       # the ramps of _some_sends are under way
    m.pool.set_buses(0)
    assert m.pool.buses == B
    with pytest.raises(ax.AidaxError) as e:
        m.pool.process_buses(blocks[5])
    assert e.value.code == ERR_STATE
    for blk in blocks[5:8]:
        assert same(m.pool.process(blk), plain.process(blk))
        assert same(m.pool.read_buses(), before)
    assert [m.pool.stream_send(s, 2) for s in range(S)] == sends and m.pool.kernel_name == plain.kernel_name
    m.send(1, 1, 2, 0.5, 3)                                     # a host record, on or off
    m.pool.set_buses(B)
    for blk in blocks[8:]:
        y, _ = m.process(blk)
        assert same(y, plain.process(blk))
    m.check_sends()
    m.close()
    plain.close()


ALLOC = {"hipMalloc", "hipHostMalloc", "hipHostRegister", "hipEventCreateWithFlags", "hipStreamCreateWithFlags", "hipStreamCreateWithPriority"}
FREE = {"hipFree", "hipHostFree", "hipHostUnregister", "hipEventDestroy", "hipStreamDestroy"}
WAIT = {"hipStreamSynchronize", "hipEventSynchronize", "hipDeviceSynchronize", "hipMemcpy"}


def test_the_calls_of_a_pass(model):
    """counted by the test build's table of the pool's HIP calls: a pool that never had buses and one whose buses are off make the same
    calls per pass; with the buses on a pass adds one launch of k_mix and, behind a changed send only, the plan's upload; set_send is a
    host record; nothing allocates, frees or waits"""
    if conftest.SHIP_LEG:
        pytest.skip("aidax_test_hip_calls: a test hook — the shipped library has none")
    import torch
    fn = ax.lib().aidax_test_hip_calls
    fn.argtypes = [C.c_char_p, C.c_uint32]
    fn.restype = C.c_int
    buf = C.create_string_buffer(4096)

    def calls():
        fn(buf, len(buf))
        return {line.split()[0]: int(line.split()[1]) for line in buf.value.decode().splitlines()}

    S, B, n = 70, 4, 256
    plain, p = _pool(model, S, n), _pool(model, S, n)
    calls()
    p.set_buses(0)                                              # off before any on: nothing at all
    assert calls() == {} and p.buses == 0
    p.set_buses(B)                                              # set-up side: the bus block and the plan; the staging and four snapshots
    c = calls()
    assert c.get("hipMalloc") == 2 and c.get("hipHostMalloc") == 5, c
    stream = torch.cuda.Stream()
    d_x = torch.from_numpy(modelgen.signal(S, n, seed=41)).cuda()
    d_y = torch.empty_like(d_x)
    torch.cuda.synchronize()

    def pass_(pool, frames=n):
        with torch.cuda.stream(stream):
            pool.process_device(d_x.data_ptr(), d_y.data_ptr(), frames, stream.cuda_stream)
        return calls()

    for q in (plain, p):
        pass_(q)
    stream.synchronize()
    calls()
    # (buses on?, a send set ahead of the pass?, frames, k_mix launches, plan uploads)
    for on, change, frames, launches, uploads in ((True, False, n, 1, 0), (True, True, n, 1, 1), (True, False, 100, 1, 0), (True, True, 0, 0, 0), (True, False, n, 1, 1),
                                                 (False, True, n, 0, 0), (False, False, 64, 0, 0), (True, False, n, 1, 1), (True, False, n, 1, 0)):
        p.set_buses(B if on else 0)
        if change:
            p.set_send(ax.ALL_STREAMS, 1, 2, 0.5, 1000)
        assert calls() == {}, "set_buses after the first call and set_send are host records"
        base = pass_(plain, frames)
        c = pass_(p, frames)
        assert not {k: v for k, v in c.items() if k in ALLOC | FREE | WAIT}, (on, frames, c)
        extra = {k: c.get(k, 0) - base.get(k, 0) for k in set(c) | set(base) if c.get(k, 0) != base.get(k, 0)}
        want = {"launch_mix": launches} if launches else {}
        if uploads:
            want.update(hipMemcpyAsync=1, hipEventRecord=1)
        assert extra == want, (on, change, frames, extra, base, c)
    stream.synchronize()
    p.close()
    plain.close()


def test_errors(model):
    S, B = 5, 3
    p = _pool(model, S, 64)
    out = np.zeros((B, 64), np.float32)
    fp = C.POINTER(C.c_float)

    def code(fn, *a):
        with pytest.raises(ax.AidaxError) as e:
            fn(*a)
        return e.value.code

    # before aidax_pool_set_buses
    assert p.buses == 0 and p.stream_send(0, 0) == (NONE, 0.0, 0.0, 0)
    assert code(p.set_send, 0, 0, 0, 1.0, 0) == ERR_STATE and code(p.set_send, 0, 0, NONE, 0.0, 0) == ERR_STATE
    assert code(p.read_buses, 0, 1) == ERR_STATE and code(lambda: p.buses_device) == ERR_STATE and code(p.process_buses, np.zeros((S, 8), np.float32)) == ERR_STATE
    assert code(p.set_buses, ax.MAX_BUSES + 1) == ERR_ARG and p.buses == 0
    p.set_buses(0)
    assert p.buses == 0
    p.set_buses(B)
    assert p.buses == B
    assert code(p.set_buses, B + 1) == ERR_STATE and p.buses == B
    p.set_buses(B)                                              # the same count again: fine
    # refused sends change nothing
    p.set_send(1, 2, 1, 0.5, 7)
    state = [p.stream_send(s, j) for s in range(S) for j in range(ax.SENDS)]
    for a in ((S, 0, 0, 1.0, 0), (-2, 0, 0, 1.0, 0), (0, ax.SENDS, 0, 1.0, 0), (0, 0, B, 1.0, 0), (0, 0, -2, 1.0, 0), (ALL, 0, 0, float("nan"), 0),
              (0, 0, 0, float("inf"), 0), (0, 0, 0, 16.5, 0), (ALL, 0, 0, -17.0, 0), (0, 0, 0, 1.0, (1 << 24) + 1), (1, 2, NONE, float("nan"), 0)):
        assert code(p.set_send, *a) == ERR_ARG, a
    assert [p.stream_send(s, j) for s in range(S) for j in range(ax.SENDS)] == state
    assert code(p.stream_send, S, 0) == ERR_ARG and code(p.stream_send, 0, ax.SENDS) == ERR_ARG
    p.set_send(0, 0, 0, 16.0, 1 << 24)                          # the bounds themselves are fine
    p.set_send(0, 0, 0, -16.0, 0)
    # reads
    for first, count in ((0, 0), (2, 2), (3, 1), (0, 4), (0xFFFFFFFF, 2)):
        assert code(p.read_buses, first, count) == ERR_ARG, (first, count)
    p.process(modelgen.signal(S, 64, seed=42))
    L = ax.lib()
    n = C.c_uint32(99)
    assert L.aidax_pool_read_buses(p.h, 0, B, out.ctypes.data_as(fp), B * 64 - 1, C.byref(n)) == ERR_ARG and n.value == 99      # too small a buffer
    assert L.aidax_pool_read_buses(p.h, 0, B, None, B * 64, C.byref(n)) == ERR_ARG
    assert L.aidax_pool_read_buses(p.h, 1, 2, out.ctypes.data_as(fp), 2 * 64, None) == 0
    assert L.aidax_pool_read_buses(p.h, 0, B, out.ctypes.data_as(fp), B * 64, C.byref(n)) == 0 and n.value == 64 and out[0].any()
    assert L.aidax_pool_buses_device(p.h, None) == ERR_ARG and L.aidax_pool_set_buses(None, 1) == ERR_ARG and L.aidax_pool_buses(None) == 0
    x = np.zeros((S, 65), np.float32)
    assert L.aidax_pool_process_buses(p.h, x.ctypes.data_as(fp), out.ctypes.data_as(fp), 65) == ERR_ARG                            # beyond max_frames
    assert L.aidax_pool_process_buses(p.h, None, out.ctypes.data_as(fp), 64) == ERR_ARG
    assert L.aidax_pool_process_buses(p.h, None, None, 0) == 0                                                                       # the pre-run
    # reset_stream keeps sends and running ramps
    p.set_send(2, 1, 1, 0.75, 1000)
    p.process(modelgen.signal(S, 64, seed=43))
    before = p.stream_send(2, 1)
    p.reset_stream(2)
    assert p.stream_send(2, 1) == before and before[3] == 1000 - 64
    p.close()
