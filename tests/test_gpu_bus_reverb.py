"""The bus reverbs on the GPU (-m gpu): after every pass the bus block is, bit for bit, what the numpy restatement (tests/reverbhelp.py:
frame by frame, not the kernel's chunks) makes of the raw bus block that k_mix produced for that pass. The raw block is a twin pool's,
one with the same sends and no reverb stage, whose stream block must be the pool's own. The buses are driven by disabled streams (a
disabled stream's row is its raw input), so the bus samples are chosen frame by frame; one bus carries NaN, +-Inf, 3e38 and 1e6.
tests/test_bus_reverb_host.py holds those inputs to the conditions that every reverb sounds, every ring row wraps twice and the
feedback goes round eight times. No tolerance anywhere.

Shapes: an LSTM-16 model and the ragged block plan 1, 3, 0, 63, 64, 65, 257, 4, repeated (every tail around the kernel's chunks of 64,
128, 192 and 256 frames; records with m_min = 64, 65, 255, 256 and 257 sit on the switches between them)."""
import ctypes as C
import importlib

import numpy as np
import pytest

from tests import conftest, gatehelp as gh, limithelp as lh, modelgen, reverbhelp as rh

pytestmark = pytest.mark.gpu
ax = importlib.import_module("aidadsp-lv2_amd")

ERR_ARG, ERR_STATE = -1, -6
MAXF = rh.MAXF
f32 = np.float32


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def same(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def to_c(rec):
    return ax.BusReverbRec((C.c_uint32 * 8)(*rec.m), (C.c_float * 8)(*[float(g) for g in rec.gq]), float(rec.a), float(rec.wet), float(rec.dry), 0, 0)


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    p = str(tmp_path_factory.mktemp("reverb") / "lstm16.json")
    modelgen.write_model(modelgen.make_model(kind="lstm", hidden=16, input_size=1, seed=5), p)
    return ax.Model(p)


def _pool(model, S, max_frames, buses, disabled=()):
    p = ax.Pool(S, max_frames)
    p.set_model(model)
    p.set_buses(buses)
    for s in disabled:
        p.set_controls(ax.default_controls(enabled=0.0), s)
    return p


def _cuts(x, plan):
    at = 0
    for n in plan:
        yield np.ascontiguousarray(x[:, at:at + n])
        at += n


class Rig:
    """a pool with buses and the reverb stage, its twin with the same buses and sends and no stage, and the restatement; limit: the
    limiter capacities, for a pool that has both stages (the twin has neither)"""

    def __init__(self, model, S, B, capacity, max_frames=MAXF, disabled=(), limit=None):
        self.pool, self.twin = _pool(model, S, max_frames, B, disabled), _pool(model, S, max_frames, B, disabled)
        self.pool.set_bus_reverbs(True, capacity)
        self.ref, self.S, self.B = rh.Reference(B, capacity), S, B
        self.lim = None
        if limit:
            self.pool.set_bus_limiting(True, *limit)
            self.lim = lh.Reference(B)
        assert self.pool.bus_reverbs and not self.twin.bus_reverbs

    def both(self):
        return self.pool, self.twin

    def send(self, stream, send, bus, gain=1.0, ramp=0):
        for p in self.both():
            p.set_send(stream, send, bus, gain, ramp)

    def reverb(self, bus, rec):
        """rec: a reverbhelp.Rec or None"""
        self.pool.set_bus_reverb_rec(None if rec is None else to_c(rec), bus)
        self.ref.set(bus, rec)

    def reset(self, bus):
        self.pool.reset_bus_reverb(bus)
        self.ref.reset(bus)

    def expect(self, raw, what=""):
        """the pool's bus block against the restatement over the raw block `raw` of the pass just issued"""
        got, want = self.pool.read_buses(), self.ref.process(raw)
        if self.lim:
            want = self.lim.process(want)
        assert same(got, want), f"{what}: a pass of {raw.shape[1]} frames, buses {np.flatnonzero((bits(got) != bits(want)).any(axis=1))}"
        return got

    def process(self, blk, what=""):
        """one blocking pass through both pools: (the stream block, the bus block, the raw bus block)"""
        y = self.pool.process(blk)
        assert same(y, self.twin.process(blk)), f"{what}: the stream block is the twin's"
        raw = self.twin.read_buses()
        if blk.shape[1] == 0:
            return y, self.pool.read_buses(), raw
        return y, self.expect(raw, what), raw

    def close(self):
        self.pool.close()
        self.twin.close()


@pytest.mark.parametrize("case", [c[0] for c in rh.CASES])
def test_bit_for_bit(model, case):
    recs, capacity, plan, xb = rh.case(case)
    B, T = len(recs), sum(plan)
    S = B + 1
    r = Rig(model, S, B, capacity, disabled=range(B))
    for b in range(B):
        r.send(b, 0, b, 1.0)
        r.reverb(b, recs[b])
        _, got, on, since = r.pool.bus_reverb(b)
        assert on and since == 0 and tuple(got.m) == recs[b].m and got.on == 1
    x = np.ascontiguousarray(np.vstack([xb, modelgen.signal(1, T, seed=50)]), f32)
    outs, last = [], None
    for k, blk in enumerate(_cuts(x, plan)):
        y, got, raw = r.process(blk, f"{case} pass {k}")
        if blk.shape[1] == 0:
            assert same(got, last)                               # a pass of no frames reverberates nothing: the last block stands
        else:
            fin = np.isfinite(blk[:B])
            assert np.array_equal(bits(raw)[fin], bits(blk[:B])[fin]) and not np.isfinite(raw[~fin]).any()      # the raw block is the chosen one
            outs.append(got)
        last = got
    out = np.concatenate(outs, axis=1)
    assert out.shape == (B, T) and np.isfinite(out).all() and not np.isfinite(x[1]).all()
    for b in range(B):                                           # every reverb sounded
        dry = recs[b].dry * rh.sanitise(x[b])
        assert 2 * int((bits(out[b]) != bits(dry)).sum()) >= T - min(recs[b].m)
        assert r.pool.bus_reverb(b)[3] == T == r.ref.since[b]
    r.close()


def test_mixed_records_on_one_launch(model):
    """70 buses, 12 disabled streams: m_min on every side of the chunk switches, every fifth reverb off, 22 empty buses (on and off)"""
    S, B = rh.MIXED_S, rh.MIXED_B
    r = Rig(model, S, B, rh.MIXED_CAPACITY, disabled=range(S))
    for b, stream, send, rec in rh.mixed_layout():
        if stream is not None:
            r.send(stream, send, b, 1.0)
        r.reverb(b, rec)
    x = np.ascontiguousarray(np.vstack([rh.mixed_signal(s) for s in range(S)]), f32)
    outs, raws = [], []
    for k, blk in enumerate(_cuts(x, rh.MIXED_PLAN)):
        _, got, raw = r.process(blk, f"pass {k}")
        if blk.shape[1]:
            outs.append(got)
            raws.append(raw)
    out, raw = np.concatenate(outs, axis=1), np.concatenate(raws, axis=1)
    for b, stream, _, rec in rh.mixed_layout():
        if rec is None:
            assert same(out[b], raw[b])
        elif stream is None:
            assert not out[b].any()
        else:
            assert np.isfinite(out[b]).all() and (bits(out[b]) != bits(rec.dry * rh.sanitise(raw[b]))).sum() > out.shape[1] // 2
    r.close()


def test_cuts_do_not_show(model):
    recs, capacity, plan, x = rh.case("edges")
    B, T = len(recs), sum(plan)
    other = [200, 57] * (T // 257 + 1)
    rigs = [Rig(model, B, B, capacity, max_frames=mf, disabled=range(B)) for mf in (T, MAXF, 200)]
    for r in rigs:
        for b in range(B):
            r.send(b, 0, b, 1.0)
            r.reverb(b, recs[b])
    _, one, _ = rigs[0].process(x, "one block")
    for r, p in ((rigs[1], plan), (rigs[2], other)):
        pieces = [r.process(blk, f"pass {k}")[1] for k, blk in enumerate(_cuts(x, p)) if blk.shape[1]]
        assert same(np.concatenate(pieces, axis=1), one)
    for b in range(B):
        assert same(one[b], rh.reverb(x[b], recs[b]))
    for r in rigs:
        r.close()


def test_an_off_bus_returns_the_raw_bits_and_a_dry_one_the_sanitised_input(model):
    S = B = 3
    r = Rig(model, S, B, 128, disabled=range(S))
    for b in range(B):
        r.send(b, 0, b, 1.0)
    base = rh.CASES[0][1][1]
    r.reverb(1, base)
    r.reverb(2, rh.Rec(base.m, base.gq, base.a, 0.0, 1.0))       # wet = 0, dry = 1
    assert [r.pool.bus_reverb(b)[2] for b in range(B)] == [False, True, True]
    plan = rh.PLAN1 * 2
    x = np.ascontiguousarray(np.vstack([rh.signal(61 + b, sum(plan), "wild") for b in range(B)]), f32)
    n_bad = 0
    for k, blk in enumerate(_cuts(x, plan)):
        _, got, raw = r.process(blk, f"pass {k}")
        if blk.shape[1]:
            assert same(got[0], raw[0]) and np.array_equal(np.isnan(got[0]), np.isnan(blk[0])) and np.array_equal(np.isinf(got[0]), np.isinf(blk[0]))
            assert np.isfinite(got[1:]).all() and np.array_equal(got[2], rh.sanitise(blk[2]))
            n_bad += int((~np.isfinite(blk[0])).sum())
    assert n_bad > 10
    r.close()


def test_which_changes_of_record_cut_the_tail(model):
    """another gq / a / wet / dry keeps the memories; another delay, off -> on and reset_bus_reverb start a new epoch: the next m_min
    frames are dry * x, bit for bit, and the restatement agrees throughout. The neighbour keeps its record."""
    S = B = 2
    base, neighbour = rh.CASES[0][1][0], rh.CASES[0][1][1]
    r = Rig(model, S, B, 128, max_frames=300, disabled=range(S))
    for b in range(B):
        r.send(b, 0, b, 1.0)
    r.reverb(0, base)
    r.reverb(1, neighbour)
    m_min = min(base.m)
    n = 300
    moved = tuple(k + 2 for k in base.m)
    # (what happens ahead of the block, the record in force from then on, is the tail cut?)
    steps = [(None, base, False),
             (lambda: r.reverb(0, rh.Rec(base.m, base.gq * f32(0.5), 0.5, 2.0, 0.5)), rh.Rec(base.m, base.gq * f32(0.5), 0.5, 2.0, 0.5), False),
             (lambda: r.reverb(0, rh.Rec(moved, base.gq, base.a, base.wet, base.dry)), rh.Rec(moved, base.gq, base.a, base.wet, base.dry), True),
             (lambda: r.reverb(0, rh.Rec(moved[:7] + (64,), base.gq, base.a, base.wet, base.dry)), rh.Rec(moved[:7] + (64,), base.gq, base.a, base.wet, base.dry), True),
             (lambda: (r.reverb(0, None), r.reverb(0, base)), base, True),
             (lambda: r.reset(0), base, True),
             (lambda: r.reverb(0, base), base, False),                # the same record again: nothing moves
             (lambda: r.reverb(0, None), None, False)]
    x = np.ascontiguousarray(np.vstack([rh.signal(71, n * len(steps)), rh.signal(72, n * len(steps))]), f32)
    issued = 0
    for k, (blk, (change, rec, cut)) in enumerate(zip(_cuts(x, [n] * len(steps)), steps)):
        if change:
            change()
        _, got, raw = r.process(blk, f"block {k}")
        if rec is None:
            assert same(got[0], raw[0]) and r.pool.bus_reverb(0)[2:] == (False, 0)
            continue
        first = (rec.dry * rh.sanitise(raw[0]) + rec.wet * f32(0))[:min(rec.m)]
        assert same(got[0, :min(rec.m)], first) == (cut or k == 0), k
        issued = n if cut or k == 0 else issued + n
        assert r.pool.bus_reverb(0)[2:] == (True, issued), k
        assert r.pool.bus_reverb(1)[2:] == (True, n * (k + 1))
    assert m_min == 64
    r.close()


def test_the_limiters_see_the_reverberated_block(model):
    S = B = 3
    r = Rig(model, S, B, 128, disabled=range(S), limit=(64, 100))
    recs = rh.CASES[0][1]
    for b in range(B):
        r.send(b, 0, b, 1.0)
        r.reverb(b, recs[b] if b else None)                     # bus 0: no reverb, a limiter
    lim = [(-20.0, 64, 100), (-20.0, 3, 0), None]
    for b, rec in enumerate(lim):
        r.pool.set_bus_limiter(None if rec is None else ax.BusLimitParams(rec[0], lh.ms(rec[1]), lh.ms(rec[2])), b)
        if rec is not None:
            d = ax.bus_limit_design(ax.BusLimitParams(rec[0], lh.ms(rec[1]), lh.ms(rec[2])), 48000.0)
            r.lim.set(b, (f32(d.ceiling), d.lookahead, d.hold))
    plan = rh.PLAN1 * 3
    x = np.ascontiguousarray(np.vstack([rh.signal(81 + b, sum(plan), "wild" if b == 1 else "plain") for b in range(B)]), f32)
    for k, blk in enumerate(_cuts(x, plan)):
        r.process(blk, f"pass {k}")
        if blk.shape[1]:
            got, want = r.pool.read_bus_meters(), r.lim.read_meters()
            assert got.tobytes() == want.tobytes(), (k, got, want)
    m = r.pool.read_bus_meters()
    assert (m["limited"][:2] > 0).all() and m["in_peak"][2] > np.abs(rh.sanitise(x[2])).max()      # the meter's input is the reverberated block
    r.close()


class _DeviceBlock:
    """a view of device memory for torch.as_tensor (the bus block belongs to the pool)"""

    def __init__(self, ptr, shape):
        self.__cuda_array_interface__ = {"shape": shape, "typestr": "<f4", "data": (ptr, False), "version": 2}


def _path_rig(model, n):
    S, B = 6, 3
    r = Rig(model, S, B, 128, max_frames=n, disabled=(0, 1, 2))
    for s in range(S):
        r.send(s, 0, s % B, 1.0 if s < 3 else 0.25)
    for b, rec in enumerate(rh.CASES[0][1]):
        r.reverb(b, rec)
    return r


def test_every_path_next_to_a_gate_meters_and_an_ir(model):
    """process, process_device in place on a caller's stream, submit / collect, process_buses, the buses off and on again, the stage off
    and on again: the bus block is always the restatement's over the twin's raw block, the stream block the twin's"""
    import torch
    n = 65
    r = _path_rig(model, n)
    S, B = r.S, r.B
    for p in r.both():
        p.set_ir(np.array([0.5, 0.25, -0.125], f32))
        p.set_metering(True)
        p.set_gate(gh.params(**gh.SETS[0]), 4)
    x = np.ascontiguousarray(np.vstack([rh.signal(90 + s, 16 * n, "wild" if s == 1 else "plain") for s in range(3)] + list(gh.signal(3, 16 * n, seed=53))), f32)
    blocks = iter(_cuts(x, [n, 64, n, 33, n, n, n, n, 64, n, n, n]))

    r.process(next(blocks), "process")
    r.process(next(blocks), "process, 64 frames")

    # process_device in place on a caller's stream; the bus block is read on that stream
    stream, d_bus = torch.cuda.Stream(), r.pool.buses_device
    blk = next(blocks)
    want_y = r.twin.process(blk)
    d_x = torch.from_numpy(blk).cuda()
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        r.pool.process_device(d_x.data_ptr(), d_x.data_ptr(), n, stream.cuda_stream)
        on_stream = torch.as_tensor(_DeviceBlock(d_bus, (B, n)), device="cuda").clone()
    stream.synchronize()
    assert same(d_x.cpu().numpy(), want_y)
    assert same(on_stream.cpu().numpy(), r.expect(r.twin.read_buses(), "process_device"))

    # submit / collect with two blocks in flight, a record changed between them: one bus block, the last block's
    b1, b2 = next(blocks), next(blocks)
    base = rh.CASES[0][1][1]
    changed = rh.Rec(base.m, base.gq, 0.0, 1.0, 0.0)
    r.pool.submit(b1)
    r.pool.set_bus_reverb_rec(to_c(changed), 1)
    r.pool.submit(b2)
    y1, y2 = r.pool.collect(b1.shape[1]), r.pool.collect(b2.shape[1])
    assert same(y1, r.twin.process(b1))
    r.ref.process(r.twin.read_buses())                            # (the restatement follows block by block)
    r.ref.set(1, changed)
    assert same(y2, r.twin.process(b2))
    r.expect(r.twin.read_buses(), "submit / collect")

    # process_buses downloads the reverberated block
    blk = next(blocks)
    got = r.pool.process_buses(blk)
    r.twin.process(blk)
    assert same(got, r.expect(r.twin.read_buses(), "process_buses"))

    # the buses off: nothing is mixed or reverberated, the bus block stays; on again, the memories go on from where they were
    before, since = r.pool.read_buses(), r.pool.bus_reverb(0)[3]
    for p in r.both():
        p.set_buses(0)
    blk = next(blocks)
    assert same(r.pool.process(blk), r.twin.process(blk)) and same(r.pool.read_buses(), before)
    assert r.pool.bus_reverbs and r.pool.bus_reverb(0)[3] == since
    for p in r.both():
        p.set_buses(B)
    r.process(next(blocks), "buses on again")

    # the stage off: the bus block is the raw one again and the memories do not move; on again with the same capacity
    r.pool.set_bus_reverbs(False)
    assert not r.pool.bus_reverbs
    blk = next(blocks)
    assert same(r.pool.process(blk), r.twin.process(blk)) and same(r.pool.read_buses(), r.twin.read_buses())
    assert same(r.pool.process_buses(blk), r.twin.process_buses(blk))
    r.reverb(2, rh.Rec(rh.CASES[0][1][2].m, base.gq, 0.1, 0.3, 1.0))      # a host record, on or off: only the gains change, the tail stays
    r.pool.set_bus_reverbs(True, 128)
    for k in range(3):
        r.process(next(blocks), f"stage on again, pass {k}")
    assert r.pool.read_meters().tobytes() == r.twin.read_meters().tobytes() and r.pool.read_gate().tobytes() == r.twin.read_gate().tobytes()
    r.close()


def test_a_prefix_pass(model):
    """the hub's pass over the first n_active streams only, which no public call reaches on a pool with buses (the test build's
    aidax_test_process_prefix does): k_mix leaves the other streams' entries out, the reverbs run over every bus, and the memories go on
    through it"""
    if conftest.SHIP_LEG:
        pytest.skip("aidax_test_process_prefix: a test hook — the shipped library has none")
    import torch
    n = 65
    r = _path_rig(model, n)
    x = np.ascontiguousarray(np.vstack([rh.signal(95 + s, 4 * n) for s in range(3)] + list(gh.signal(3, 4 * n, seed=54))), f32)
    blocks = list(_cuts(x, [n, n, 33, n]))
    hook = ax.lib().aidax_test_process_prefix
    hook.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32]
    r.process(blocks[0], "a whole pass")
    for k, n_active in ((1, 4), (2, 1)):
        blk, ys = blocks[k], []
        for p in r.both():
            d_x = torch.from_numpy(blk).cuda()
            d_y = torch.zeros_like(d_x)
            torch.cuda.synchronize()
            assert hook(p.h, d_x.data_ptr(), d_y.data_ptr(), blk.shape[1], None, n_active) == 0
            p.sync()
            ys.append(d_y.cpu().numpy())
        assert same(ys[0], ys[1]) and not ys[0][n_active:].any()
        raw = r.twin.read_buses()
        if n_active == 1:
            assert not raw[1:].any()                             # buses 1 and 2 have lost all their entries: their tails sound on into the silence
        got = r.expect(raw, f"a prefix pass of {n_active} streams")
        if n_active == 1:
            assert got[1:].any(axis=1).all()
    r.process(blocks[3], "a whole pass behind them")
    r.close()


ALLOC = {"hipMalloc", "hipHostMalloc", "hipHostRegister", "hipEventCreateWithFlags", "hipStreamCreateWithFlags", "hipStreamCreateWithPriority"}
FREE = {"hipFree", "hipHostFree", "hipHostUnregister", "hipEventDestroy", "hipStreamDestroy"}
WAIT = {"hipStreamSynchronize", "hipEventSynchronize", "hipDeviceSynchronize", "hipMemcpy"}


def test_the_calls_of_a_pass(model):
    """counted by the test build's table of the pool's HIP calls: with the stage on a pass adds exactly one launch of k_bus_reverb and,
    behind a changed record only, one upload; only the first enabling call allocates; set_bus_reverb, set_bus_reverb_rec and
    reset_bus_reverb are host records; with the stage off a pass makes exactly the calls of a pool that has only buses"""
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
    plain, p = _pool(model, S, n, B), _pool(model, S, n, B)
    for q in (plain, p):
        q.set_send(ax.ALL_STREAMS, 0, 1, 0.5, 0)
    calls()
    p.set_bus_reverbs(False, 4096)                               # off before any on: nothing at all
    assert calls() == {} and not p.bus_reverbs
    p.set_bus_reverbs(True, 4096)                                # set-up side: the rings and the records; four snapshots
    c = calls()
    assert c.get("hipMalloc") == 2 and c.get("hipHostMalloc") == 4 and c.get("hipEventCreateWithFlags") == 4, c
    p.set_bus_reverbs(True, 4096)
    p.set_bus_reverbs(False, 0)
    p.set_bus_reverbs(True, 4096)
    assert calls() == {} and p.bus_reverbs, "only the first enabling call allocates"
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
    designed = ax.BusReverbParams(1.0, 1.0, 0.3, 0.5, 1.0, 0)
    # (stage on?, what is set ahead of the pass, frames, k_bus_reverb launches, record uploads)
    for on, change, frames, launches, uploads in ((True, None, n, 1, 0), (True, "params", n, 1, 1), (True, None, 100, 1, 0), (True, "rec", 0, 0, 0), (True, None, n, 1, 1),
                                                 (False, "reset", n, 0, 0), (False, None, 64, 0, 0), (True, None, n, 1, 1), (True, None, n, 1, 0)):
        p.set_bus_reverbs(on, 4096)
        if change == "params":
            p.set_bus_reverb(designed)
            p.set_bus_reverb(None, 2)
        elif change == "rec":
            p.set_bus_reverb_rec(to_c(rh.CASES[1][1][0]), 3)
        elif change == "reset":
            p.reset_bus_reverb()
        assert calls() == {}, "set_bus_reverbs after the first call, set_bus_reverb, set_bus_reverb_rec and reset_bus_reverb are host records"
        base = pass_(plain, frames)
        c = pass_(p, frames)
        assert not {k: v for k, v in c.items() if k in ALLOC | FREE | WAIT}, (on, frames, c)
        extra = {k: c.get(k, 0) - base.get(k, 0) for k in set(c) | set(base) if c.get(k, 0) != base.get(k, 0)}
        want = {"launch_bus_reverb": launches} if launches else {}
        if uploads:
            want.update(hipMemcpyAsync=1, hipEventRecord=1)
        assert extra == want, (on, change, frames, extra, base, c)
    stream.synchronize()
    p.close()
    plain.close()


def test_errors(model):
    S, B = 3, 3
    p = ax.Pool(S, 64)
    p.set_model(model)
    L = ax.lib()

    def code(fn, *a, **kw):
        with pytest.raises(ax.AidaxError) as e:
            fn(*a, **kw)
        return e.value.code

    good = rh.CASES[0][1][0]
    params = ax.BusReverbParams(1.0, 0.05, 0.3, 0.5, 1.0, 0)    # 71 .. 151 frames at 48 kHz
    # before aidax_pool_set_buses
    assert code(p.set_bus_reverbs, True, 128) == ERR_STATE and code(p.set_bus_reverbs, False, 128) == ERR_STATE and not p.bus_reverbs
    assert code(p.bus_reverb, 0) == ERR_ARG
    p.set_buses(B)
    # before the stage's first enabling
    assert code(p.set_bus_reverb, params) == ERR_STATE and code(p.set_bus_reverb, None, 0) == ERR_STATE
    assert code(p.set_bus_reverb_rec, to_c(good), 0) == ERR_STATE and code(p.reset_bus_reverb) == ERR_STATE
    pr, rec, on, since = p.bus_reverb(0)
    assert (pr.rt60_s, pr.size, pr.variant, on, since) == (0.0, 0.0, 0, False, 0) and bytes(rec) == bytes(96)
    p.set_bus_reverbs(False, 0)                                  # off before any on: nothing to do, whatever the capacity
    for cap in (0, 63, 32769, 0xFFFFFFFF):
        assert code(p.set_bus_reverbs, True, cap) == ERR_ARG, cap
    assert not p.bus_reverbs and code(p.reset_bus_reverb) == ERR_STATE
    p.set_bus_reverbs(True, 256)
    assert p.bus_reverbs
    for cap in (255, 257, 64, 32768):
        assert code(p.set_bus_reverbs, True, cap) == ERR_STATE, cap
    p.set_bus_reverbs(True, 256)                                 # the same capacity again: fine
    p.set_bus_reverbs(False, 1)
    assert not p.bus_reverbs
    p.set_bus_reverbs(True, 256)
    # refused records change nothing
    p.set_bus_reverb(params, 1)
    p.set_bus_reverb_rec(to_c(good), 2)
    want = rh.design(1.0, 0.05, 0.3, 0.5, 1.0, 0, 48000.0)
    pr, rec, on, since = p.bus_reverb(1)
    assert on and tuple(rec.m) == want.m and (pr.rt60_s, pr.size, pr.variant) == (1.0, f32(0.05), 0) and np.allclose(np.array(rec.gq, f32), want.gq, rtol=1e-6, atol=0)
    pr, rec, on, since = p.bus_reverb(2)
    assert on and tuple(rec.m) == good.m and pr.rt60_s == 0.0

    def state():
        return [(bytes(q), bytes(rec), on, since) for q, rec, on, since in (p.bus_reverb(b) for b in range(B))]

    def bad(**kw):
        c = to_c(good)
        for k, v in kw.items():
            if isinstance(v, tuple):
                getattr(c, k)[v[0]] = v[1]
            else:
                setattr(c, k, v)
        return c

    before = state()
    assert [s[2] for s in before] == [False, True, True]
    nan = float("nan")
    for bus, rec in ((B, to_c(good)), (-2, to_c(good)), (B, None), (0, bad(m=(3, 257))), (ax.ALL_BUSES, bad(m=(0, 63))), (1, bad(m=(7, 32769))),
                     (1, bad(gq=(0, 0.36))), (1, bad(gq=(5, -0.1))), (2, bad(gq=(2, nan))), (ax.ALL_BUSES, bad(a=0.51)), (0, bad(a=-0.1)), (0, bad(a=nan)),
                     (0, bad(wet=4.5)), (0, bad(dry=-4.5)), (0, bad(wet=nan)), (0, bad(dry=float("inf")))):
        assert code(p.set_bus_reverb_rec, rec, bus) == ERR_ARG, (bus, rec)
    for bus, pr in ((B, params), (-2, params), (B, None), (0, ax.BusReverbParams(1.0, 1.0, 0.3, 0.5, 1.0, 0)),      # (1423 .. 2999 frames: beyond 256)
                    (ax.ALL_BUSES, ax.BusReverbParams(0.05, 0.05, 0.3, 0.5, 1.0, 0)), (1, ax.BusReverbParams(1.0, 0.05, 0.3, 0.5, 1.0, 4)), (2, ax.BusReverbParams(1.0, 0.05, nan, 0.5, 1.0, 0))):
        assert code(p.set_bus_reverb, pr, bus) == ERR_ARG, bus
    for bus in (B, -2, 7):
        assert code(p.reset_bus_reverb, bus) == ERR_ARG
    assert state() == before and code(p.bus_reverb, B) == ERR_ARG
    assert L.aidax_pool_bus_reverb(p.h, 1, None, None, None, None) == 0
    # a pass, then every reverb off: the raw bits again
    x = modelgen.signal(S, 64, seed=42)
    twin = _pool(model, S, 64, B)
    for q in (p, twin):
        q.set_send(0, 0, 1, 1.0)
    assert same(p.process(x), twin.process(x)) and same(p.read_buses()[0], twin.read_buses()[0])
    assert [s[3] for s in state()] == [0, 64, 64]
    p.set_bus_reverb(None)
    assert same(p.process(x), twin.process(x)) and same(p.read_buses(), twin.read_buses())
    assert [s[2:] for s in state()] == [(False, 0)] * B
    p.close()
    twin.close()
