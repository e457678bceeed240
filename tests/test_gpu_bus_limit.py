"""The bus limiters and bus meters on the GPU (-m gpu): after every pass the bus block and the bus meter records are, bit for bit, what the
numpy restatement (tests/limithelp.py: explicit windows, not the kernel's algorithm) makes of the raw bus block that k_mix produced for
that pass. The raw block is a twin pool's, one with the same sends and no limiter stage, whose stream block must be the pool's own. The
buses are driven by disabled streams (a disabled stream's row is its raw input), so the bus samples are chosen frame by frame: a sample
at the ceiling, one ulp above it, peaks at four times the ceiling, 1e6 times, 3e38, NaN and Inf; tests/test_bus_limit_host.py holds
those inputs to the condition that every limiter acts on them. No tolerance anywhere.

Shapes: an LSTM-16 model and the ragged block plan of tests/test_gpu_mix.py (1, 3, 0, 63, 64, 65, 257, 4, twice: every tail around the
kernel's tile of 256 frames, the window and the ring crossing block cuts)."""
import ctypes as C
import importlib

import numpy as np
import pytest

from tests import conftest, gatehelp as gh, limithelp as lh, modelgen

pytestmark = pytest.mark.gpu
ax = importlib.import_module("aidadsp-lv2_amd")

ERR_ARG, ERR_STATE = -1, -6
PLAN, MAXF, T = lh.PLAN, lh.MAXF, lh.T
f32 = np.float32


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def same(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def params(db, L, H):
    return ax.BusLimitParams(db, lh.ms(L), lh.ms(H))


def rec_of(db, L, H):
    r = ax.bus_limit_design(params(db, L, H), 48000.0)
    assert (r.lookahead, r.hold, r.on) == (L, H, 1)
    return f32(r.ceiling), L, H


def ceiling(db):
    return rec_of(db, 1, 0)[0]


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    p = str(tmp_path_factory.mktemp("limit") / "lstm16.json")
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
    """a pool with buses and the limiter stage, its twin with the same buses and sends and no stage, and the restatement"""

    def __init__(self, model, S, B, caps, max_frames=MAXF, disabled=()):
        self.pool, self.twin = _pool(model, S, max_frames, B, disabled), _pool(model, S, max_frames, B, disabled)
        self.pool.set_bus_limiting(True, *caps)
        self.ref, self.S, self.B = lh.Reference(B), S, B
        assert self.pool.bus_limiting and not self.twin.bus_limiting

    def both(self):
        return self.pool, self.twin

    def send(self, stream, send, bus, gain=1.0, ramp=0):
        for p in self.both():
            p.set_send(stream, send, bus, gain, ramp)

    def limiter(self, bus, rec):
        """rec: (ceiling_db, L, H) or None"""
        self.pool.set_bus_limiter(None if rec is None else params(*rec), bus)
        self.ref.set(bus, None if rec is None else rec_of(*rec))

    def expect(self, raw, what=""):
        """the pool's bus block against the restatement over the raw block `raw` of the pass just issued"""
        got, want = self.pool.read_buses(), self.ref.process(raw)
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

    def check_meters(self, what=""):
        got, want = self.pool.read_bus_meters(), self.ref.read_meters()
        assert got.tobytes() == want.tobytes(), (what, got, want)
        return got

    def close(self):
        self.pool.close()
        self.twin.close()


def _case_input(db, model_rows=2, seed=50):
    """three chosen rows around the ceiling of `db` and `model_rows` rows of an ordinary signal for streams that play the model"""
    C_ = ceiling(db)
    rows = [lh.signal(C_, lh.SEEDS[b], kind=lh.KINDS[b]) for b in range(3)]
    return np.ascontiguousarray(np.vstack(rows + list(modelgen.signal(model_rows, T, seed=seed))), f32), C_


@pytest.mark.parametrize("case", [c[0] for c in lh.CASES])
def test_bit_for_bit(model, case):
    _, db, recs, caps = next(c for c in lh.CASES if c[0] == case)
    S, B = 5, 3
    r = Rig(model, S, B, caps, disabled=(0, 1, 2))
    for b in range(B):
        r.send(b, 0, b, 1.0)
        r.limiter(b, (db, *recs[b]))
        p, on, latency = r.pool.bus_limiter(b)
        assert on and latency == recs[b][0] and (p.ceiling_db, p.lookahead_ms) == (db, f32(lh.ms(recs[b][0])))
    x, C_ = _case_input(db)
    outs, last = [], None
    for k, blk in enumerate(_cuts(x, PLAN)):
        y, got, raw = r.process(blk, f"{case} pass {k}")
        if blk.shape[1] == 0:
            assert same(got, last)                               # a pass of no frames limits nothing: the last block stands
        else:
            fin = np.isfinite(blk[:B])
            assert np.array_equal(bits(raw)[fin], bits(blk[:B])[fin]) and not np.isfinite(raw[~fin]).any()      # the raw block is the chosen one
            outs.append(got)
        r.check_meters(f"{case} pass {k}")
        last = got
    out = np.concatenate(outs, axis=1)
    m = r.check_meters()
    assert np.isfinite(out).all() and (np.abs(out) <= C_).all()
    for b in range(B):                                           # every limiter acted, and not everywhere
        assert 0 < m["limited"][b] < T == m["frames"][b] and (np.abs(out[b]) == C_).any() and m["out_peak"][b] == C_ and m["min_gain"][b] < 1
    assert m["in_nonfinite"][1] == (~np.isfinite(x[1])).sum() > 0 and m["in_nonfinite"][0] == 0 and m["passes"][0] == sum(1 for n in PLAN if n)
    r.close()


def test_mixed_records_on_one_launch(model):
    """70 buses, 12 disabled streams: every look-ahead with every hold, five ceilings, every fifth limiter off, 22 empty buses (on and off)"""
    S, B = lh.MIXED_S, lh.MIXED_B
    r = Rig(model, S, B, (512, 4096), disabled=range(S))
    for b, stream, send, rec in lh.mixed_layout():
        if stream is not None:
            r.send(stream, send, b, 1.0)
        r.limiter(b, rec)
    x = np.ascontiguousarray(np.vstack([lh.mixed_signal(s, ceiling) for s in range(S)]), f32)
    outs = []
    for k, blk in enumerate(_cuts(x, [257, 257, 1, 63, 0, 257, 79])):
        _, got, _ = r.process(blk, f"pass {k}")
        if blk.shape[1]:
            outs.append(got)
    out = np.concatenate(outs, axis=1)
    m = r.check_meters()
    for b, xb, rec in lh.mixed_buses(ceiling):
        if xb is None:
            assert not out[b].any() and m["limited"][b] == 0 and m["min_gain"][b] == 1 and m["frames"][b] == T
        elif rec is None:
            assert m["limited"][b] == 0 and m["min_gain"][b] == 1 and m["out_peak"][b] == m["in_peak"][b] == f32(3e38)
        else:
            assert 0 < m["limited"][b] < T and (np.abs(out[b]) == rec[0]).any() and (np.abs(out[b]) <= rec[0]).all()
    r.close()


def test_cuts_do_not_show(model):
    _, db, recs, caps = lh.CASES[1]
    B = 3
    x, C_ = _case_input(db)
    whole, cut = Rig(model, 3, B, caps, max_frames=T, disabled=(0, 1, 2)), Rig(model, 3, B, caps, disabled=(0, 1, 2))
    for r in (whole, cut):
        for b in range(B):
            r.send(b, 0, b, 1.0)
            r.limiter(b, (db, *recs[b]))
    x = np.ascontiguousarray(x[:3])
    _, one, _ = whole.process(x, "one block")
    pieces = [cut.process(blk, f"pass {k}")[1] for k, blk in enumerate(_cuts(x, PLAN)) if blk.shape[1]]
    assert same(np.concatenate(pieces, axis=1), one)
    for b in range(B):
        assert same(one[b], lh.limit(x[b], C_, *recs[b])[0])
    a, c = whole.check_meters(), cut.check_meters()
    for field in ("frames", "in_nonfinite", "limited", "in_peak", "out_peak", "min_gain"):
        assert a[field].tobytes() == c[field].tobytes(), field
    assert list(a["passes"]) == [1] * B and list(c["passes"]) == [sum(1 for n in PLAN if n)] * B
    whole.close()
    cut.close()


def test_a_bus_under_its_ceiling_keeps_its_bits(model):
    S, B = 2, 2
    r = Rig(model, S, B, (64, 100), disabled=(0,))
    r.send(0, 0, 0, 1.0)
    r.send(0, 1, 1, 0.5)
    r.limiter(0, (-3.0, 64, 100))
    r.limiter(1, (-3.0, 7, 0))
    C_ = ceiling(-3.0)
    x = np.ascontiguousarray(np.vstack([lh.signal(C_, 77, kind="quiet"), modelgen.signal(1, T, seed=51)[0]]), f32)
    x[0, 17], x[0, 40] = -C_, f32(1e-41)                         # at the ceiling is not beyond it; a denormal stays one
    gots, raws = [], []
    for k, blk in enumerate(_cuts(x, PLAN)):
        _, got, raw = r.process(blk, f"pass {k}")
        if blk.shape[1]:
            gots.append(got)
            raws.append(raw)
    got, raw = np.concatenate(gots, axis=1), np.concatenate(raws, axis=1)
    for b, L in ((0, 64), (1, 7)):
        assert same(got[b, L:], raw[b, :-L]) and not got[b, :L].any()
    assert same(raw[0], x[0]) and np.abs(raw[0]).max() == C_
    m = r.check_meters()
    assert list(m["limited"]) == [0, 0] and list(m["min_gain"]) == [1, 1] and m["out_peak"][0] == C_ == m["in_peak"][0]
    r.close()


def test_an_off_bus_returns_the_raw_bits(model):
    S, B = 2, 2
    r = Rig(model, S, B, (64, 0), disabled=(0, 1))
    C_ = ceiling(-6.0)
    r.send(0, 0, 0, 1.0)
    r.send(1, 0, 1, 1.0)
    r.limiter(1, (-6.0, 64, 0))
    assert r.pool.bus_limiter(0)[1:] == (False, 0) and r.pool.bus_limiter(1)[1:] == (True, 64)
    x = np.ascontiguousarray(np.vstack([lh.signal(C_, 61, kind="wild"), lh.signal(C_, 62, kind="wild")]), f32)
    n_bad = 0
    for k, blk in enumerate(_cuts(x, PLAN)):
        _, got, raw = r.process(blk, f"pass {k}")
        if blk.shape[1]:
            assert same(got[0], raw[0]) and np.array_equal(np.isnan(got[0]), np.isnan(blk[0])) and np.array_equal(np.isinf(got[0]), np.isinf(blk[0]))
            assert np.isfinite(got[1]).all()
            n_bad += int((~np.isfinite(blk[0])).sum())
    m = r.check_meters()
    assert m["in_nonfinite"][0] == n_bad > 20 and m["limited"][0] == 0 and m["min_gain"][0] == 1 and m["out_peak"][0] == m["in_peak"][0] == f32(3e38)
    assert m["limited"][1] > 0
    r.close()


def test_a_change_of_record_between_passes(model):
    """off -> on, another look-ahead (another delay), another ceiling, another hold, on -> off -> on: each pass is evaluated with the
    record in force when it was issued, over the whole history, the frames mixed under an older record (or none) included"""
    S, B = 3, 2
    r = Rig(model, S, B, (512, 100), disabled=(0, 1))
    r.send(0, 0, 0, 1.0)
    r.send(1, 0, 1, 1.0)
    r.limiter(1, (-6.0, 64, 1))                                  # (the neighbour keeps its record throughout)
    C_ = ceiling(-6.0)
    x = np.ascontiguousarray(np.vstack([lh.signal(C_, 71), lh.signal(C_, 72, kind="wild"), modelgen.signal(1, T, seed=52)[0]]), f32)
    changes = {3: (-6.0, 64, 0), 6: (-6.0, 7, 0), 9: (-12.0, 7, 100), 11: None, 12: (-6.0, 64, 0), 14: (-6.0, 512, 100), 15: (-6.0, 1, 0)}
    for k, blk in enumerate(_cuts(x, PLAN)):
        if k in changes:
            r.limiter(0, changes[k])
            assert r.pool.bus_limiter(0)[1:] == ((True, changes[k][1]) if changes[k] else (False, 0))
        r.process(blk, f"pass {k}")
        r.check_meters(f"pass {k}")
    assert r.ref.read_meters()["limited"][0] > 0
    r.close()


class _DeviceBlock:
    """a view of device memory for torch.as_tensor (the bus block belongs to the pool)"""

    def __init__(self, ptr, shape):
        self.__cuda_array_interface__ = {"shape": shape, "typestr": "<f4", "data": (ptr, False), "version": 2}


def test_every_path_next_to_a_gate_meters_and_an_ir(model):
    """process, process_device on a caller's stream, submit / collect, process_buses, the buses off and on again, the stage off and on
    again: the bus block is always the restatement's over the twin's raw block, the stream block the twin's"""
    import torch
    S, B, n = 6, 3, 65
    r = Rig(model, S, B, (64, 100), max_frames=n, disabled=(0, 1, 2))
    for p in r.both():
        p.set_ir(np.array([0.5, 0.25, -0.125], f32))
        p.set_metering(True)
        p.set_gate(gh.params(**gh.SETS[0]), 4)
    for s in range(S):
        r.send(s, 0, s % B, 1.0 if s < 3 else 0.25)
    for b, rec in enumerate(((-20.0, 64, 100), (-20.0, 3, 0), (-26.0, 33, 7))):
        r.limiter(b, rec)
    C_ = ceiling(-20.0)
    x = np.ascontiguousarray(np.vstack([lh.signal(C_, 80 + s, n=16 * n) for s in range(3)] + list(gh.signal(3, 16 * n, seed=53))), f32)
    x[:3, 5::50] = f32(3.0) * C_                                 # (a peak in every block)
    blocks = iter(_cuts(x, [n, 64, n, 33, n, n, n, n, 64, n, n, n]))
    fp = C.POINTER(C.c_float)

    r.process(next(blocks), "process")
    r.process(next(blocks), "process, 64 frames")

    # process_device on a caller's stream; the bus block is read on that stream
    stream, d_bus = torch.cuda.Stream(), r.pool.buses_device
    blk = next(blocks)
    want_y = r.twin.process(blk)
    d_x = torch.from_numpy(blk).cuda()
    d_y = torch.empty_like(d_x)
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        r.pool.process_device(d_x.data_ptr(), d_y.data_ptr(), n, stream.cuda_stream)
        on_stream = torch.as_tensor(_DeviceBlock(d_bus, (B, n)), device="cuda").clone()
    stream.synchronize()
    assert same(d_y.cpu().numpy(), want_y) and same(d_x.cpu().numpy(), blk)
    assert same(on_stream.cpu().numpy(), r.expect(r.twin.read_buses(), "process_device"))

    # submit / collect with two blocks in flight, a record changed between them: one bus block, the last block's
    b1, b2 = next(blocks), next(blocks)
    r.pool.submit(b1)
    r.limiter(1, (-20.0, 5, 1))
    r.pool.submit(b2)
    y1, y2 = r.pool.collect(b1.shape[1]), r.pool.collect(b2.shape[1])
    r.ref.set(1, rec_of(-20.0, 3, 0))                            # (the restatement follows block by block)
    assert same(y1, r.twin.process(b1))
    r.ref.process(r.twin.read_buses())
    r.ref.set(1, rec_of(-20.0, 5, 1))
    assert same(y2, r.twin.process(b2))
    r.expect(r.twin.read_buses(), "submit / collect")

    # process_buses downloads the limited block
    blk = next(blocks)
    got = r.pool.process_buses(blk)
    r.twin.process(blk)
    assert same(got, r.expect(r.twin.read_buses(), "process_buses"))

    # the buses off: nothing is mixed or limited, the bus block and the bus meters stay; on again, the history goes on from where it was
    before, meters = r.pool.read_buses(), r.check_meters("before off")
    for p in r.both():
        p.set_buses(0)
    blk = next(blocks)
    assert same(r.pool.process(blk), r.twin.process(blk)) and same(r.pool.read_buses(), before)
    assert r.pool.read_bus_meters().tobytes() == meters.tobytes() and r.pool.bus_limiting
    for p in r.both():
        p.set_buses(B)
    r.process(next(blocks), "buses on again")

    # the stage off: the bus block is the raw one again and the history does not move; on again with the same capacities
    r.pool.set_bus_limiting(False)
    assert not r.pool.bus_limiting
    blk = next(blocks)
    assert same(r.pool.process(blk), r.twin.process(blk)) and same(r.pool.read_buses(), r.twin.read_buses())
    assert same(r.pool.process_buses(blk), r.twin.process_buses(blk))
    r.limiter(2, (-20.0, 64, 0))                                 # a host record, on or off
    r.pool.set_bus_limiting(True, 64, 100)
    for k in range(3):
        r.process(next(blocks), f"stage on again, pass {k}")
    m = r.check_meters("the end")
    assert (m["limited"] > 0).all()
    assert r.pool.read_meters().tobytes() == r.twin.read_meters().tobytes() and r.pool.read_gate().tobytes() == r.twin.read_gate().tobytes()
    r.close()


def test_a_prefix_pass(model):
    """the hub's pass over the first n_active streams only, which no public call reaches on a pool with buses (the test build's
    aidax_test_process_prefix does): k_mix leaves the other streams' entries out, the limiters run over every bus, and the history
    goes on through it"""
    if conftest.SHIP_LEG:
        pytest.skip("aidax_test_process_prefix: a test hook — the shipped library has none")
    import torch
    S, B, n = 6, 3, 65
    r = Rig(model, S, B, (64, 100), max_frames=n, disabled=(0, 1, 2))
    for s in range(S):
        r.send(s, 0, s % B, 1.0 if s < 3 else 0.25)
    for b, rec in enumerate(((-20.0, 64, 100), (-20.0, 3, 0), (-26.0, 33, 7))):
        r.limiter(b, rec)
    C_ = ceiling(-20.0)
    x = np.ascontiguousarray(np.vstack([lh.signal(C_, 85 + s, n=4 * n) for s in range(3)] + list(gh.signal(3, 4 * n, seed=54))), f32)
    x[:3, 5::50] = f32(3.0) * C_
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
        assert same(ys[0], ys[1]) and not ys[0][n_active:].any() and same(ys[0][0], blk[0])      # the rows left out are not written
        raw = r.twin.read_buses()
        if n_active == 1:
            assert not raw[1:].any()                             # buses 1 and 2 have lost all their entries: silence goes through their limiters
        r.expect(raw, f"a prefix pass of {n_active} streams")
        r.check_meters(f"a prefix pass of {n_active} streams")
    r.process(blocks[3], "a whole pass behind them")
    assert (r.check_meters()["limited"] > 0).all()
    r.close()


def test_read_bus_meters_with_and_without_clear(model):
    S, B = 3, 3
    r = Rig(model, S, B, (64, 0), max_frames=64, disabled=(0, 1, 2))
    C_ = ceiling(-6.0)
    for b in range(B):
        r.send(b, 0, b, 1.0)
        r.limiter(b, (-6.0, 8 * (b + 1), 0))
    x = np.ascontiguousarray(np.vstack([lh.signal(C_, 90 + b, n=256) for b in range(B)]), f32)
    x[:, 20::64] = f32(2.0) * C_
    blocks = list(_cuts(x, [64] * 4))
    cleared = np.zeros(1, lh.METER_DTYPE)
    cleared["min_gain"] = 1.0
    assert r.pool.read_bus_meters().tobytes() == np.repeat(cleared, B).tobytes()                 # as allocated: cleared
    r.process(blocks[0])
    r.process(blocks[1])
    first = r.check_meters("no clear")
    assert (first["frames"] == 128).all() and (first["passes"] == 2).all() and (first["limited"] > 0).all() and (first["min_gain"] == 0.5).all()
    assert r.check_meters("no clear, again").tobytes() == first.tobytes()
    assert r.pool.read_bus_meters(1, 1, clear=True).tobytes() == first[1:2].tobytes()            # the copy is the record before the clear
    r.ref.meters[1] = cleared[0]
    after = r.check_meters("bus 1 cleared")
    assert after[1].tobytes() == cleared.tobytes() and after[0].tobytes() == first[0].tobytes()
    r.process(blocks[2])
    assert r.check_meters("a pass behind the clear")["frames"].tolist() == [192, 64, 192]
    assert r.pool.read_bus_meters(clear=True).tobytes() == r.ref.read_meters(clear=True).tobytes()
    assert r.check_meters("all cleared").tobytes() == np.repeat(cleared, B).tobytes()
    r.process(blocks[3])
    r.check_meters("the history is not cleared with the meters")
    r.close()


ALLOC = {"hipMalloc", "hipHostMalloc", "hipHostRegister", "hipEventCreateWithFlags", "hipStreamCreateWithFlags", "hipStreamCreateWithPriority"}
FREE = {"hipFree", "hipHostFree", "hipHostUnregister", "hipEventDestroy", "hipStreamDestroy"}
WAIT = {"hipStreamSynchronize", "hipEventSynchronize", "hipDeviceSynchronize", "hipMemcpy"}


def test_the_calls_of_a_pass(model):
    """counted by the test build's table of the pool's HIP calls: with the stage on a pass adds exactly one launch of k_bus_limit and,
    behind a changed record only, one upload; only the first enabling call allocates; set_bus_limiter is a host record; with the stage
    off a pass makes exactly the calls of a pool that has only buses"""
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
    p.set_bus_limiting(False, 64, 100)                          # off before any on: nothing at all
    assert calls() == {} and not p.bus_limiting
    p.set_bus_limiting(True, 64, 100)                           # set-up side: side block, rings, records, meters; the staging and four snapshots
    c = calls()
    assert c.get("hipMalloc") == 4 and c.get("hipHostMalloc") == 5 and c.get("hipEventCreateWithFlags") == 4, c
    p.set_bus_limiting(True, 64, 100)
    p.set_bus_limiting(False, 0, 0)
    p.set_bus_limiting(True, 64, 100)
    assert calls() == {} and p.bus_limiting, "only the first enabling call allocates"
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
    # (stage on?, a record set ahead of the pass?, frames, k_bus_limit launches, record uploads)
    for on, change, frames, launches, uploads in ((True, False, n, 1, 0), (True, True, n, 1, 1), (True, False, 100, 1, 0), (True, True, 0, 0, 0), (True, False, n, 1, 1),
                                                 (False, True, n, 0, 0), (False, False, 64, 0, 0), (True, False, n, 1, 1), (True, False, n, 1, 0)):
        p.set_bus_limiting(on, 64, 100)
        if change:
            p.set_bus_limiter(params(-6.0, 64, 100))
            p.set_bus_limiter(None, 2)
        assert calls() == {}, "set_bus_limiting after the first call and set_bus_limiter are host records"
        base = pass_(plain, frames)
        c = pass_(p, frames)
        assert not {k: v for k, v in c.items() if k in ALLOC | FREE | WAIT}, (on, frames, c)
        extra = {k: c.get(k, 0) - base.get(k, 0) for k in set(c) | set(base) if c.get(k, 0) != base.get(k, 0)}
        want = {"launch_bus_limit": launches} if launches else {}
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

    # before aidax_pool_set_buses
    assert code(p.set_bus_limiting, True, 64, 0) == ERR_STATE and code(p.set_bus_limiting, False, 64, 0) == ERR_STATE and not p.bus_limiting
    assert code(p.bus_limiter, 0) == ERR_ARG
    p.set_buses(B)
    # before the stage's first enabling
    assert code(p.set_bus_limiter, params(-6.0, 8, 0)) == ERR_STATE and code(p.set_bus_limiter, None, 0) == ERR_STATE and code(p.read_bus_meters) == ERR_STATE
    pr, on, latency = p.bus_limiter(0)
    assert (pr.ceiling_db, pr.lookahead_ms, pr.hold_ms, on, latency) == (0.0, 0.0, 0.0, False, 0)
    p.set_bus_limiting(False, 0, 0)                              # off before any on: nothing to do, whatever the capacities
    for caps in ((0, 0), (513, 0), (64, 4097), (0xFFFFFFFF, 0)):
        assert code(p.set_bus_limiting, True, *caps) == ERR_ARG, caps
    assert not p.bus_limiting and code(p.read_bus_meters) == ERR_STATE
    p.set_bus_limiting(True, 64, 100)
    assert p.bus_limiting
    for caps in ((65, 100), (64, 99), (512, 4096)):
        assert code(p.set_bus_limiting, True, *caps) == ERR_STATE, caps
    p.set_bus_limiting(True, 64, 100)                            # the same capacities again: fine
    p.set_bus_limiting(False, 1, 1)
    assert not p.bus_limiting
    p.set_bus_limiting(True, 64, 100)
    # refused records change nothing
    p.set_bus_limiter(params(-6.0, 64, 100), 1)
    p.set_bus_limiter(params(0.0, 1, 0), 2)

    def state():
        return [(q.ceiling_db, q.lookahead_ms, q.hold_ms, on, lat) for q, on, lat in (p.bus_limiter(b) for b in range(B))]

    before = state()
    assert [s[3:] for s in before] == [(False, 0), (True, 64), (True, 1)]
    for bus, pr in ((B, params(-6.0, 8, 0)), (-2, params(-6.0, 8, 0)), (B, None), (0, params(-6.0, 65, 0)), (ax.ALL_BUSES, params(-6.0, 64, 101)),
                    (1, params(float("nan"), 8, 0)), (1, params(13.0, 8, 0)), (ax.ALL_BUSES, params(-6.0, 0, 0)), (2, ax.BusLimitParams(-6.0, 1.0, float("inf")))):
        assert code(p.set_bus_limiter, pr, bus) == ERR_ARG, bus
    assert state() == before and code(p.bus_limiter, B) == ERR_ARG
    # reads
    for first, count in ((0, 0), (2, 2), (3, 1), (0, 4), (0xFFFFFFFF, 2)):
        assert code(p.read_bus_meters, first, count) == ERR_ARG, (first, count)
    assert L.aidax_pool_read_bus_meters(p.h, 0, B, None, 0) == ERR_ARG
    assert L.aidax_pool_bus_limiter(p.h, 1, None, None, None) == 0
    x = modelgen.signal(S, 64, seed=42)
    twin = _pool(model, S, 64, B)
    assert same(p.process(x), twin.process(x))
    m = p.read_bus_meters()
    assert m["frames"].tolist() == [64] * B and m["passes"].tolist() == [1] * B
    p.set_bus_limiter(None)                                      # every limiter off: the raw bits again
    p.set_send(0, 0, 0, 1.0)
    twin.set_send(0, 0, 0, 1.0)
    assert same(p.process(x), twin.process(x)) and same(p.read_buses(), twin.read_buses())
    assert [s[3:] for s in state()] == [(False, 0)] * B
    p.close()
    twin.close()
