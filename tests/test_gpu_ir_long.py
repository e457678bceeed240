"""Cabinet IRs above 8192 taps (GPU, -m gpu): aidax_pool_set_ir_capacity and the stage on a history ring sized for up to 65536 taps.

The bit-for-bit cases run the exact-arithmetic families of tests/irdata.py (A, B, C take any length) the way tests/test_gpu_ir_exact.py
does: a real model with every stream disabled, so the stage's input is the test's input, np.array_equal against a truth computed by
superposition. Each pool's capacity is set to its IR's length, which makes the ring R = the power of two >= L + max_frames, and every
run is longer than 2 R frames: the enlarged ring wraps at least twice. A and C keep to pools of at most 64 streams (their impulses sit
more than L frames apart, so their arrays grow with L). Random IRs are held to fp64 under the project's bound for one convolution,
TAU = 4e-6 per sample against (|h| * |dry|)_t (tests/test_gpu_ir.py), and the fade pass of a 65536-tap IR to tests/irfade.py under the
same bound, as tests/test_gpu_ir_fade.py does."""
import ctypes as C
import importlib

import numpy as np
import pytest

from tests import conftest, errlog, irdata, irfade, modelgen
from tests.test_gpu_ir import TAU, _tau

pytestmark = pytest.mark.gpu
ax = importlib.import_module("aidadsp-lv2_amd")
ERR_ARG, ERR_STATE = -1, -6

RAGGED = [1, 17, 0, 255, 256, 64, 3, 200, 128, 31, 33, 250]            # (tests/test_gpu_ir.py's plan)
PLAN_2048 = [2048, 64, 1000, 256, 2048, 0, 1, 2047]


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    p = str(tmp_path_factory.mktemp("ir_long") / "lstm16.json")
    modelgen.write_model(modelgen.make_model(kind="lstm", hidden=16, input_size=1, seed=5), p)
    return ax.Model(p)


def _ring(capacity, max_frames):
    R = 1
    while R < capacity + max_frames:
        R <<= 1
    return R


def _pool(model, S, max_frames, capacity=None, sr=48000.0, fade=0):
    p = ax.Pool(S, max_frames, sr)
    p.set_model(model)
    p.set_controls(ax.default_controls(enabled=0.0))
    if capacity is not None:
        p.set_ir_capacity(capacity)
        assert p.ir_capacity() == capacity
    if fade:
        p.set_ir_fade(fade)
    return p


def _sizes(plan, total):
    out = []
    while sum(out) <= total:
        out.extend(plan)
    return out


def _run(pool, x, sizes, at=None):
    """x through the pool in blocks of `sizes`; at: {block index: callable(pool)} run before that block"""
    out = np.empty_like(x)
    pos = 0
    for i, n in enumerate(sizes):
        if at and i in at:
            at[i](pool)
        out[:, pos:pos + n] = pool.process(np.ascontiguousarray(x[:, pos:pos + n]))
        pos += n
    assert pos == x.shape[1]
    return out


def _mismatch(tag, got, truth):
    bad = np.argwhere(got != truth)
    return [] if bad.size == 0 else [(tag, bad.shape[0], tuple(int(i) for i in bad[0]))]


def _ir(L, seed, sign=1.0):
    rng = np.random.default_rng(seed)
    return (sign * rng.standard_normal(L) * np.exp(-np.arange(L) / max(L / 6.0, 1.0))).astype(np.float32)


def test_the_premise(model):
    """a pool without an IR, every stream disabled, returns its input bit for bit, whatever its capacity"""
    for cap in (None, 65536):
        p = _pool(model, 5, 256, cap)
        x = modelgen.signal(5, 256, seed=1)
        assert np.array_equal(p.process(x), x)
        p.close()


def test_capacity_life_cycle(model):
    L = ax.lib()
    h = irdata.family_b(20000, 3, 512, seed=1)
    p = _pool(model, 3, 256)
    assert p.ir_capacity() == 8192
    for bad in (0, 8191, 65537):
        assert L.aidax_pool_set_ir_capacity(p.h, bad) == ERR_ARG
        assert "IR capacity must be 8192 .. 65536" in L.aidax_last_error().decode()
        assert p.ir_capacity() == 8192
    p.set_ir_capacity(65536)
    assert p.ir_capacity() == 65536
    p.set_ir_capacity(8192)                                              # any number of times before the first prepare
    assert p.ir_capacity() == 8192
    p.set_ir_capacity(20000)
    # an IR above the capacity is refused with the capacity in the message, and the pool is as it was: no IR, no history (the
    # capacity can still be set)
    taps, x, truth = h
    long = np.concatenate([taps, np.ones(1, np.float32)])
    with pytest.raises(ax.AidaxError) as e:
        p.set_ir(long)
    assert e.value.code == ERR_ARG and "IR length must be 1 .. 20000 taps (the pool's IR capacity)" in str(e.value)
    with pytest.raises(ax.AidaxError):
        p.set_ir_slot(5, long)
    assert np.array_equal(p.process(np.ascontiguousarray(x[:, :256])), x[:, :256])
    p.set_ir_capacity(20001)
    p.set_ir_capacity(20000)
    # the first prepare fixes it: a prepare that is never committed, of a slot's emptying at that
    sg = p.prepare_ir_slot(7, None)
    assert L.aidax_pool_set_ir_capacity(p.h, 30000) == ERR_STATE
    assert "IR capacity is fixed once the first" in L.aidax_last_error().decode()
    assert L.aidax_pool_set_ir_capacity(p.h, 20000) == ERR_STATE        # the value it has, too
    assert L.aidax_pool_set_ir_capacity(p.h, 7) == ERR_ARG              # (the range is checked first)
    assert p.ir_capacity() == 20000
    p.staged_free(sg)
    with pytest.raises(ax.AidaxError):
        p.set_ir(long)
    p.set_ir(taps)                                                       # exactly the capacity
    got = np.concatenate([p.process(np.ascontiguousarray(x[:, :256])), p.process(np.ascontiguousarray(x[:, 256:]))], axis=1)
    assert np.array_equal(got, irdata.exact_conv(taps, x))              # (the first block above went by before the history existed)
    p.close()


def test_a_default_pool_still_refuses_8193_taps(model):
    p = _pool(model, 3, 256)
    for call in (lambda h: p.set_ir(h), lambda h: p.set_ir_slot(0, h), lambda h: p.prepare_ir(h)):
        with pytest.raises(ax.AidaxError) as e:
            call(np.ones(8193, np.float32))
        assert e.value.code == ERR_ARG and str(e.value).endswith("IR length must be 1 .. 8192 taps")
    p.set_ir(np.ones(8192, np.float32))
    assert ax.lib().aidax_pool_set_ir_capacity(p.h, 8192) == ERR_STATE
    assert p.ir_capacity() == 8192
    p.close()


def _exact(model, S, L, max_frames, plan, families, seed, commits=False):
    """families of (L, S) on pools whose capacity is L, over more than two turns of the ring; returns the mismatches.
    commits: the IR is prepared at 10 % of the run (the history starts there), committed at 25 %, removed at 50 % and set again at 60 %"""
    R = _ring(L, max_frames)
    sizes = _sizes(plan, 2 * R)
    T = sum(sizes)
    assert T > 2 * R
    starts = np.concatenate([[0], np.cumsum(sizes)])
    bad = []
    for f in families:
        h, x, truth = irdata.FAMILIES[f](L, S, T, seed)
        p = _pool(model, S, max_frames, L)
        if not commits:
            p.set_ir(h)
            want = truth
            marks = None
        else:
            staged = []

            def prepare(q):
                staged.append(q.prepare_ir(h))

            def commit(q):
                q.commit_ir(staged[0])
                q.staged_free(staged[0])
            marks = {}
            live = np.zeros(len(sizes), bool)
            for frac, fn, on in ((0.1, prepare, False), (0.25, commit, True), (0.5, lambda q: q.set_ir(None), False), (0.6, lambda q: q.set_ir(h), True)):
                i = int(np.searchsorted(starts, frac * T))
                marks[i] = fn
                live[i:] = on
            x_hist = x.copy()
            x_hist[:, :starts[min(marks)]] = 0.0
            t2 = irdata.exact_conv(h, x_hist)
            want = x.copy()
            for i in np.flatnonzero(live):
                want[:, starts[i]:starts[i + 1]] = t2[:, starts[i]:starts[i + 1]]
        bad += _mismatch(f"{f}{L}x{S}", _run(p, x, sizes, marks), want)
        p.close()
    return bad


# (S, L, max_frames, plan, families): every length of the issue's list on one-stream pools (the K split: 64 workgroups per block)
@pytest.mark.parametrize("L", [8193, 16384, 16511, 33021, 65536])
def test_one_stream_every_length(model, L):
    plan = RAGGED if L in (8193, 65536) else [64] if L == 16384 else [256] if L == 16511 else PLAN_2048
    bad = _exact(model, 1, L, max(plan), plan, "ABC", seed=L)
    assert not bad, bad


@pytest.mark.parametrize("S,L,max_frames,plan,families", [
    (16, 65536, 256, [256], "ABC"),
    (16, 8193, 64, [64], "ABC"),
    (64, 16384, 2048, PLAN_2048, "AC"),
    (100, 16511, 256, RAGGED, "B"),
    (100, 65536, 2048, [2048], "B"),
    (1024, 8193, 256, [256], "B"),
    (1024, 16384, 256, [256], "B"),
    (1024, 8193, 2048, [2048, 777], "B"),
])
def test_pools_of_16_to_1024_streams(model, S, L, max_frames, plan, families):
    bad = _exact(model, S, L, max_frames, plan, families, seed=S + L)
    assert not bad, bad


@pytest.mark.parametrize("S,L", [(1, 33021), (16, 33021), (100, 65536)])
def test_an_ir_committed_mid_run(model, S, L):
    bad = _exact(model, S, L, 256, RAGGED if S < 100 else [256], "B" if S > 64 else "AB", seed=7 * S + L, commits=True)
    assert not bad, bad


@pytest.mark.parametrize("S", [1, 17])
def test_every_entry_point_gives_the_exact_bits(model, S):
    import torch
    L = 16511
    R = _ring(L, 256)
    sizes = _sizes([n for n in RAGGED if n], 2 * R)
    T = sum(sizes)
    h, x, truth = irdata.family_a(L, S, T, seed=500 + S)
    starts = np.concatenate([[0], np.cumsum(sizes)])
    blocks = [np.ascontiguousarray(x[:, starts[i]:starts[i + 1]]) for i in range(len(sizes))]
    pools = [_pool(model, S, 256, L) for _ in range(3)]
    for p in pools:
        p.set_ir(h)
    bad = _mismatch("process", np.concatenate([pools[0].process(b) for b in blocks], axis=1), truth)
    got = []
    for i, b in enumerate(blocks):                                       # submit / collect, three blocks in flight
        if i >= 3:
            got.append(pools[1].collect(sizes[i - 3]))
        pools[1].submit(b)
    got += [pools[1].collect(n) for n in sizes[-3:]]
    bad += _mismatch("submit", np.concatenate(got, axis=1), truth)
    s = torch.cuda.Stream()                                              # process_device on a torch stream, in place
    got = []
    for b in blocks:
        d = torch.from_numpy(b.copy()).cuda()
        torch.cuda.current_stream().synchronize()
        with torch.cuda.stream(s):
            pools[2].process_device(d.data_ptr(), d.data_ptr(), b.shape[1], s.cuda_stream)
        s.synchronize()
        got.append(d.cpu().numpy())
    bad += _mismatch("process_device", np.concatenate(got, axis=1), truth)
    for p in pools:
        p.close()
    assert not bad, bad


def test_a_mixed_plan_of_long_and_short_irs(model):
    """bank slots of 65536, 8192 and 100 taps beside a pool IR of 16384, the streams dealt round-robin (one on no IR): each stream's
    output is its own IR's exact convolution"""
    S, n = 70, 256
    R = _ring(65536, n)
    sizes = _sizes([n], 2 * R)
    T = sum(sizes)
    _, x, _ = irdata.family_b(65536, S, T, seed=11)
    irs = {ax.IR_POOL: irdata.family_b(16384, 1, 8, seed=12)[0], 0: irdata.family_b(65536, 1, 8, seed=13)[0],
           1: irdata.family_b(8192, 1, 8, seed=14)[0], 2: irdata.family_b(100, 1, 8, seed=15)[0], ax.IR_NONE: None}
    keys = list(irs)
    p = _pool(model, S, n, 65536)
    p.set_ir(irs[ax.IR_POOL])
    for k in (0, 1, 2):
        p.set_ir_slot(k, irs[k])
    assign = [keys[s % len(keys)] for s in range(S)]
    for s, k in enumerate(assign):
        p.assign_ir(s, k)
    got = _run(p, x, sizes)
    p.close()
    bad = []
    for k in keys:
        rows = [s for s in range(S) if assign[s] == k]
        want = x[rows] if irs[k] is None else irdata.exact_conv(irs[k], x[rows])
        bad += _mismatch(f"slot {k}", got[rows], want)
    assert not bad, bad


def test_every_stream_on_one_long_slot_is_that_ir_as_the_pool_ir(model):
    """random data (nothing exact about it): the same bits from a bank slot as from the pool IR"""
    S, n, L = 70, 256, 65536
    h = _ir(L, 21)
    a, b = _pool(model, S, n, L), _pool(model, S, n, L)
    a.set_ir(h)
    b.set_ir_slot(9, h)
    b.assign_ir(ax.ALL_STREAMS, 9)
    for i in range(6):
        x = modelgen.signal(S, n, seed=30 + i)
        ya, yb = a.process(x), b.process(x)
        assert np.abs(ya).max() > 0 and np.array_equal(ya, yb), i
    a.close()
    b.close()


@pytest.mark.parametrize("S,L,n", [(1, 65536, 64), (1, 33021, 256), (17, 65536, 256), (3, 16511, 2048)])
def test_random_long_irs_against_fp64(model, S, L, n):
    """per sample <= TAU (|h| * |dry|)_t, the bound of tests/test_gpu_ir.py (measured there: 4.3e-7 at up to 8192 taps)"""
    R = _ring(L, n)
    T = (R + L) // n * n + n
    h = _ir(L, 40 + S)
    x = modelgen.signal(S, T, seed=50 + S)
    p = _pool(model, S, n, L)
    p.set_ir(h)
    got = _run(p, x, [n] * (T // n))
    p.close()
    worst = _tau(f"long{L}x{S}x{n}", got, x, h)
    print(f"ir_long {L} taps, {S} streams, blocks of {n}: max |y - y64| / (|h| * |dry|) = {worst:.3e} (bound {TAU:.0e})")


def _fade_check(tag, got, new, x, h_old, h_new, F, n):
    lf = min(F, n)
    assert np.array_equal(got[:, lf:], new[:, lf:]), (tag, "frames past the fade")
    y64, E = irfade.expected(x, h_old, h_new, F, n)
    err = np.abs(got.astype(np.float64) - y64)
    over = np.maximum(err - 1e-12 * E.max(), 0.0)                       # (the FFT's noise on near-silent samples, as in test_gpu_ir_fade.py)
    assert not over[E <= 0].any(), tag
    ratio = (over / np.where(E > 0, E, 1.0)).max()
    print(f"ir_long fade {tag}: max |y - y64| / E = {ratio:.3e}")
    errlog.bound(ratio, TAU, f"gpu_ir_long_fade_tau:{tag}")
    # the fade is really there: most of its frames are far from the abrupt switch
    far = np.abs(got.astype(np.float64) - new)[:, :lf - 1] > 10 * TAU * E[:, :lf - 1]
    assert far.mean() > 0.9, (tag, far.mean())


@pytest.mark.parametrize("S,n,F", [(5, 256, 100), (1, 64, 64)])
def test_a_fade_from_a_65536_tap_ir_to_a_short_one_and_back(model, S, n, F):
    h_long, h_short = _ir(65536, 60), _ir(333, 61, sign=-1.0)
    fade, twin = _pool(model, S, n, 65536, fade=F), _pool(model, S, n, 65536)
    x = np.zeros((S, 0), np.float32)

    def block(seed):
        nonlocal x
        blk = modelgen.signal(S, n, seed=seed)
        x = np.concatenate([x, blk], axis=1)
        return fade.process(blk), twin.process(blk)
    for p in (fade, twin):
        p.set_ir(h_long)
    for i in range(5):
        a, b = block(70 + i)
        assert np.array_equal(a, b), "before any change the fade length changes nothing"
    seed = 80
    for tag, h_old, h_new in (("long -> short", h_long, h_short), ("short -> long", h_short, h_long)):
        for p in (fade, twin):
            p.set_ir(h_new)
        a, b = block(seed)
        _fade_check(f"{tag} x{S}", a, b, x, h_old, h_new, F, n)
        for i in range(3):                                               # later passes: a pool that always had the new IR
            a, b = block(seed + 1 + i)
            assert np.array_equal(a, b), (tag, i)
        seed += 10
    fade.close()
    twin.close()


# ---- the real-time contract with the capacity raised (the test build's table of HIP calls, as tests/test_gpu_ir_bank_rt.py)

ALLOC = {"hipMalloc", "hipHostMalloc", "hipHostRegister", "hipEventCreateWithFlags", "hipStreamCreateWithFlags", "hipStreamCreateWithPriority"}
FREE = {"hipFree", "hipHostFree", "hipHostUnregister", "hipEventDestroy", "hipStreamDestroy"}
WAIT = {"hipStreamSynchronize", "hipEventSynchronize", "hipDeviceSynchronize", "hipMemcpy"}


@pytest.fixture
def calls():
    if conftest.SHIP_LEG:
        pytest.skip("aidax_test_hip_calls: a test hook — the shipped library has none")
    fn = ax.lib().aidax_test_hip_calls
    fn.argtypes = [C.c_char_p, C.c_uint32]
    fn.restype = C.c_int
    buf = C.create_string_buffer(4096)

    def read():
        n = fn(buf, len(buf))
        out = {}
        for line in buf.value.decode().splitlines():
            name, k = line.split()
            out[name] = int(k)
        assert len(out) == n, (n, out)
        return out
    read()
    return read


def _quiet(c, what):
    bad = {k: v for k, v in c.items() if k in ALLOC | FREE | WAIT}
    assert not bad, (what, bad, c)


class _Device:
    def __init__(self, S, n, seed):
        import torch
        self.torch = torch
        self.s = torch.cuda.Stream()
        self.x = torch.from_numpy(modelgen.signal(S, n, seed=seed)).cuda()
        self.y = torch.empty_like(self.x)
        torch.cuda.synchronize()

    def pass_(self, pool):
        with self.torch.cuda.stream(self.s):
            pool.process_device(self.x.data_ptr(), self.y.data_ptr(), self.x.shape[1], self.s.cuda_stream)

    def wait(self):
        self.s.synchronize()
        return self.y.cpu().numpy()


def test_the_audio_side_stays_quiet_with_the_capacity_raised(model, calls):
    """set_ir_capacity itself makes no HIP call; with 65536-tap IRs in place, assign_ir makes none, a slot's commit and the passes
    behind both allocate, free and wait for nothing, and a pass is one append and one convolution launch"""
    S = 70
    p = ax.Pool(S, 256)
    p.set_model(model)
    calls()
    p.set_ir_capacity(65536)
    assert p.ir_capacity() == 65536
    assert calls() == {}
    p.set_ir(_ir(65536, 1))
    p.set_ir_slot(3, _ir(40000, 2))
    dev = _Device(S, 256, seed=3)
    dev.pass_(p)
    dev.wait()
    calls()
    p.assign_ir(5, 3)
    p.assign_ir(6, ax.IR_NONE)
    assert calls() == {}
    dev.pass_(p)
    c = calls()
    _quiet(c, "pass after assign_ir")
    assert c["launch_ir_append"] == 1 and c["launch_ir_conv"] == 1 and "launch_ir_fade" not in c, c
    dev.wait()
    for taps in (_ir(65536, 6), None, _ir(8193, 7)):
        sg = p.prepare_ir_slot(3, taps)                                  # (worker side)
        calls()
        p.commit_ir(sg)                                                  # audio side
        c = calls()
        _quiet(c, "commit_ir")
        assert "launch_ir_append" not in c and "launch_ir_conv" not in c, c
        dev.pass_(p)
        c = calls()
        _quiet(c, "pass after commit_ir")
        assert c["launch_ir_append"] == 1 and c["launch_ir_conv"] == 1, c
        dev.wait()
        p.staged_free(sg)
        calls()
    p.close()


def test_a_default_pool_makes_the_launches_the_header_promises(model, calls):
    """a pool that never sets a capacity: one k_ir_append and one k_ir_conv launcher call per pass and no other stage call, and call for
    call what a pool makes whose capacity was raised (the capacity changes sizes, never the sequence of calls)"""
    S = 70
    counts = []
    for cap in (None, 65536):
        p = ax.Pool(S, 256)
        p.set_model(model)
        if cap:
            p.set_ir_capacity(cap)
        p.set_ir(_ir(8192, 4))
        dev = _Device(S, 256, seed=5)
        dev.pass_(p)
        dev.wait()
        calls()
        per_pass = []
        for _ in range(3):
            dev.pass_(p)
            c = calls()
            _quiet(c, "steady pass")
            per_pass.append(c)
            dev.wait()
        assert per_pass[0] == per_pass[1] == per_pass[2], per_pass
        c = per_pass[0]
        assert c["launch_ir_append"] == 1 and c["launch_ir_conv"] == 1 and "launch_ir_fade" not in c, c
        counts.append(c)
        p.close()
    assert counts[0] == counts[1], counts
