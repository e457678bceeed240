"""Per-stream cabinet IRs (GPU, -m gpu): the IR bank of a pool, aidax_pool_assign_ir and the plan that groups the streams by IR into the
work items of one k_ir_conv launch (IrPlan in aidax_ir.cpp, IrStage in aidax_ir_stage.cpp, aidax_ir_mfma.hip).

The exact tests use the families of tests/irdata.py, on which the correct output is the true convolution to the last bit whatever the
order of the additions, the K split or the reduce; every stream is compared with np.array_equal against the exact convolution of ITS OWN
IR (or with its dry block). As in tests/test_gpu_ir_exact.py, the pools run a real model with every stream disabled, so that the IR
stage's input is exactly the test's input, and every test first holds an IR-less twin to that."""
import importlib

import numpy as np
import pytest

from tests import irdata, modelgen
from tests.test_gpu_ir import _tau

pytestmark = pytest.mark.gpu
ax = importlib.import_module("aidadsp-lv2_amd")

ERR_ARG = -1
RING = 16384
RAGGED = [1, 17, 0, 255, 256, 64, 3, 200, 128, 31, 33, 250]
PLAN_8192 = [8192, 1, 8191, 4097, 64, 4096, 255, 8192, 0, 17, 3000]
# IRs of the bank: (family, length), the edges of 16-frame diagonals and 32-frame windows, 1 ... 8192 taps
BANK = [("A", 8192), ("B", 1), ("C", 33), ("D", 12), ("A", 17), ("B", 4097), ("C", 1000), ("D", 5), ("A", 2), ("B", 8191),
        ("C", 47), ("D", 1), ("A", 4096), ("B", 31), ("C", 16), ("A", 49)]


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    p = str(tmp_path_factory.mktemp("ir_bank") / "lstm16.json")
    modelgen.write_model(modelgen.make_model(kind="lstm", hidden=16, input_size=1, seed=5), p)
    return ax.Model(p)


def _pool(model, S, max_frames, sr=48000.0):
    p = ax.Pool(S, max_frames, sr)
    p.set_model(model)
    p.set_controls(ax.default_controls(enabled=0.0))
    return p


def _sizes(plan, total):
    out = []
    while sum(out) < total:
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


def _twin_copies(model, x, sizes, max_frames, sr=48000.0):
    """the premise: a pool without an IR, every stream disabled, returns its input bit for bit"""
    twin = _pool(model, x.shape[0], max_frames, sr)
    got = _run(twin, x, sizes)
    twin.close()
    assert np.array_equal(got, x), np.count_nonzero(got != x)


def _mismatch(got, want, assign):
    """per IR key: (key, streams that differ, first stream)"""
    bad = {}
    for s in np.flatnonzero((got != want).any(axis=1)):
        bad.setdefault(int(assign[s]), []).append(int(s))
    return {k: (len(v), v[0]) for k, v in bad.items()}


def _empty_slot(K, pattern):
    """the slot a "mixed" assignment leaves empty: K, or the last one when the bank is full (it then holds 63 IRs + the pool IR)"""
    return None if pattern != "mixed" else min(K, ax.IR_SLOTS - 1)


def _assignment(S, K, pattern, seed):
    """per stream: a bank slot 0 .. K-1, or (pattern "mixed") also ax.IR_NONE, the pool IR, or an empty slot"""
    rng = np.random.default_rng([S, K, seed])
    if pattern == "round_robin":
        return np.arange(S) % K
    if pattern == "runs":
        return np.minimum(np.arange(S) * K // S, K - 1)
    if pattern == "random":
        return rng.integers(0, K, size=S)
    choice = np.array(sorted(set(range(K)) | {_empty_slot(K, pattern)}) + [ax.IR_NONE, ax.IR_POOL])
    return choice[rng.integers(0, choice.size, size=S)]


def _mixed_case(S, K, pattern, T, seed, pool_ir=("C", 4095)):
    """(assignment, {key: h}, x, want): key = bank slot, or ax.IR_POOL; every stream's input drawn from its own IR's family (dry
    streams: family B's dense input) and its truth the exact convolution with that IR"""
    assign = _assignment(S, K, pattern, seed)
    irs = {k: BANK[(k + seed) % len(BANK)] for k in range(K) if k != _empty_slot(K, pattern)}
    irs[ax.IR_POOL] = pool_ir
    x = np.empty((S, T), np.float32)
    want = np.empty((S, T), np.float32)
    hs = {}
    for key in np.unique(assign):
        rows = np.flatnonzero(assign == key)
        if int(key) in irs:
            f, L = irs[int(key)]
            h, xk, tk = irdata.FAMILIES[f](L, rows.size, T, seed * 1000 + int(key) + 7)
            hs[int(key)] = h
        else:                                              # AIDAX_IR_NONE, or a slot that is never loaded: the dry block
            xk = irdata.family_b(8, rows.size, T, seed * 1000 + 999)[1]
            tk = xk
        x[rows], want[rows] = xk, tk
    return assign, hs, x, want


def _load(pool, assign, hs):
    for k, h in hs.items():
        if k == ax.IR_POOL:
            pool.set_ir(h)
        else:
            pool.set_ir_slot(k, h)
    for s, k in enumerate(assign):
        pool.assign_ir(s, int(k))


def _exact_mixed(model, S, K, pattern, plan, total, seed, max_frames=256, sr=48000.0):
    sizes = _sizes(plan, total)
    T = sum(sizes)
    assign, hs, x, want = _mixed_case(S, K, pattern, T, seed)
    _twin_copies(model, x, sizes, max_frames, sr)
    p = _pool(model, S, max_frames, sr)
    _load(p, assign, hs)
    assert [p.stream_ir(s) for s in range(S)] == [int(k) for k in assign]
    got = _run(p, x, sizes)
    p.close()
    return _mismatch(got, want, assign)


# (S, number of distinct bank IRs, assignment): the edges of 16-stream groups and 64-stream items, 1 ... 64 IRs
MIXED = [(1, 1, "runs"), (1, 2, "mixed"), (15, 2, "round_robin"), (15, 5, "mixed"), (16, 5, "runs"), (16, 2, "random"),
         (17, 5, "round_robin"), (17, 2, "mixed"), (63, 5, "random"), (63, 64, "mixed"), (64, 64, "round_robin"), (64, 2, "runs"),
         (65, 5, "mixed"), (65, 64, "random"), (200, 64, "mixed"), (200, 5, "runs"), (1024, 64, "round_robin"), (1024, 5, "mixed"),
         (1024, 16, "runs"), (4096, 64, "mixed"), (4096, 1, "round_robin")]


@pytest.mark.parametrize("S,K,pattern", MIXED, ids=[f"S{s}-K{k}-{p}" for s, k, p in MIXED])
def test_mixed_plans_are_exact_per_stream(model, S, K, pattern):
    # (at least the longest IR's length: irdata.exact_conv takes blocks as long as the IR)
    total = 2 * RING + 700 if S <= 65 else RING + 300 if S <= 200 else 8192 + 300
    bad = _exact_mixed(model, S, K, pattern, RAGGED, total, seed=S + 7 * K)
    assert not bad, bad


@pytest.mark.parametrize("S,K", [(1, 1), (1024, 5)])
def test_mixed_plans_on_blocks_of_8192_frames(model, S, K):
    bad = _exact_mixed(model, S, K, "mixed" if S > 1 else "runs", PLAN_8192, 2 * RING if S == 1 else 8192 + 8193, seed=50 + S,
                       max_frames=8192)
    assert not bad, bad


@pytest.mark.parametrize("sr", [44100.0, 96000.0])
def test_mixed_plans_at_other_host_rates(model, sr):
    bad = _exact_mixed(model, 40, 5, "mixed", RAGGED, RING + 500, seed=int(sr) % 97, sr=sr)
    assert not bad, bad


@pytest.mark.parametrize("f", ["A", "B"])
def test_reassignment_and_slot_swaps_mid_run(model, f):
    """streams change slot at block boundaries and slots are re-committed (prepare on the side, commit between blocks) or emptied while
    streams use them: every block after a change is the exact convolution of the whole history with the IR then in force"""
    S = 40
    sizes = _sizes(RAGGED, 4 * RING)
    T = sum(sizes)
    Ls = (1, 33, 4097, 8192, 1000, 17)
    # one input for every IR: family A's impulses spaced past the longest IR, or family B's dense input (B's IRs are <= 4 taps)
    x = irdata.FAMILIES[f](max(Ls), S, T, seed=600)[1]
    hs = [irdata.FAMILIES[f](L, 1, 64, seed=610 + i)[0] for i, L in enumerate(Ls)]
    truth = [irdata.exact_conv(h, x) for h in hs]
    _twin_copies(model, x, sizes, 256)
    starts = np.concatenate([[0], np.cumsum(sizes)])
    nb = len(sizes)
    # which IR (index into hs, -1 dry) each stream hears per block
    hear = np.full((nb, S), -1)
    slot_ir = {0: 0, 1: 1, 2: 2, 3: 3}                     # slot -> index into hs
    assign = np.arange(S) % 4
    staged = []
    events = {}

    def mark(i, fn):
        events.setdefault(i, []).append(fn)

    def frac(v):
        return int(np.searchsorted(starts, v * T))

    cur = dict(assign=assign.copy(), slot_ir=dict(slot_ir))
    plan = [(0.0, "assign", assign.copy()),
            (0.15, "assign", (np.arange(S) * 7 + 3) % 4),                 # everybody moves
            (0.3, "prepare", (2, 4)),                                     # slot 2's next IR, prepared a while before it is committed
            (0.35, "commit", 2),
            (0.5, "assign", np.where(np.arange(S) % 5 == 0, ax.IR_NONE, np.arange(S) % 4)),
            (0.6, "empty", 1),                                           # slot 1 emptied while its streams use it: they return dry
            (0.7, "set", (1, 5)),                                        # ... and loaded again with another IR
            (0.85, "assign", np.full(S, 3))]                              # one IR for every stream: the identity plan
    for v, kind, arg in plan:
        i = frac(v)
        if kind == "assign":
            a = arg.copy()
            mark(i, lambda p, a=a: [p.assign_ir(s, int(k)) for s, k in enumerate(a)])
        elif kind == "prepare":
            mark(i, lambda p, arg=arg: staged.append(p.prepare_ir_slot(arg[0], hs[arg[1]])))
        elif kind == "commit":
            def commit(p):
                p.commit_ir(staged[0])
                p.staged_free(staged[0])
            mark(i, commit)
        elif kind == "empty":
            mark(i, lambda p, arg=arg: p.set_ir_slot(arg, None))
        elif kind == "set":
            mark(i, lambda p, arg=arg: p.set_ir_slot(arg[0], hs[arg[1]]))
    # the IR each stream hears, block by block
    timeline = sorted(((frac(v), kind, arg) for v, kind, arg in plan), key=lambda e: e[0])
    k = 0
    for b in range(nb):
        while k < len(timeline) and timeline[k][0] == b:
            _, kind, arg = timeline[k]
            if kind == "assign":
                cur["assign"] = arg.copy()
            elif kind == "commit":
                cur["slot_ir"][arg] = 4
            elif kind == "empty":
                cur["slot_ir"].pop(arg, None)
            elif kind == "set":
                cur["slot_ir"][arg[0]] = arg[1]
            k += 1
        hear[b] = [cur["slot_ir"].get(int(a), -1) if a >= 0 else -1 for a in cur["assign"]]
    p = _pool(model, S, 256)
    for slot, i in slot_ir.items():
        p.set_ir_slot(slot, hs[i])
    got = _run(p, x, sizes, {i: (lambda p, fns=fns: [fn(p) for fn in fns]) for i, fns in events.items()})
    p.close()
    want = np.empty_like(x)
    for b in range(nb):
        for s in range(S):
            src = x if hear[b, s] < 0 else truth[hear[b, s]]
            want[s, starts[b]:starts[b + 1]] = src[s, starts[b]:starts[b + 1]]
    assert len({tuple(r) for r in hear}) >= 6
    bad = np.argwhere(got != want)
    assert bad.size == 0, (bad.shape[0], tuple(int(i) for i in bad[0]), hear[np.searchsorted(starts, bad[0][1], "right") - 1, bad[0][0]])


def _ir(L, seed):
    rng = np.random.default_rng(seed)
    t = np.arange(L)
    return (rng.standard_normal(L) * np.exp(-t / max(L / 6.0, 1.0))).astype(np.float32)


@pytest.mark.parametrize("S", [1, 17, 200])
def test_one_bank_slot_for_every_stream_is_bit_identical_to_the_pool_ir(model, S):
    """all streams on bank slot j against a twin that holds the same taps as its pool IR, on random decaying IRs (no exact family): the
    identity plan runs the one-IR pool's grid, K split and summation order, on every entry point"""
    import torch
    L = 4097
    h = _ir(L, 700 + S)
    sizes = _sizes([n for n in RAGGED if n], RING + 300)
    x = modelgen.signal(S, sum(sizes), seed=710 + S)
    starts = np.concatenate([[0], np.cumsum(sizes)])
    blocks = [np.ascontiguousarray(x[:, starts[i]:starts[i + 1]]) for i in range(len(sizes))]
    pools = []
    for j in (None, 0, 37, 63):
        p = ax.Pool(S, 256)
        p.set_model(model)
        p.set_controls(ax.default_controls(pregain_db=3.0, master_db=-2.0))
        if j is None:
            p.set_ir(h)
        else:
            p.set_ir(_ir(33, 1))                            # a pool IR that nobody hears
            p.set_ir_slot(j, h)
            p.set_ir_slot((j + 1) % 64, _ir(1000, 2))       # ... and a slot that nobody uses
            p.assign_ir(ax.ALL_STREAMS, j)
        pools.append(p)

    def by_process(p):
        return np.concatenate([p.process(b) for b in blocks], axis=1)

    def by_submit(p):
        got = []
        for i, b in enumerate(blocks):
            if i >= 3:
                got.append(p.collect(sizes[i - 3]))
            p.submit(b)
        got += [p.collect(n) for n in sizes[-3:]]
        return np.concatenate(got, axis=1)

    def by_device(p):
        s = torch.cuda.Stream()
        got = []
        for b in blocks:
            d = torch.from_numpy(b.copy()).cuda()
            torch.cuda.current_stream().synchronize()
            with torch.cuda.stream(s):
                p.process_device(d.data_ptr(), d.data_ptr(), b.shape[1], s.cuda_stream)
            s.synchronize()
            got.append(d.cpu().numpy())
        return np.concatenate(got, axis=1)

    for path in (by_process, by_submit, by_device):
        outs = [path(p) for p in pools]
        assert np.abs(outs[0]).max() > 0.01
        for j, o in zip((0, 37, 63), outs[1:]):
            assert np.array_equal(o, outs[0]), (path.__name__, j, np.count_nonzero(o != outs[0]))
    for p in pools:
        p.close()


def test_mixed_plans_on_a_real_chain_are_within_the_fp64_bound(model, tmp_path):
    """random decaying IRs of 1 ... 8192 taps, one per slot, under a mixed plan after a non-trivial chain (LSTM-16 enabled, EQ, gains):
    every stream within TAU (|h_s| * |dry_s|)_t of the fp64 convolution of its own dry output (the IR-less twin's) with its own IR"""
    S = 70
    Ls = (1, 31, 32, 33, 1000, 4097, 8192)
    hs = [_ir(L, 800 + L) for L in Ls]
    assign = _assignment(S, len(Ls), "mixed", 8)
    sizes = _sizes(RAGGED, 8192 + 2000)
    x = modelgen.signal(S, sum(sizes), seed=801)
    ctl = ax.default_controls(pregain_db=3.0, bass_boost_db=2.0, master_db=-2.0)
    pools = []
    for with_ir in (False, True):
        p = ax.Pool(S, 256)
        p.set_model(model)
        p.set_controls(ctl)
        if with_ir:
            p.set_ir(hs[2])
            for k, h in enumerate(hs):
                p.set_ir_slot(k, h)
            for s, k in enumerate(assign):
                p.assign_ir(s, int(k))
        pools.append(p)
    outs = []
    for p in pools:
        outs.append(_run(p, x, sizes))
        p.close()
    dry, got = outs
    assert np.abs(dry).max() > 0.01
    for key in np.unique(assign):
        rows = np.flatnonzero(assign == key)
        k = int(key)
        if k == ax.IR_NONE or k == _empty_slot(len(Ls), "mixed"):
            assert np.array_equal(got[rows], dry[rows]), k
            continue
        h = hs[2] if k == ax.IR_POOL else hs[k]
        _tau(f"bank:{k}", got[rows], dry[rows], h)


def test_plans_in_flight_keep_the_plan_they_were_issued_with(model):
    """three blocks submitted with the assignments changed between the submits, then collected: bit-identical to the blocking path with
    the same changes before the same blocks (the plan goes to the device stream-ordered, from snapshots). A change is one call for every
    stream plus a few exceptions, so that the host issues the next blocks while the GPU still runs the first"""
    S = 1024
    hs = [_ir(L, 900 + L) for L in (8192, 33, 1000, 4097)]
    sizes = _sizes([256, 64, 256, 200, 256, 17], 256 * 30)
    x = modelgen.signal(S, sum(sizes), seed=901)
    rng = np.random.default_rng(902)
    changes = {i: (int(rng.integers(-2, 4)), {int(s): int(rng.integers(-2, 4)) for s in rng.choice(S, 8, replace=False)})
               for i in range(len(sizes)) if i % 3 != 2}
    changes[len(sizes) // 2] = (2, {})                       # a uniform plan in between
    pools = []
    for _ in range(2):
        p = ax.Pool(S, 256)
        p.set_model(model)
        p.set_controls(ax.default_controls(pregain_db=3.0))
        p.set_ir(hs[1])
        for k, h in enumerate(hs):
            p.set_ir_slot(k, h)
        pools.append(p)

    def apply(p, i):
        if i in changes:
            base, some = changes[i]
            p.assign_ir(ax.ALL_STREAMS, base)
            for s, k in some.items():
                p.assign_ir(s, k)

    starts = np.concatenate([[0], np.cumsum(sizes)])
    blocks = [np.ascontiguousarray(x[:, starts[i]:starts[i + 1]]) for i in range(len(sizes))]
    want = []
    for i, b in enumerate(blocks):
        apply(pools[0], i)
        want.append(pools[0].process(b))
    got = []
    for i, b in enumerate(blocks):
        if i >= 3:
            got.append(pools[1].collect(sizes[i - 3]))
        apply(pools[1], i)
        pools[1].submit(b)
    got += [pools[1].collect(n) for n in sizes[-3:]]
    for p in pools:
        p.close()
    want, got = np.concatenate(want, axis=1), np.concatenate(got, axis=1)
    assert np.abs(want).max() > 0.01
    assert np.array_equal(got, want), np.count_nonzero(got != want)


def test_life_cycle_and_argument_checks(model):
    S = 20
    p = _pool(model, S, 256)
    # argument checks
    for call in (lambda: p.assign_ir(S, 0), lambda: p.assign_ir(-3, 0), lambda: p.assign_ir(0, 64), lambda: p.assign_ir(0, -3),
                 lambda: p.stream_ir(S), lambda: p.set_ir_slot(64, np.ones(4, np.float32)), lambda: p.prepare_ir_slot(100, None),
                 lambda: p.set_ir_slot(0, np.zeros(0, np.float32)), lambda: p.set_ir_slot(0, np.ones(8193, np.float32)),
                 lambda: p.set_ir_slot(0, np.array([1.0, np.nan], np.float32)), lambda: p.set_ir_slot(0, np.ones(4, np.float32), 44100.0)):
        with pytest.raises(ax.AidaxError) as e:
            call()
        assert e.value.code == ERR_ARG
    assert [p.stream_ir(s) for s in range(S)] == [ax.IR_POOL] * S           # the default: every stream follows the pool IR
    p.assign_ir(ax.ALL_STREAMS, 7)
    p.assign_ir(3, ax.IR_NONE)
    p.assign_ir(4, ax.IR_POOL)
    assert [p.stream_ir(s) for s in range(S)] == [7, 7, 7, ax.IR_NONE, ax.IR_POOL] + [7] * (S - 5)
    # exact family B input: every block is the exact convolution of the stream's history with its IR
    sizes = _sizes(RAGGED, RING + 900)
    T = sum(sizes)
    h7, x, _ = irdata.family_b(4097, S, T, seed=1000)
    hp = irdata.family_b(33, 1, 64, seed=1001)[0]
    _twin_copies(model, x, sizes, 256)
    starts = np.concatenate([[0], np.cumsum(sizes)])
    half = int(np.searchsorted(starts, T // 2))
    three_q = int(np.searchsorted(starts, 3 * T // 4))

    def run():
        q = _pool(model, S, 256)
        q.set_ir(hp)
        q.set_ir_slot(7, h7)
        q.assign_ir(ax.ALL_STREAMS, 7)
        q.assign_ir(3, ax.IR_NONE)
        q.assign_ir(4, ax.IR_POOL)

        def reset(q):
            q.reset_stream(5)
            assert q.stream_ir(5) == 7                              # reset keeps the assignment
        got = _run(q, x, sizes, {half: reset, three_q: lambda q: q.set_ir_slot(7, None)})
        q.close()
        return got
    got = run()
    assert np.array_equal(got, run())                                # twice: the same bits
    want = irdata.exact_conv(h7, x)
    want[3] = x[3]
    want[4] = irdata.exact_conv(hp, x[4:5])[0]
    x5 = x[5:6].copy()
    x5[:, :starts[half]] = 0.0                                       # stream 5's history starts again at the reset
    want[5, starts[half]:] = irdata.exact_conv(h7, x5)[0, starts[half]:]
    emptied = np.ones(S, bool)
    emptied[[3, 4]] = False
    want[emptied, starts[three_q]:] = x[emptied, starts[three_q]:]   # the emptied slot's streams return dry
    bad = np.argwhere(got != want)
    assert bad.size == 0, (bad.shape[0], tuple(int(i) for i in bad[0]))
    p.close()


def test_one_stream_on_a_bank_slot_round_trips_like_the_pool_ir(model):
    """the LV2 case: a one-stream pool, 64-frame blocks, the IR in a bank slot against the same IR as the pool IR"""
    h = _ir(8192, 1100)
    sizes = [64] * 300
    x = modelgen.signal(1, sum(sizes), seed=1101)
    outs = []
    for slot in (None, 9):
        p = ax.Pool(1, 64)
        p.set_model(model)
        p.set_controls(ax.default_controls(master_db=-3.0))
        if slot is None:
            p.set_ir(h)
        else:
            p.set_ir_slot(slot, h)
            p.assign_ir(0, slot)
        outs.append(_run(p, x, sizes))
        p.close()
    assert np.abs(outs[0]).max() > 0.01
    assert np.array_equal(outs[0], outs[1])
