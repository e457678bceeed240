"""The cabinet IR stage bit for bit (GPU, -m gpu): k_ir_conv on the exact-arithmetic families of tests/irdata.py, where the correct output
is the true convolution to the last bit whatever the order of the additions, the K split or the reduce (tests/test_ir_arith.py shows
that, and that a kernel which drops or misplaces any one of its six term products, or splits an operand into two bf16 terms, changes
thousands of those bits). So every comparison here is np.array_equal against a truth computed by superposition.

The pools run a real model (LSTM-16) with every stream disabled: a disabled stream's output is a raw copy of its input, and the IR is
applied whatever `enabled` says (include/aidax.h), so the IR stage's input is exactly the test's input. Every test first holds an IR-less
twin to that. The history ring of a pool is R = 16384 frames (8192 taps + up to 8192 frames per block, rounded up to a power of two); the
runs below wrap it at least twice."""
import importlib

import numpy as np
import pytest

from tests import irdata, modelgen

pytestmark = pytest.mark.gpu
ax = importlib.import_module("aidadsp-lv2_amd")

RING = 16384
LENGTHS = (1, 2, 15, 16, 17, 31, 32, 33, 47, 48, 49, 1000, 4095, 4096, 4097, 8191, 8192)   # the edges of 16-frame diagonals, 32-frame windows
D_LENGTHS = (1, 5, 12)
STREAMS = (1, 3, 16, 17, 64, 65)                                                             # the edges of 16-stream groups and 64-stream waves
RAGGED = [1, 17, 0, 255, 256, 64, 3, 200, 128, 31, 33, 250]                                 # (tests/test_gpu_ir.py's plan)
PLAN_1024 = [1024, 1000, 17, 1024, 0, 1, 513, 1024, 64, 999]
PLAN_8192 = [8192, 1, 8191, 4097, 64, 4096, 255, 8192, 0, 17, 3000]


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    p = str(tmp_path_factory.mktemp("ir_exact") / "lstm16.json")
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


def _mismatch(tag, got, truth):
    bad = np.argwhere(got != truth)
    return [] if bad.size == 0 else [(tag, bad.shape[0], tuple(int(i) for i in bad[0]))]


def _exact(model, S, max_frames, plan, total, cases, seed, sr=48000.0):
    """every (family, L) of `cases` on a pool of its own with the same block plan; returns the mismatches"""
    sizes = _sizes(plan, total)
    T = sum(sizes)
    _twin_copies(model, irdata.family_b(8, S, T, seed)[1], sizes, max_frames, sr)
    bad = []
    for f, L in cases:
        h, x, truth = irdata.FAMILIES[f](L, S, T, seed)
        p = _pool(model, S, max_frames, sr)
        p.set_ir(h)
        bad += _mismatch(f"{f}{L}", _run(p, x, sizes), truth)
        p.close()
    return bad


@pytest.mark.parametrize("S", STREAMS)
def test_every_length_is_exact_on_ragged_blocks(model, S):
    cases = [(f, L) for f in "ABC" for L in LENGTHS] + [("D", L) for L in D_LENGTHS]
    bad = _exact(model, S, 256, RAGGED, 3 * RING, cases, seed=S)
    assert not bad, bad


def test_blocks_of_up_to_1024_frames(model):
    cases = [(f, L) for f in "ABC" for L in (1, 33, 1000, 4097, 8192)] + [("D", 12)]
    bad = []
    for S in (1, 17):
        bad += _exact(model, S, 1024, PLAN_1024, 3 * RING, cases, seed=100 + S)
    assert not bad, bad


def test_blocks_of_8192_frames_one_stream(model):
    """S = 1: short blocks split K over up to 64 workgroups, an 8192-frame block over 8; the 8192-frame blocks hold the whole IR and fill
    the ring exactly (8192 frames of history + 8192 of block = R)"""
    cases = [(f, L) for f in "ABC" for L in (1, 17, 4096, 4097, 8191, 8192)] + [("D", 12)]
    bad = _exact(model, 1, 8192, PLAN_8192, 4 * RING, cases, seed=200)
    assert not bad, bad


def test_blocks_of_8192_frames_1024_streams(model):
    """S = 1024: the partial sums' budget caps the K split at 2 (short blocks split in two, 8192-frame blocks do not)"""
    bad = _exact(model, 1024, 8192, PLAN_8192, 2 * RING, [("A", 8192), ("B", 8192)], seed=300)
    assert not bad, bad


@pytest.mark.parametrize("f", ["A", "B"])
def test_an_ir_committed_mid_run_sounds_the_history_since_the_first_prepare(model, f):
    """no history before the first prepare_ir; from then on the ring fills whether an IR is live or not: prepared (not live), committed,
    removed (set_ir(None): the dry signal again), set again (the convolution over everything since the prepare)"""
    S, L = 17, 4097
    sizes = _sizes(RAGGED, 4 * RING)
    T = sum(sizes)
    h, x, _ = irdata.FAMILIES[f](L, S, T, seed=400)
    _twin_copies(model, x, sizes, 256)
    marks = {}
    starts = np.concatenate([[0], np.cumsum(sizes)])
    live = np.zeros(len(sizes), bool)
    staged = []

    def prepare(p):
        staged.append(p.prepare_ir(h))

    def commit(p):
        p.commit_ir(staged[0])
        p.staged_free(staged[0])

    for frac, fn, on in ((0.1, prepare, False), (0.25, commit, True), (0.5, lambda p: p.set_ir(None), False), (0.6, lambda p: p.set_ir(h), True)):
        i = int(np.searchsorted(starts, frac * T))
        marks[i] = fn
        live[i:] = on
    first = min(marks)
    x_hist = x.copy()
    x_hist[:, :starts[first]] = 0.0
    truth = irdata.exact_conv(h, x_hist)
    p = _pool(model, S, 256)
    got = _run(p, x, sizes, marks)
    p.close()
    want = x.copy()
    for i in np.flatnonzero(live):
        want[:, starts[i]:starts[i + 1]] = truth[:, starts[i]:starts[i + 1]]
    assert live.any() and not live.all()
    assert np.array_equal(got, want), _mismatch(f, got, want)


@pytest.mark.parametrize("S", [1, 17])
def test_every_entry_point_gives_the_exact_bits(model, S):
    import torch
    L = 4097
    sizes = _sizes([n for n in RAGGED if n], 3 * RING)
    T = sum(sizes)
    h, x, truth = irdata.family_a(L, S, T, seed=500 + S)
    _twin_copies(model, x, sizes, 256)
    starts = np.concatenate([[0], np.cumsum(sizes)])
    blocks = [np.ascontiguousarray(x[:, starts[i]:starts[i + 1]]) for i in range(len(sizes))]
    pools = [_pool(model, S, 256) for _ in range(4)]
    for p in pools:
        p.set_ir(h)
    bad = []
    # process
    bad += _mismatch("process", np.concatenate([pools[0].process(b) for b in blocks], axis=1), truth)
    # submit / collect, three blocks in flight
    got = []
    for i, b in enumerate(blocks):
        if i >= 3:
            got.append(pools[1].collect(sizes[i - 3]))
        pools[1].submit(b)
    got += [pools[1].collect(n) for n in sizes[-3:]]
    bad += _mismatch("submit", np.concatenate(got, axis=1), truth)
    # submit_to on registered buffers, three pairs in flight
    cap = S * 256
    ins = [np.zeros(cap, np.float32) for _ in range(3)]
    outs = [np.zeros(cap, np.float32) for _ in range(3)]
    for a in ins + outs:
        pools[2].register_host(a)
    got = []
    for i, b in enumerate(blocks):
        if i >= 3:
            k, n = (i - 3) % 3, sizes[i - 3]
            got.append(pools[2].collect(n, outs[k][:S * n].reshape(S, n)).copy())
        k, n = i % 3, sizes[i]
        src, dst = ins[k][:S * n].reshape(S, n), outs[k][:S * n].reshape(S, n)
        src[...] = b
        pools[2].submit_to(src, dst)
    for i in range(len(blocks) - 3, len(blocks)):
        k, n = i % 3, sizes[i]
        got.append(pools[2].collect(n, outs[k][:S * n].reshape(S, n)).copy())
    for a in ins + outs:
        pools[2].unregister_host(a)
    bad += _mismatch("submit_to", np.concatenate(got, axis=1), truth)
    # process_device on a torch stream, in place
    s = torch.cuda.Stream()
    got = []
    for b in blocks:
        d = torch.from_numpy(b.copy()).cuda()
        torch.cuda.current_stream().synchronize()
        with torch.cuda.stream(s):
            pools[3].process_device(d.data_ptr(), d.data_ptr(), b.shape[1], s.cuda_stream)
        s.synchronize()
        got.append(d.cpu().numpy())
    bad += _mismatch("process_device", np.concatenate(got, axis=1), truth)
    for p in pools:
        p.close()
    assert not bad, bad


@pytest.mark.parametrize("sr", [44100.0, 96000.0])
def test_pools_at_other_host_rates_take_an_ir_at_their_own_rate(model, sr):
    cases = [("A", 1), ("A", 4097), ("A", 8192)]
    bad = _exact(model, 3, 256, RAGGED, 3 * RING, cases, seed=int(sr), sr=sr)
    assert not bad, bad
