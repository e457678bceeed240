"""The cabinet IR stage on the GPU (aidax_pool_prepare_ir / commit_ir / set_ir, k_ir_conv): every stream's output is the causal
convolution of the signal the pool would have returned without an IR (`dry`, read from an IR-less twin pool with the same model,
controls and input) with the IR, continuous across blocks of every length the pool takes.

A single tap that is a power of two must reproduce the dry signal exactly (delayed, scaled): the three-term bf16 split is exact, so any
indexing or history error shows as a mismatch. Random decaying IRs are held against an fp64 convolution of the twin's output at
1e-5 * ||h||_1 * max|dry| and, per output sample, at TAU * (|h| * |dry|)_t, so that an error confined to quiet passages or to one tile
or block edge cannot hide under the loudest sample. IRs are synthesised here (seeded exponentially decaying noise); the bit-exact tests
of every term product are in tests/test_gpu_ir_exact.py."""
import ctypes as C
import importlib
import queue
import threading

import numpy as np
import pytest

from tests import errlog, modelgen

pytestmark = pytest.mark.gpu
ax = importlib.import_module("aidadsp-lv2_amd")
ERR_ARG = -1
RAGGED = [1, 17, 0, 255, 256, 64, 3, 200, 128, 31, 33, 250]


def _model(tmp_path, name, **kw):
    j = modelgen.make_model(**kw)
    p = str(tmp_path / f"{name}.json")
    modelgen.write_model(j, p)
    return ax.Model(p)


def _ctl():
    return ax.default_controls(pregain_db=3.0, bass_boost_db=2.0, master_db=-2.0)


def _pools(model, n, S, max_frames=256):
    out = []
    for _ in range(n):
        p = ax.Pool(S, max_frames)
        p.set_model(model)
        p.set_controls(_ctl())
        out.append(p)
    return out


def _ir(L, seed):
    rng = np.random.default_rng(seed)
    t = np.arange(L)
    return (rng.standard_normal(L) * np.exp(-t / max(L / 6.0, 1.0))).astype(np.float32)


def _sizes(pattern, total):
    out = []
    while sum(out) < total:
        out.extend(pattern)
    return out


def _run(pools, x, sizes):
    """the same block sequence through every pool: [pool][S][frames]"""
    outs = [[] for _ in pools]
    pos = 0
    for n in sizes:
        blk = np.ascontiguousarray(x[:, pos:pos + n])
        for i, p in enumerate(pools):
            outs[i].append(p.process(blk))
        pos += n
    return [np.concatenate(o, axis=1) for o in outs]


def _conv64(dry, h):
    """causal convolution of every row with h, in fp64 (FFT), truncated to the rows' length"""
    T, L = dry.shape[1], h.size
    nfft = 1 << int(np.ceil(np.log2(T + L)))
    H = np.fft.rfft(h.astype(np.float64), nfft)
    return np.fft.irfft(np.fft.rfft(dry.astype(np.float64), nfft, axis=1) * H[None, :], nfft, axis=1)[:, :T]


# per output sample: |y - y64|_t <= TAU (|h| * |dry|)_t + 1e-12 max(|h| * |dry|), the floor for the FFT's noise on near-silent samples.
# ~10x the largest value measured on the MI355X (errlog tags gpu_ir_tau:*): 4.3e-7, random IRs of 1 - 8192 taps on 1 - 17 streams
TAU = 4e-6


def _tau(tag, got, dry, h, slack=0.0):
    """the per-sample bound; slack: an absolute error allowed on top (a dry reference that is itself within a bound)"""
    err = np.abs(got.astype(np.float64) - _conv64(dry, h))
    env = _conv64(np.abs(dry), np.abs(h))
    floor = 1e-12 * env.max() + slack
    over = np.maximum(err - floor, 0.0)
    assert not over[env <= 0].any(), (tag, over[env <= 0].max())
    return errlog.bound((over / np.where(env > 0, env, 1.0)).max(), TAU, f"gpu_ir_tau:{tag}")


def _check(tag, got, dry, h):
    err = np.abs(got.astype(np.float64) - _conv64(dry, h)).max()
    scale = float(np.abs(h.astype(np.float64)).sum() * np.abs(dry).max())
    errlog.bound(err / scale, 1e-5, f"gpu_ir:{tag}")
    _tau(tag, got, dry, h)


def test_unit_impulse_reproduces_the_dry_signal_delayed_and_scaled(tmp_path):
    m = _model(tmp_path, "u", kind="lstm", hidden=16, input_size=1, seed=5)
    S = 3
    cases = [(D, g) for D in (0, 1, 4095, 8191) for g in (1.0, 0.125)]
    pools = _pools(m, len(cases) + 1, S)
    for p, (D, g) in zip(pools[1:], cases):
        h = np.zeros(D + 1, np.float32)
        h[D] = g
        p.set_ir(h)
    sizes = _sizes(RAGGED, 8192 + 700)
    x = modelgen.signal(S, sum(sizes), seed=11)
    outs = _run(pools, x, sizes)
    dry = outs[0]
    assert np.abs(dry).max() > 0.01
    for got, (D, g) in zip(outs[1:], cases):
        want = np.zeros_like(dry)
        want[:, D:] = dry[:, :dry.shape[1] - D] * np.float32(g)
        assert np.array_equal(got, want), (D, g, np.abs(got - want).max())


@pytest.mark.parametrize("S", [1, 3, 17])
def test_random_decaying_irs_match_an_fp64_convolution(tmp_path, S):
    m = _model(tmp_path, "r", kind="lstm", hidden=16, input_size=1, seed=7)
    Ls = (1, 31, 32, 33, 1000, 8192)
    pools = _pools(m, len(Ls) + 1, S)
    irs = [_ir(L, 100 + L) for L in Ls]
    for p, h in zip(pools[1:], irs):
        p.set_ir(h)
    # ragged blocks past the longest IR's length, then blocks of 64 and of 256 frames on the same, continuing history
    sizes = _sizes(RAGGED, 8192 + 300) + [64] * 40 + [256] * 10
    x = modelgen.signal(S, sum(sizes), seed=20 + S)
    outs = _run(pools, x, sizes)
    for got, h in zip(outs[1:], irs):
        _check(f"S{S}", got, outs[0], h)


def test_many_streams_full_length_ir(tmp_path):
    """1024 streams, past the 8192-tap IR's full length, on 256-frame blocks and a few ragged ones"""
    m = _model(tmp_path, "c", kind="lstm", hidden=16, input_size=1, seed=9)
    S = 1024
    pools = _pools(m, 3, S)
    irs = [_ir(1000, 3), _ir(8192, 4)]
    for p, h in zip(pools[1:], irs):
        p.set_ir(h)
    sizes = [256] * 34 + [1, 17, 200]
    x = modelgen.signal(S, sum(sizes), seed=31)
    outs = _run(pools, x, sizes)
    for got, h in zip(outs[1:], irs):
        _check(f"S1024_L{h.size}", got, outs[0], h)


@pytest.mark.parametrize("S", [1, 5])
def test_every_entry_point_gives_the_same_bits(tmp_path, S):
    import torch
    m = _model(tmp_path, "e", kind="lstm", hidden=16, input_size=1, seed=13)
    h = _ir(4000, 77)
    pools = _pools(m, 4, S)
    for p in pools:
        p.set_ir(h)
    sizes = [64, 17, 256, 1, 128, 64, 255, 64, 64, 200]
    x = modelgen.signal(S, sum(sizes), seed=41)
    offs = np.concatenate([[0], np.cumsum(sizes)])
    blocks = [np.ascontiguousarray(x[:, offs[i]:offs[i + 1]]) for i in range(len(sizes))]
    # process (one stream: the zero-copy path)
    ref = np.concatenate([pools[0].process(b) for b in blocks], axis=1)
    # submit / collect with two blocks in flight
    got = []
    for i, b in enumerate(blocks):
        pools[1].submit(b)
        if i >= 2:
            got.append(pools[1].collect(sizes[i - 2]))
    got += [pools[1].collect(sizes[-2]), pools[1].collect(sizes[-1])]
    assert np.array_equal(np.concatenate(got, axis=1), ref)
    # submit_to on registered buffers (two pairs, alternating)
    cap = S * 256
    ins = [np.zeros(cap, np.float32) for _ in range(2)]
    outs = [np.zeros(cap, np.float32) for _ in range(2)]
    for a in ins + outs:
        pools[2].register_host(a)
    got = []
    for i, b in enumerate(blocks):
        k, n = i % 2, sizes[i]
        src, dst = ins[k][:S * n].reshape(S, n), outs[k][:S * n].reshape(S, n)
        src[...] = b
        pools[2].submit_to(src, dst)
        got.append(pools[2].collect(n, dst).copy())
    for a in ins + outs:
        pools[2].unregister_host(a)
    assert np.array_equal(np.concatenate(got, axis=1), ref)
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
    assert np.array_equal(np.concatenate(got, axis=1), ref)


def test_ir_swaps_on_a_worker_thread_removal_and_reset(tmp_path):
    m = _model(tmp_path, "l", kind="lstm", hidden=16, input_size=1, seed=17)
    S = 4
    wet, twin, fresh = _pools(m, 3, S)
    irs = [_ir(300, 1), _ir(8192, 2), None, _ir(33, 3), _ir(5000, 4)]
    wet.set_ir(irs[0])                                       # the history starts here; this is the first IR
    sizes = _sizes([128, 64, 1, 255, 17], 8192 * 3)
    x = modelgen.signal(S, sum(sizes), seed=51)
    todo, ready, retired = queue.Queue(), queue.Queue(), queue.Queue()
    for h in irs[1:]:
        todo.put(h)
    failure = []

    def worker():
        try:
            while True:
                h = todo.get()
                if h is False:
                    return
                while not retired.empty():
                    wet.staged_free(retired.get())
                ready.put((wet.prepare_ir(h), h))
        except Exception as e:                               # (reported by the audio side)
            failure.append(e)

    th = threading.Thread(target=worker)
    th.start()
    live, plan = irs[0], []
    got_w, got_d = [], []
    pos = 0
    try:
        for i, n in enumerate(sizes):
            if i % 25 == 24 and not ready.empty():
                sg, h = ready.get()
                wet.commit_ir(sg)
                retired.put(sg)
                live = h
            blk = np.ascontiguousarray(x[:, pos:pos + n])
            got_w.append(wet.process(blk))
            got_d.append(twin.process(blk))
            plan.append((pos, n, live))
            pos += n
    finally:
        todo.put(False)
        th.join()
    assert not failure, failure
    while not retired.empty():
        wet.staged_free(retired.get())
    while not ready.empty():
        wet.staged_free(ready.get()[0])
    assert len({id(h) for _, _, h in plan}) == len(irs), "every IR was live for some blocks"
    W, D = np.concatenate(got_w, axis=1), np.concatenate(got_d, axis=1)
    refs = {id(h): _conv64(D, h) for h in irs if h is not None}
    scale = {id(h): float(np.abs(h.astype(np.float64)).sum() * np.abs(D).max()) for h in irs if h is not None}
    for p0, n, h in plan:
        if h is None:                                        # removed: bit-identical to the twin
            assert np.array_equal(W[:, p0:p0 + n], D[:, p0:p0 + n])
        elif n:
            errlog.bound(np.abs(W[:, p0:p0 + n] - refs[id(h)][:, p0:p0 + n]).max() / scale[id(h)], 1e-5, "gpu_ir:swaps")
    # reset_stream: stream 2 matches a fresh pool's stream 2 (same IR, same stream count) from then on, bit for bit
    h = _ir(2000, 9)
    wet.set_ir(h)
    fresh.set_ir(h)
    wet.reset_stream(2)
    y = modelgen.signal(S, 4096, seed=52)
    for b in range(0, 4096, 256):
        blk = np.ascontiguousarray(y[:, b:b + 256])
        a, f = wet.process(blk), fresh.process(blk)
        assert np.array_equal(a[2], f[2]), b


@pytest.mark.parametrize("S", [1, 19])
def test_a_model_swap_under_a_live_ir_is_the_convolution_of_the_dry_output(tmp_path, S):
    """prepare_model / commit_model at the same block on a pool with an IR and on its twin without: over the swap the wet output is the
    convolution of the twin's output (the new model's first blocks sound through the IR's tail with the old model's last ones)"""
    m1 = _model(tmp_path, "s1", kind="lstm", hidden=16, input_size=1, seed=21)
    m2 = _model(tmp_path, "s2", kind="gru", hidden=24, input_size=1, seed=22)
    h = _ir(3000, 23)
    dry, wet = _pools(m1, 2, S)
    wet.set_ir(h)
    sizes = _sizes(RAGGED, 3 * 8192)
    x = modelgen.signal(S, sum(sizes), seed=24)
    swap_at = len(sizes) // 2
    outs = [[], []]
    pos = 0
    for i, n in enumerate(sizes):
        if i == swap_at:
            for p in (dry, wet):
                sg = p.prepare_model(m2)
                p.commit_model(sg)
                p.staged_free(sg)
        blk = np.ascontiguousarray(x[:, pos:pos + n])
        for o, p in zip(outs, (dry, wet)):
            o.append(p.process(blk))
        pos += n
    D, W = (np.concatenate(o, axis=1) for o in outs)
    start = int(np.sum(sizes[:swap_at]))
    assert np.abs(D[:, :start]).max() > 0.01 and np.abs(D[:, start:start + 256]).max() > 0.01
    _check(f"model_swap_S{S}", W, D, h)


def test_refusals(tmp_path):
    m = _model(tmp_path, "f", kind="lstm", hidden=16, input_size=1, seed=19)
    pool, = _pools(m, 1, 2)
    for taps, sr in ((np.zeros(0, np.float32), None), (np.ones(8193, np.float32), None), (np.array([1.0, np.nan], np.float32), None),
                     (np.array([np.inf], np.float32), None), (np.ones(4, np.float32), 44100.0)):
        with pytest.raises(ax.AidaxError) as e:
            pool.set_ir(taps, sr)
        assert e.value.code == ERR_ARG
        with pytest.raises(ax.AidaxError) as e:
            pool.prepare_ir(taps, sr)
        assert e.value.code == ERR_ARG
    # a staged IR is no model, and a staged model no IR
    sg = pool.prepare_ir(np.ones(8, np.float32))
    assert ax.lib().aidax_pool_commit_model(pool.h, sg) == ERR_ARG
    pool.commit_ir(sg)
    assert ax.lib().aidax_pool_commit_ir(pool.h, sg) == -6              # committed already
    pool.staged_free(sg)
    sm = pool.prepare_model(m)
    assert ax.lib().aidax_pool_commit_ir(pool.h, sm) == ERR_ARG
    pool.staged_free(sm)
    # n_frames == 0 (the pre-run) touches nothing
    x = modelgen.signal(2, 256, seed=3)
    a = pool.process(np.zeros((2, 0), np.float32))
    assert a.shape == (2, 0)
    pool.process(x)


@pytest.mark.parametrize("kind", ["cfg2", "stacked", "conv"])
def test_other_launch_forms_and_determinism(tmp_path, kind):
    """cfg2's pool (1024 streams, LSTM-32) with an 8192-tap IR on sampled streams; a stacked pool (k_mfma_ls: several launches per pass)
    and a conv-stack pool; two wet pools run the same blocks and must agree bit for bit"""
    kw, S, sizes = {"cfg2": (dict(kind="lstm", hidden=32, input_size=1, seed=32), 1024, [256] * 6),
                    "stacked": (dict(kind="lstm", hidden=16, input_size=1, seed=916, n_rnn=2), 40, [256, 1, 0, 37, 255, 64] * 3),
                    "conv": (dict(kind="conv", hidden=16, input_size=1, seed=4), 24, [256, 64, 17, 256] * 3)}[kind]
    m = _model(tmp_path, kind, **kw)
    dry, w1, w2 = _pools(m, 3, S)
    if kind == "stacked":
        assert "k_mfma_ls" in dry.kernel_name, dry.kernel_name
    h = _ir(8192, 1234)
    w1.set_ir(h)
    w2.set_ir(h)
    x = modelgen.signal(S, sum(sizes), seed=61)
    D, A, B = _run([dry, w1, w2], x, sizes)
    assert np.array_equal(A, B)
    rows = np.arange(S) if S <= 64 else np.array([0, 1, 15, 16, 63, 64, 511, 700, 1022, 1023])
    _check(kind, A[rows], D[rows], h)
