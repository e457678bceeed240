"""The model bank on the GPU (-m gpu): per-stream amp models as weight variants of the pool model's architecture, played by
k_lstm_pipe_bank<H> / k_gru_pipe_bank<H>.

Shapes are small on purpose: 7 streams, a pool model and three slot models of other seeds (one with in_skip = 1, all with their own
in_gain / out_gain), ragged blocks [1, 17, 0, 64, 33, 256, 16] repeated over 1935 frames of modelgen.signal.

Bars. A banked stream runs the same instructions on the same numbers as the same stream of a pool whose POOL model is that stream's
file on k_*_pipe (the twin), so everything against a twin is np.array_equal. Against the oracle the bar is the project's own
(tests/test_gpu_parity.py): THR * max(1, downstream linear gain) with THR = 1e-5 (TEST_MODEL_THR, rt-neural-generic.h:182) and the
downstream gain of a stream = its model's linear out_gain x DB_CO(master_db) x the EQ's largest possible gain (the product of its
positive boosts, 1 with the EQ flat or bypassed). No measured number is in it; the measured maxima go through tests/errlog.py."""
import importlib

import numpy as np
import pytest

from oracle import oracle as O
from tests import errlog, modelgen
from tests.test_gpu_ir_bank_rt import _Device, _quiet, calls        # noqa: F401  (the call-table fixture: it skips on the ship leg)

pytestmark = pytest.mark.gpu
ax = importlib.import_module("aidadsp-lv2_amd")

THR = 1.0e-5
ERR_ARG, ERR_ARCH, ERR_STATE = -1, -4, -6
S = 7
PLAN = [1, 17, 0, 64, 33, 256, 16]
SIZES = PLAN * 5                                            # 1935 frames
N = sum(SIZES)
KEYS = (ax.MODEL_POOL, 0, 1, 2)                             # stream s plays KEYS[s % 4]
EQ = dict(bass_boost_db=4.0, mid_boost_db=-3.0, mid_freq=750.0, mid_q=1.2, treble_boost_db=2.0, presence_boost_db=3.0)


def _files(tmp_path, kind, hidden, isz):
    """[(path, spec)] for the pool model and slots 0 .. 2: one architecture, four seeds, distinct gains, slot 1 with in_skip"""
    out = []
    for k, kw in enumerate((dict(in_gain=1.5, out_gain=-1.0), dict(in_gain=-2.0, out_gain=2.5), dict(in_skip=1, in_gain=-4.0, out_gain=-3.0),
                            dict(in_gain=3.0, out_gain=4.0))):
        j = modelgen.make_model(kind=kind, hidden=hidden, input_size=isz, seed=7000 + 10 * hidden + k, **kw)
        p = str(tmp_path / f"{kind}{hidden}_{isz}_{k}.json")
        modelgen.write_model(j, p)
        out.append((p, O.parse_model(j)))
    return out


def _key_file(key):
    return 0 if key == ax.MODEL_POOL else key + 1


def _banked_pool(files, n_streams=S, max_frames=256, assign=True, samplerate=48000.0):
    pool = ax.Pool(n_streams, max_frames, samplerate)
    pool.set_model(ax.Model(files[0][0]))
    for k in range(3):
        pool.set_model_slot(k, ax.Model(files[k + 1][0]))
    if assign:
        for s in range(n_streams):
            pool.assign_model(s, KEYS[s % 4], ax.START_WARMUP)
    return pool


def _params(bi):
    return dict(param1=0.1 + 0.025 * (bi % 30), param2=0.9 - 0.02 * (bi % 35))


def _drive(pool, x, sizes=SIZES, ctl=None, events=None):
    """x through pool.process in blocks of `sizes`; ctl(bi) -> control kwargs of block bi (None: untouched); events[bi](pool) runs first"""
    out = np.empty_like(x)
    pos = 0
    for bi, n in enumerate(sizes):
        if events and bi in events:
            events[bi](pool)
        if ctl is not None:
            pool.set_controls(ax.default_controls(**ctl(bi)))
        out[:, pos:pos + n] = pool.process(np.ascontiguousarray(x[:, pos:pos + n]))
        pos += n
    return out


def _bar(spec, ctl_kw):
    c = ax.default_controls(**ctl_kw)
    g = spec.output_gain * 10.0 ** (c.master_db / 20.0)
    if c.eq_bypass == 0.0:
        boosts = (c.bass_boost_db, c.mid_boost_db, c.treble_boost_db, c.depth_boost_db, c.presence_boost_db)
        g *= 10.0 ** (sum(max(0.0, b) for b in boosts) / 20.0)
    return THR * max(1.0, g)


CELLS = [("lstm", 12, 1), ("lstm", 32, 1), ("lstm", 40, 1), ("gru", 8, 1), ("gru", 40, 1), ("lstm", 16, 2), ("lstm", 16, 3)]
_RUNS = {}


def _banked_run(tmp_path, kind, hidden, isz):
    """the banked pool's run of a cell, computed once per session: (files, x, output, [(h, c)] per stream, kernel name)"""
    key = (kind, hidden, isz)
    if key not in _RUNS:
        files = _files(tmp_path, kind, hidden, isz)
        x = modelgen.signal(S, N, seed=2024 + hidden)
        pool = _banked_pool(files)
        name = pool.kernel_name
        got = _drive(pool, x, ctl=_params if isz > 1 else None)
        states = [pool.read_state(s, hidden=hidden) for s in range(S)]
        assert [pool.stream_model(s) for s in range(S)] == [KEYS[s % 4] for s in range(S)]
        pool.close()
        _RUNS[key] = (files, x, got, states, name)
    return _RUNS[key]


# ---------------------------------------------------------------- 1: bit identity with one-model pools

@pytest.mark.parametrize("kind,hidden,isz", CELLS)
def test_banked_streams_are_their_twins_bit_for_bit(kind, hidden, isz, tmp_path, monkeypatch):
    files, x, got, states, name = _banked_run(tmp_path, kind, hidden, isz)
    assert name == f"k_{kind}_pipe_bank<{hidden}>"
    monkeypatch.setenv("AIDAX_PIPE4", "0")                  # the twins on k_*_pipe at every block length
    for key in KEYS:
        twin = ax.Pool(S, 256)
        twin.set_model(ax.Model(files[_key_file(key)][0]))
        assert twin.kernel_name == f"k_{kind}_pipe<{hidden}>"
        want = _drive(twin, x, ctl=_params if isz > 1 else None)
        for s in range(S):
            if KEYS[s % 4] != key:
                continue
            assert np.abs(want[s]).max() > 1e-3
            assert np.array_equal(got[s].view(np.uint32), want[s].view(np.uint32)), (key, s)
            h, c = twin.read_state(s, hidden=hidden)
            assert np.array_equal(states[s][0], h) and np.array_equal(states[s][1], c), (key, s)
        twin.close()
    # the four keys really differ (a Dense row or a gain read from the pool model would pass a weaker test)
    assert not np.array_equal(got[0], got[1]) and not np.array_equal(got[1], got[2])


# ---------------------------------------------------------------- 2: against the oracle

@pytest.mark.parametrize("kind,hidden,isz", CELLS)
def test_banked_streams_against_the_oracle(kind, hidden, isz, tmp_path):
    files, x, got, _, _ = _banked_run(tmp_path, kind, hidden, isz)
    for s in range(S):
        spec = files[_key_file(KEYS[s % 4])][1]
        plug = O.OraclePlugin()
        plug.set_model(O.OracleModel(spec))
        want = np.empty(N, np.float32)
        pos = 0
        for bi, n in enumerate(SIZES):
            kw = _params(bi) if isz > 1 else {}
            want[pos:pos + n] = plug.run(O.default_controls(**kw), x[s, pos:pos + n])
            pos += n
        err = float(np.abs(got[s] - want).max())
        bar = _bar(spec, {})
        print(f"model bank {kind}{hidden} in{isz} stream {s} (key {KEYS[s % 4]}): max |gpu - oracle| = {err:.3e}, bar {bar:.3e}")
        errlog.bound(err / bar, 1.0, f"model_bank:oracle_{kind}{hidden}_in{isz}")


# ---------------------------------------------------------------- 3: assignment mid-run

def test_streams_move_between_models_mid_run(tmp_path):
    """LSTM-16 with PARAM1 / PARAM2 as inputs, the EQ in circuit. Before block 0: stream 2 -> slot 1, 5 -> slot 0, 6 -> slot 2. Then
    stream 1: pool -> slot 0 (block 3, warm-up) -> pool (block 9, warm-up); stream 2: slot 1 -> slot 2 (block 6, reset only); stream 5:
    slot 0 reloaded (block 12); stream 3: pool -> slot 2 at block 16 with `loading` set from block 15 to block 17. Streams 0, 4, 6 stay."""
    files = _files(tmp_path, "lstm", 16, 3)
    x = modelgen.signal(S, N, seed=99)
    ctl_kw = dict(EQ, master_db=-2.0, pregain_db=3.0)

    def ctl(bi):
        return dict(ctl_kw, **_params(bi))
    start = {2: 1, 5: 0, 6: 2}
    moves = {3: (1, 0, ax.START_WARMUP), 6: (2, 2, ax.START_RESET), 9: (1, ax.MODEL_POOL, ax.START_WARMUP), 12: (5, 0, ax.START_WARMUP),
             16: (3, 2, ax.START_WARMUP)}
    loading = {15: (3, True), 17: (3, False)}

    def make(with_moves):
        pool = _banked_pool(files, assign=False)
        for s, k in start.items():
            pool.assign_model(s, k, ax.START_WARMUP)
        events = {}
        if with_moves:
            for bi, (s, k, mode) in moves.items():
                events[bi] = (lambda p, s=s, k=k, mode=mode: p.assign_model(s, k, mode))
            for bi, (s, on) in loading.items():
                events[bi] = (lambda p, s=s, on=on: p.set_loading(on, s))
        return pool, events
    pool, events = make(True)
    got = _drive(pool, x, ctl=ctl, events=events)
    assert [pool.stream_model(s) for s in range(S)] == [-1, -1, 2, 2, -1, 0, 2]
    pool.close()
    still, ev0 = make(False)
    ref = _drive(still, x, ctl=ctl, events=ev0)
    still.close()
    for s in (0, 4, 6):
        assert np.array_equal(got[s].view(np.uint32), ref[s].view(np.uint32)), s
    for s in (1, 2, 3, 5):
        assert not np.array_equal(got[s], ref[s]), s
    # the oracle: one plugin per stream, its model replaced at the same boundaries around the PARAM targets the old one holds
    for s in range(S):
        key = start.get(s, ax.MODEL_POOL)
        plug = O.OraclePlugin()
        plug.set_model(O.OracleModel(files[_key_file(key)][1]))
        pos = 0
        worst = 0.0
        for bi, n in enumerate(SIZES):
            if bi in moves and moves[bi][0] == s:
                _, key, mode = moves[bi]
                old = plug.model.ptr.contents
                plug.set_model(O.OracleModel(files[_key_file(key)][1], old.param1Coeff.target, old.param2Coeff.target,
                                             warmup=mode == ax.START_WARMUP))
            if bi in loading and loading[bi][0] == s:
                plug.set_loading(loading[bi][1])
            want = plug.run(O.default_controls(**ctl(bi)), x[s, pos:pos + n])
            if n:                                           # every block against the bar of the model it plays
                worst = max(worst, float(np.abs(got[s, pos:pos + n] - want).max()) / _bar(files[_key_file(key)][1], ctl_kw))
            pos += n
        print(f"model bank moves, stream {s}: max |gpu - oracle| / bar = {worst:.3e}")
        errlog.bound(worst, 1.0, "model_bank:moves")


# ---------------------------------------------------------------- 4: a loaded but unused bank changes nothing

@pytest.mark.parametrize("n_streams,sizes", [(S, PLAN * 2), (8, [64, 16, 256, 64])])
def test_a_loaded_but_unused_bank_changes_nothing(n_streams, sizes, tmp_path):
    files = _files(tmp_path, "lstm", 16, 1)
    x = modelgen.signal(n_streams, sum(sizes), seed=5)
    plain = ax.Pool(n_streams, 256)
    plain.set_model(ax.Model(files[0][0]))
    banked = _banked_pool(files, n_streams=n_streams, assign=False)
    old_name = plain.kernel_name
    assert banked.kernel_name == old_name
    if n_streams == 8:
        assert old_name == "k_lstm_pipe4<16>"              # whole tiles, two full workgroups: the four-stream pipeline serves
    half = len(sizes) // 2
    a = _drive(plain, x[:, :sum(sizes[:half])], sizes[:half])
    b = _drive(banked, x[:, :sum(sizes[:half])], sizes[:half])
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32)) and np.abs(a).max() > 1e-3
    # one stream visits a slot and returns: the bank kernel's name while it is there, the old name again afterwards
    banked.assign_model(n_streams - 1, 1, ax.START_RESET)
    assert banked.kernel_name == "k_lstm_pipe_bank<16>"
    banked.assign_model(n_streams - 1, ax.MODEL_POOL, ax.START_RESET)
    assert banked.kernel_name == old_name
    # (the visitor is a fresh DynamicModel now: every other stream goes on as if nothing had happened)
    rest = x[:, sum(sizes[:half]):]
    a = _drive(plain, rest, sizes[half:])
    b = _drive(banked, rest, sizes[half:])
    assert np.array_equal(a[:-1].view(np.uint32), b[:-1].view(np.uint32))
    plain.close()
    banked.close()


# ---------------------------------------------------------------- 5: passes see their own records

def _three_blocks(files):
    """reference for the ordering tests: blocks 0 and 1 with stream 1 on slot 0 and stream 2 on slot 1, then 1 -> slot 2 and
    2 -> pool, block 2 — one blocking call after the other"""
    x = modelgen.signal(S, 3 * 256, seed=31)
    pool = _banked_pool(files)
    blocks = [np.ascontiguousarray(x[:, i * 256:(i + 1) * 256]) for i in range(3)]
    want = [pool.process(blocks[0]), pool.process(blocks[1])]
    pool.assign_model(1, 2, ax.START_WARMUP)
    pool.assign_model(2, ax.MODEL_POOL, ax.START_WARMUP)
    want.append(pool.process(blocks[2]))
    pool.close()
    return blocks, want


def test_blocks_in_flight_play_the_assignment_they_were_issued_with(tmp_path):
    files = _files(tmp_path, "lstm", 32, 1)
    blocks, want = _three_blocks(files)
    pool = _banked_pool(files)
    pool.submit(blocks[0])
    pool.submit(blocks[1])
    pool.assign_model(1, 2, ax.START_WARMUP)
    pool.assign_model(2, ax.MODEL_POOL, ax.START_WARMUP)
    pool.submit(blocks[2])
    got = [pool.collect(256) for _ in range(3)]
    pool.close()
    for k in range(3):
        assert np.array_equal(got[k].view(np.uint32), want[k].view(np.uint32)), k
    assert not np.array_equal(want[1][1], want[2][1])


def test_passes_on_a_callers_stream_play_the_assignment_they_were_issued_with(tmp_path):
    import torch
    files = _files(tmp_path, "lstm", 32, 1)
    blocks, want = _three_blocks(files)
    pool = _banked_pool(files)
    st = torch.cuda.Stream()
    d_in = [torch.from_numpy(b).cuda() for b in blocks]
    d_out = [torch.empty((S, 256), dtype=torch.float32, device="cuda") for _ in range(3)]
    torch.cuda.synchronize()
    pool.process_device(d_in[0].data_ptr(), d_out[0].data_ptr(), 256, st.cuda_stream)
    pool.process_device(d_in[1].data_ptr(), d_out[1].data_ptr(), 256, st.cuda_stream)
    pool.assign_model(1, 2, ax.START_WARMUP)
    pool.assign_model(2, ax.MODEL_POOL, ax.START_WARMUP)
    pool.process_device(d_in[2].data_ptr(), d_out[2].data_ptr(), 256, st.cuda_stream)
    pool.sync()
    st.synchronize()
    for k in range(3):
        assert np.array_equal(d_out[k].cpu().numpy().view(np.uint32), want[k].view(np.uint32)), k
    pool.close()


def test_the_rate_adapter_around_a_banked_pool_is_its_parts(tmp_path):
    """44.1 kHz host blocks around banked pools at 48 kHz, as tests/test_gpu_rate.py composes them: adapter = resampler + pool +
    resampler bit for bit, with an assignment between two host blocks"""
    import torch
    from tests import rateref as rr
    files = _files(tmp_path, "lstm", 16, 1)
    host, pool_rate = 44100, 48000
    host_blocks = (64, 1, 0, 255, 17, 256, 0, 7, 128)
    p1, p2 = _banked_pool(files, max_frames=288), _banked_pool(files, max_frames=288)
    ad = ax.RateAdapter(p1, float(host), 256)
    H_A, d_B = rr.delays(host, pool_rate)
    A = ax.Resampler(S, float(host), float(pool_rate), H_A, 0, 256)
    B = ax.Resampler(S, float(pool_rate), float(host), 0, d_B, 288)
    x = modelgen.signal(S, sum(host_blocks), seed=77)
    st = torch.cuda.Stream()
    got, want, at = [], [], 0
    with torch.cuda.stream(st):
        for bi, (n, m) in enumerate(zip(host_blocks, rr.pool_frames(host_blocks, host, pool_rate))):
            if bi == 4:
                for p in (p1, p2):
                    p.assign_model(0, 1, ax.START_WARMUP)
                    p.assign_model(1, ax.MODEL_POOL, ax.START_RESET)
            d_x = torch.from_numpy(np.ascontiguousarray(x[:, at:at + n])).cuda()
            at += n
            y1, y2 = torch.empty((S, n), dtype=torch.float32, device="cuda"), torch.empty((S, n), dtype=torch.float32, device="cuda")
            ya, yb = torch.empty((S, m), dtype=torch.float32, device="cuda"), torch.empty((S, m), dtype=torch.float32, device="cuda")
            ad.process_device(d_x.data_ptr() if n else 0, y1.data_ptr() if n else 0, n, st.cuda_stream)
            if n == 0:
                p2.process_device(0, 0, 0, st.cuda_stream)
            else:
                A.process_device(d_x.data_ptr(), n, ya.data_ptr() if m else 0, m, st.cuda_stream)
                p2.process_device(ya.data_ptr() if m else 0, yb.data_ptr() if m else 0, m, st.cuda_stream)
                B.process_device(yb.data_ptr() if m else 0, m, y2.data_ptr(), n, st.cuda_stream)
            st.synchronize()
            got.append(y1.cpu().numpy())
            want.append(y2.cpu().numpy())
    got, want = np.concatenate(got, axis=1), np.concatenate(want, axis=1)
    assert p1.kernel_name == "k_lstm_pipe_bank<16>" and np.abs(want).max() > 1e-3
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    for h in (A, B, ad, p1, p2):
        h.close()


# ---------------------------------------------------------------- 6: life cycle and refusals

def _code(fn, *a):
    with pytest.raises(ax.AidaxError) as e:
        fn(*a)
    return e.value.code


def test_refused_calls_change_nothing(tmp_path):
    """(blocks of 60 frames: no whole tiles, so the pools without an assigned stream run k_gru_pipe too)"""
    files = _files(tmp_path, "gru", 8, 1)
    x = modelgen.signal(S, 4 * 60, seed=8)
    blocks = [np.ascontiguousarray(x[:, i * 60:(i + 1) * 60]) for i in range(4)]
    a, b = _banked_pool(files, max_frames=64), _banked_pool(files, max_frames=64)
    plain = ax.Pool(S, 64)
    plain.set_model(ax.Model(files[0][0]))
    for p in (a, b):                                        # slot 2 empty in both: its streams move to slot 0 first
        for s in range(S):
            if p.stream_model(s) == 2:
                p.assign_model(s, 0, ax.START_RESET)
        p.set_model_slot(2, None)
    ya, yb, y0 = a.process(blocks[0]), b.process(blocks[0]), plain.process(blocks[0])
    assert np.array_equal(ya.view(np.uint32), yb.view(np.uint32))
    ma = ax.Model(files[3][0])
    # a commit into an assigned slot (content and NULL), a pool-model commit under assigned streams, an assignment to an empty slot
    assert _code(a.set_model_slot, 0, ma) == ERR_STATE
    assert _code(a.set_model_slot, 0, None) == ERR_STATE
    assert _code(a.set_model, ax.Model(files[2][0])) == ERR_STATE and "empty the model bank first" in ax.last_error()
    assert _code(a.set_model, None) == ERR_STATE
    assert _code(a.assign_model, 3, 2) == ERR_STATE
    assert _code(a.assign_model, S, 0) == ERR_ARG and _code(a.assign_model, ax.ALL_STREAMS, 0) == ERR_ARG
    assert _code(a.assign_model, 0, ax.MODEL_SLOTS) == ERR_ARG and _code(a.assign_model, 0, 0, 7) == ERR_ARG
    assert _code(a.set_model_slot, ax.MODEL_SLOTS, ma) == ERR_ARG
    assert [a.stream_model(s) for s in range(S)] == [b.stream_model(s) for s in range(S)]
    ya, yb, y1 = a.process(blocks[1]), b.process(blocks[1]), plain.process(blocks[1])
    assert np.array_equal(ya.view(np.uint32), yb.view(np.uint32)) and np.abs(ya).max() > 1e-3
    # the replace-a-model recipe: load a free slot, move the streams, empty the old one; staged_free before and after the next pass
    late = []
    for p, free_early in ((a, True), (b, False)):
        staged = [p.prepare_model_slot(5, ma)]
        p.commit_model(staged[0])
        for s in range(S):
            if p.stream_model(s) == 0:
                p.assign_model(s, 5, ax.START_WARMUP)
        staged.append(p.prepare_model_slot(0, None))
        p.commit_model(staged[1])
        if free_early:
            for sg in staged:
                p.staged_free(sg)
        else:
            late = staged
    ya, yb, y2 = a.process(blocks[2]), b.process(blocks[2]), plain.process(blocks[2])
    for sg in late:
        b.staged_free(sg)
    assert np.array_equal(ya.view(np.uint32), yb.view(np.uint32))
    assert _code(a.assign_model, 0, 0) == ERR_STATE        # slot 0 is empty now
    # with nobody assigned and every loaded slot compatible the pool model may change; an unload may not while a slot is loaded
    for s in range(S):
        a.assign_model(s, ax.MODEL_POOL, ax.START_RESET)
    assert a.kernel_name == plain.kernel_name
    assert _code(a.set_model, None) == ERR_STATE
    assert _code(a.set_model, ax.Model(_files(tmp_path, "lstm", 8, 1)[0][0])) == ERR_STATE      # a loaded slot would not fit
    a.set_model(ax.Model(files[2][0]))
    plain.set_model(ax.Model(files[2][0]))
    a.assign_model(6, 1, ax.START_WARMUP)                   # the bank kernel: every other stream reads the NEW pool model's record
    assert a.kernel_name == "k_gru_pipe_bank<8>"
    ya, y3 = a.process(blocks[3]), plain.process(blocks[3])
    # streams 0 and 4 have played the pool model all along: they are the plain pool's, whose pool model changed at the same boundary
    for s in (0, 4):
        assert np.array_equal(ya[s].view(np.uint32), y3[s].view(np.uint32)) and np.abs(y3[s]).max() > 1e-3
    for p in (a, b, plain):
        p.close()


def test_what_cannot_carry_a_bank_says_so(tmp_path):
    g64 = _files(tmp_path, "gru", 64, 1)
    pool = ax.Pool(S, 256)
    pool.set_model(ax.Model(g64[0][0]))
    assert pool.kernel_name == "k_gru_gs"
    assert _code(pool.set_model_slot, 0, ax.Model(g64[1][0])) == ERR_ARCH and "k_gru_gs" in ax.last_error()
    pool.close()
    l64 = _files(tmp_path, "lstm", 64, 1)
    pool = ax.Pool(S, 256)
    pool.set_model(ax.Model(l64[0][0]))
    assert _code(pool.set_model_slot, 0, ax.Model(l64[1][0])) == ERR_ARCH
    pool.close()
    l16 = _files(tmp_path, "lstm", 16, 1)
    pool = ax.Pool(S, 256)
    assert _code(pool.set_model_slot, 0, ax.Model(l16[1][0])) == ERR_STATE          # the pool has no model
    pool.set_model(ax.Model(l16[0][0]))
    other = _files(tmp_path, "lstm", 20, 1)
    assert _code(pool.set_model_slot, 0, ax.Model(other[1][0])) == ERR_ARCH and "hidden" in ax.last_error()
    assert _code(pool.set_model_slot, 0, ax.Model(_files(tmp_path, "lstm", 16, 2)[1][0])) == ERR_ARCH and "input_size" in ax.last_error()
    # a slot prepared for one pool model is refused by the commit once the pool model is another architecture
    sg = pool.prepare_model_slot(3, ax.Model(l16[1][0]))
    pool.set_model(ax.Model(other[0][0]))
    assert _code(pool.commit_model, sg) == ERR_STATE
    pool.staged_free(sg)
    pool.close()


def test_ir_bank_and_model_bank_on_one_stream_and_reset_keeps_the_assignment(tmp_path):
    files = _files(tmp_path, "lstm", 12, 1)
    x = modelgen.signal(S, 2 * 120, seed=12)                # (120 frames: no whole tiles, so a pool without a bank runs k_lstm_pipe)
    b0, b1 = np.ascontiguousarray(x[:, :120]), np.ascontiguousarray(x[:, 120:])
    dry, wet = _banked_pool(files, max_frames=128), _banked_pool(files, max_frames=128)
    ir = np.zeros(4, np.float32)
    ir[3] = 0.5                                             # a delay of three frames and a gain of 2^-1: exact
    wet.set_ir_slot(5, ir)
    wet.assign_ir(ax.ALL_STREAMS, ax.IR_NONE)
    wet.assign_ir(2, 5)
    assert wet.stream_ir(2) == 5 and wet.stream_model(2) == 1
    yd, yw = dry.process(b0), wet.process(b0)
    want = np.zeros(120, np.float32)
    want[3:] = 0.5 * yd[2, :-3]
    assert np.array_equal(yw[2], want) and np.array_equal(np.delete(yw, 2, 0), np.delete(yd, 2, 0))
    # reset_stream: a fresh instance that still plays its slot, warmed up with the slot's weights
    dry.reset_stream(2, ax.START_WARMUP)
    assert dry.stream_model(2) == 1 and dry.kernel_name == "k_lstm_pipe_bank<12>"
    fresh = ax.Pool(S, 128)
    fresh.set_model(ax.Model(files[2][0]))                  # a pool whose pool model is slot 1's file: stream 2 as just created
    got, ref = dry.process(b1), fresh.process(b1)
    assert np.array_equal(got[2].view(np.uint32), ref[2].view(np.uint32)) and np.abs(ref[2]).max() > 1e-3
    for p in (dry, wet, fresh):
        p.close()


# ---------------------------------------------------------------- 7: the one-stream pool of a plugin instance

def test_a_one_stream_pool_on_a_slot_through_the_blocking_path(tmp_path):
    """aidax_pool_process of a one-stream pool: zero-copy, the completion word written by the bank kernel's workgroup. 200 blocks of 64
    frames of fresh noise against the twin whose pool model is the slot's file (k_lstm_pipe at one stream, no hook needed)."""
    files = _files(tmp_path, "lstm", 16, 1)
    pool = ax.Pool(1, 64)
    pool.set_model(ax.Model(files[0][0]))
    pool.set_model_slot(9, ax.Model(files[2][0]))
    pool.assign_model(0, 9, ax.START_WARMUP)
    twin = ax.Pool(1, 64)
    twin.set_model(ax.Model(files[2][0]))
    assert pool.kernel_name == "k_lstm_pipe_bank<16>" and twin.kernel_name == "k_lstm_pipe<16>"
    rng = np.random.default_rng(64)
    for k in range(200):
        blk = rng.uniform(-0.5, 0.5, (1, 64)).astype(np.float32)
        a, b = pool.process(blk), twin.process(blk)
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), k
    assert np.abs(a).max() > 1e-4
    pool.close()
    twin.close()


# ---------------------------------------------------------------- 8: the audio-side calls in real time


def test_assignments_and_slot_commits_allocate_free_and_wait_for_nothing(tmp_path, calls):
    """aidax_pool_assign_model and the commit of a prepared slot on the audio thread, and the two passes behind each: nothing that
    allocates, frees or waits among the pool's HIP calls (tests/test_gpu_ir_bank_rt.py's sets). The first pass behind an assignment
    uploads the changed records — one hipMemcpyAsync more than a pass with nothing to upload — and the second one nothing."""
    files = _files(tmp_path, "lstm", 16, 1)
    pool = ax.Pool(6, 64)
    pool.set_model(ax.Model(files[0][0]))
    for k in range(2):
        pool.set_model_slot(k, ax.Model(files[k + 1][0]))
    dev = _Device(6, 64, seed=21)
    dev.pass_(pool)
    dev.wait()
    calls()
    dev.pass_(pool)
    idle = calls()
    _quiet(idle, "pass with nothing dirty")
    dev.wait()

    def two_passes(what, uploads):
        for k in range(2):
            dev.pass_(pool)
            c = calls()
            _quiet(c, f"pass {k} after {what}")
            assert c.get("hipMemcpyAsync", 0) == idle.get("hipMemcpyAsync", 0) + (uploads if k == 0 else 0), (what, k, c, idle)
        dev.wait()
        calls()
    # (stream 4 stays on its slot, so the bank is in force behind every assignment; the last one moves stream 1 back with a warm-up)
    for stream, slot, mode in ((1, 0, ax.START_RESET), (4, 1, ax.START_RESET), (1, ax.MODEL_POOL, ax.START_WARMUP)):
        pool.assign_model(stream, slot, mode)
        _quiet(calls(), f"assign_model({stream}, {slot})")
        assert pool.kernel_name == "k_lstm_pipe_bank<16>"
        two_passes(f"assign_model({stream}, {slot})", 1)
    assert [pool.stream_model(s) for s in range(6)] == [-1, -1, -1, -1, 1, -1]
    for slot, m in ((0, ax.Model(files[3][0])), (2, ax.Model(files[3][0])), (0, None)):      # replace a loaded slot, load an empty one, empty one
        sg = pool.prepare_model_slot(slot, m)               # (worker side)
        calls()
        pool.commit_model(sg)                               # audio side
        c = calls()
        _quiet(c, "commit_model of a slot")
        assert c.get("hipEventRecord", 0) >= 1, c           # the fence the retired weights wait for
        two_passes("commit_model of a slot", 0)
        pool.staged_free(sg)                                # (worker side)
        calls()
    pool.close()
