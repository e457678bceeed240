"""A post EQ that computes nothing is not run (run with -m gpu on an MI355X).

At the TTL defaults the five EQ stages behind the model are exact identities — 0 dB designs with a0 == 1, a1 == b1, a2 == b2 — and from
zero state they stay that: eq_stage_transparent (aidax_device.h) says so at the head of every launch, on the device, from what the launch
has loaded, and k_*_pipe4 then runs the post cascade with its first stage alone. The skip must be invisible:

  * GPU against GPU, the same build: a pool that skips against a pool with AIDAX_TUNE bit 4 (kTuneEqFull, test build: the full cascade
    whatever the coefficients) — outputs of every block and the read-back stream state (z, gain memories and targets, the PARAM smoothers,
    `pending`: the first 156 bytes of the record; h / c) equal as bytes. The NN is not bit-exact against the oracle, this comparison is.
  * where the model is out of circuit the chain alone IS bit-exact against the oracle: the sign of every zero (five identity stages turn
    -0.0 into +0.0, the shortened cascade must too), denormals, and a sample that is not finite (it passes, poisons the first stage's
    state, and every later sample is NaN — in that launch and in the ones after it).

That the skip was TAKEN (or not) is read from a word only the test build writes: StreamState::pad = the length of the post cascade the
last k_*_pipe4 / k_*_pipe launch ran for the stream (aidax_test_stream_state, test build only).

Shapes: 8 streams (two workgroups) and 5 (a ragged last one); blocks of 64 and 256 frames, and of 48 (three whole tiles: k_*_pipe4 as
well) and 40 (no whole tiles: the three-wave k_*_pipe, which runs every stage — the same pools' ragged blocks, and the comparisons
hold whichever form has the skip); LSTM-8 and LSTM-32; six blocks each, so that state carries over.
"""
import ctypes as C
import importlib
import json

import numpy as np
import pytest

from oracle import oracle as O

pytestmark = pytest.mark.gpu

ax = importlib.import_module("aidadsp-lv2_amd")
W = ax.workloads

FULL = "4"                     # AIDAX_TUNE: kTuneEqFull (aidax_layout.h)
NBLK = 6
REC = 160                      # sizeof(StreamState); [0, 112) z[7][2], [112, 152) ten floats, [152] pending, [156] pad
_models = {}


def _model(tmp_path_factory, hidden):
    if hidden not in _models:
        j = W.make_model("lstm", hidden, 1, seed=hidden)
        path = W.write_model(j, str(tmp_path_factory.mktemp("eqt") / f"lstm{hidden}.json"))
        _models[hidden] = (path, O.parse_model(json.loads(json.dumps(j))))
    return _models[hidden]


def _record(pool, s):
    buf = (C.c_uint8 * REC)()
    rc = ax.lib().aidax_test_stream_state(pool.h, C.c_uint32(s), buf, C.c_uint32(REC))
    assert rc == REC, rc
    return bytes(buf)


def _pad(rec):
    return int(np.frombuffer(rec[156:160], np.uint32)[0])


def _z(rec):
    return np.frombuffer(rec[:112], np.float64).reshape(7, 2)


def _run(path, hidden, S, n, x, schedule, records=True):
    """one pool over NBLK blocks of n frames; schedule[block] = [(stream or None, controls kwargs)] applied in front of that block.
    -> (kernel name, outputs [S][NBLK n], per block the streams' records, per stream (h, c) at the end)"""
    pool = ax.Pool(S, n)
    pool.set_model(ax.Model(path))
    name = pool.kernel_name
    out = np.empty_like(x)
    recs = []
    for b in range(NBLK):
        for s_, kw in schedule.get(b, []):
            pool.set_controls(ax.default_controls(**kw), **({} if s_ is None else dict(stream=s_)))
        out[:, b * n:(b + 1) * n] = pool.process(np.ascontiguousarray(x[:, b * n:(b + 1) * n]))
        if records:
            recs.append([_record(pool, s) for s in range(S)])
    hc = [pool.read_state(s, 0, hidden) for s in range(S)]
    pool.close()
    return name, out, recs, hc


def _pair(monkeypatch, path, hidden, S, n, x, schedule):
    """the same run twice on one build: as shipped (skip), and with the full cascade forced. Asserts that both are equal to the byte —
    every block's output, every block's stream records but the test build's word, h / c at the end — and returns both runs."""
    monkeypatch.setenv("AIDAX_TUNE", FULL)                      # (read when a pool is created)
    full = _run(path, hidden, S, n, x, schedule)
    monkeypatch.delenv("AIDAX_TUNE")
    skip = _run(path, hidden, S, n, x, schedule)
    assert skip[0] == full[0]
    for b in range(NBLK):
        for s in range(S):
            assert skip[1][s, b * n:(b + 1) * n].tobytes() == full[1][s, b * n:(b + 1) * n].tobytes(), ("output", b, s)
            assert skip[2][b][s][:156] == full[2][b][s][:156], ("stream record", b, s)
    for s in range(S):
        assert skip[3][s][0].tobytes() == full[3][s][0].tobytes() and skip[3][s][1].tobytes() == full[3][s][1].tobytes(), ("h / c", s)
    assert np.isfinite(skip[1]).all()
    return skip, full


def _form(hidden, n):
    """whole tiles of sixteen frames run the four-streams-per-workgroup pipeline, every other length the three-wave one"""
    return f"k_lstm_pipe4<{hidden}>" if n % 16 == 0 else f"k_lstm_pipe<{hidden}>"


def _k(n):
    """the post cascade a transparent EQ leaves: one stage where the form skips it (k_*_pipe4), all six where it does not (k_*_pipe)"""
    return 1 if n % 16 == 0 else 6


def _pads(run, b):
    return [_pad(r) for r in run[2][b]]


@pytest.mark.parametrize("n", [64, 256, 48, 40])
@pytest.mark.parametrize("S", [8, 5])
@pytest.mark.parametrize("hidden", [8, 32])
def test_default_controls_skip_the_post_eq_and_nothing_changes(tmp_path_factory, monkeypatch, hidden, S, n):
    path, _ = _model(tmp_path_factory, hidden)
    x = W.signal(S, NBLK * n, seed=1000 + n)
    skip, full = _pair(monkeypatch, path, hidden, S, n, x, {0: [(None, {})]})
    assert skip[0] == _form(hidden, n)
    for b in range(NBLK):                                       # the skip was taken, by every stream in every launch — and not under the switch
        assert _pads(skip, b) == [_k(n)] * S and _pads(full, b) == [6] * S, b
    for s in range(S):                                          # the EQ's state is the zero it was
        assert not _z(skip[2][-1][s])[2:].any()


@pytest.mark.parametrize("hidden,S,n", [(32, 8, 64), (8, 5, 256), (32, 5, 48), (8, 8, 40)])
def test_mixed_workgroup_every_stream_runs_its_own_cascade(tmp_path_factory, monkeypatch, hidden, S, n):
    """one workgroup: default | mid + 4 dB | boosted for two blocks and then flat (its state decays: all stages) | EQ bypassed"""
    path, _ = _model(tmp_path_factory, hidden)
    x = W.signal(S, NBLK * n, seed=2000 + n)
    schedule = {0: [(None, {}), (1, dict(mid_boost_db=4.0)), (2, dict(bass_boost_db=5.0, presence_boost_db=3.0)), (3, dict(eq_bypass=1.0))],
                2: [(2, {})]}
    skip, full = _pair(monkeypatch, path, hidden, S, n, x, schedule)
    for b in range(NBLK):
        assert _pads(skip, b) == [_k(n), 6, 6, 1] + [_k(n)] * (S - 4), b
        assert _pads(full, b) == [6, 6, 6, 1] + [6] * (S - 4), b
    z = _z(skip[2][-1][2])
    # the bass shelf is still ringing four blocks after the boost went (305 Hz: poles at radius 0.97, 0.97^1024 = 3e-14 of what it held; the
    # presence shelf at 900 Hz, radius 0.92, may have reached exact zero by then — 0.92^1024 is under the smallest denormal — and the stream
    # runs all stages as long as ANY stage has state)
    assert z[3].all()
    assert z.tobytes() == _z(full[2][-1][2]).tobytes()


@pytest.mark.parametrize("hidden,S,n", [(32, 5, 64), (8, 8, 256), (32, 5, 40)])
def test_flat_then_boost_starts_the_filter_from_exact_zero(tmp_path_factory, monkeypatch, hidden, S, n):
    path, _ = _model(tmp_path_factory, hidden)
    x = W.signal(S, NBLK * n, seed=3000 + n)
    skip, full = _pair(monkeypatch, path, hidden, S, n, x, {0: [(None, {})], 3: [(None, dict(treble_boost_db=3.0))]})
    assert [_pads(skip, b) for b in range(NBLK)] == [[_k(n)] * S] * 3 + [[6] * S] * 3
    assert _z(skip[2][3][0])[5].all() and not _z(skip[2][2][0])[2:].any()


def _flat_design_that_is_no_identity():
    q = float(np.float32(0.707))
    for f in np.arange(400.0, 4000.0, 1.0, dtype=np.float32):
        c = ax.biquad_design(4, float(f) / 48000.0, q, 0.0)
        if c[0] != 1.0:
            assert c[1] == c[3] and c[2] == c[4] and abs(c[0] - 1.0) < 1e-15
            return float(f)
    return None


@pytest.mark.parametrize("hidden,S,n", [(32, 8, 64), (8, 5, 256), (32, 5, 40)])
def test_a_flat_design_that_is_no_identity_runs_all_stages(tmp_path_factory, monkeypatch, hidden, S, n):
    """about one 0 dB design in eight has a0 one ulp off 1: x a0 is not x, the stage is not transparent"""
    f = _flat_design_that_is_no_identity()
    assert f is not None
    path, _ = _model(tmp_path_factory, hidden)
    x = W.signal(S, NBLK * n, seed=4000 + n)
    skip, full = _pair(monkeypatch, path, hidden, S, n, x, {0: [(None, dict(mid_freq=f))]})
    for b in range(NBLK):
        assert _pads(skip, b) == [6] * S and _pads(full, b) == [6] * S


@pytest.mark.parametrize("hidden,S,n", [(32, 5, 64), (8, 8, 256), (8, 5, 40)])
def test_bandpass_mode_is_not_skipped(tmp_path_factory, monkeypatch, hidden, S, n):
    path, _ = _model(tmp_path_factory, hidden)
    x = W.signal(S, NBLK * n, seed=5000 + n)
    skip, full = _pair(monkeypatch, path, hidden, S, n, x, {0: [(None, dict(mid_type=1.0))]})
    for b in range(NBLK):
        assert _pads(skip, b) == [6] * S and _pads(full, b) == [6] * S


# ---------------------------------------------------------------- the chain alone, against the oracle to the bit

CHAIN_ONLY = dict(net_bypass=1.0, in_lpf_pc=0.0, dc_blocker=0.0)      # model out of circuit, LPF off, DC blocker off: EQ (post) and the two gains


def _took_the_skip(pool, S):
    """-> the streams' post cascade lengths, or None on the shipped library (which has no such word)"""
    if not hasattr(ax.lib(), "aidax_test_stream_state"):
        return None
    return [_pad(_record(pool, s)) for s in range(S)]


def _chain_run(path, S, n, x):
    pool = ax.Pool(S, n)
    pool.set_model(ax.Model(path))
    pool.set_controls(ax.default_controls(**CHAIN_ONLY))
    out, pads = np.empty_like(x), []
    for b in range(NBLK):
        out[:, b * n:(b + 1) * n] = pool.process(np.ascontiguousarray(x[:, b * n:(b + 1) * n]))
        pads.append(_took_the_skip(pool, S))
    name = pool.kernel_name
    pool.close()
    return name, out, pads


@pytest.mark.parametrize("hidden,S,n", [(32, 8, 64), (8, 5, 256), (32, 5, 48), (8, 8, 40)])
def test_sign_of_zero_and_denormals_against_the_oracle(tmp_path_factory, hidden, S, n):
    path, spec = _model(tmp_path_factory, hidden)
    x = W.signal(S, NBLK * n, seed=6000 + n)
    rs = np.random.RandomState(n)
    kind = rs.randint(0, 6, size=x.shape)
    x[kind == 0] = -0.0
    x[kind == 1] = 0.0
    x[kind == 2] = np.float32(1e-40)                            # denormals, both signs
    x[kind == 3] = np.float32(-3e-42)
    name, got, pads = _chain_run(path, S, n, x)
    assert name == _form(hidden, n)
    if pads[0] is not None:
        assert pads == [[_k(n)] * S] * NBLK
    want = O.run_streams(spec, O.default_controls(**CHAIN_ONLY), x, n)
    zeros = want == 0
    print(f"zeros {int(zeros.sum())}, of them negative: oracle {int(np.signbit(want[zeros]).sum())} gpu {int(np.signbit(got[got == 0]).sum())}; "
          f"max |diff| {float(np.abs(got - want).max()):.3e}")
    assert np.array_equal(got, want)
    assert np.array_equal(np.signbit(got), np.signbit(want))
    assert got.tobytes() == want.tobytes()


@pytest.mark.parametrize("hidden,S,n", [(32, 8, 64), (8, 5, 256), (32, 5, 40)])
def test_a_sample_that_is_not_finite_poisons_the_skipped_stages(tmp_path_factory, hidden, S, n):
    """+Inf at frame 37 of block 1 on the first and the last stream: that sample passes, everything behind it is NaN — in block 1 and,
    the state being NaN, in blocks 2 and 3 — and the other streams hear nothing of it"""
    path, spec = _model(tmp_path_factory, hidden)
    x = W.signal(S, NBLK * n, seed=7000 + n)
    bad = (0, S - 1)
    for s in bad:
        x[s, n + 37] = np.inf
    name, got, pads = _chain_run(path, S, n, x)
    assert name == _form(hidden, n)
    want = O.run_streams(spec, O.default_controls(**CHAIN_ONLY), x, n)
    for b in (1, 2, 3):
        assert np.array_equal(got[:, b * n:(b + 1) * n], want[:, b * n:(b + 1) * n], equal_nan=True), b
    assert np.array_equal(got, want, equal_nan=True)
    for s in range(S):
        if s in bad:
            assert np.isfinite(got[s, :n + 37]).all() and got[s, n + 37] == np.inf and np.isnan(got[s, n + 38:]).all()
        else:
            assert np.isfinite(got[s]).all()
    if pads[0] is not None:
        ran6 = [6 if s in bad else _k(n) for s in range(S)]
        assert pads[0] == [_k(n)] * S and pads[1] == [_k(n)] * S  # block 1 itself was skipped ...
        assert pads[2] == ran6 and pads[5] == ran6                # ... and left state that is not zero: every stage from block 2 on
