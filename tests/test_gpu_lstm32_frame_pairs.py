"""k_lstm_pipe4<32>'s paired frame against the frame every other LSTM-32 kernel keeps, bit for bit (run with -m gpu on an MI355X).

The unconditioned k_lstm_pipe4<32> issues what its frame does to both gate rows of a lane as packed instructions (the input pair, the
own-unit pair, go * tanh(c) twice from one v_pk_mul_f32 for the swap, the last add of the product inside the asm statement; LstmCell's
PAIRS, aidax_kernels.hip). k_lstm_pipe<32> keeps the old frame, and on the test build AIDAX_PIPE4=0 sends the same pool through it: new
frame against old frame, same operations on the same operands in the same order, so the same bits — outputs AND the final h, c of every
stream, compared as uint32 (NaN payloads and the sign of every zero included).

cfg2's model (seed 32) and an LSTM-32 with in_skip = 1 and gains that are not 1; pools of 4, 5 and 9 streams (one whole workgroup; ragged
last workgroups); blocks of 16, 64 and 256 frames in sequence on ONE state, among them
  * a block scaled by 32 (tanh_rat clamps),
  * four all-zero 256-frame blocks behind it (the muted tail: whatever of h and of the filters' states decays, decays through the denormals),
  * a block of zeros of both signs and of denormal samples (the packed instructions' operands),
  * one stream with a NaN sample, one with +Inf then -Inf (the input low-pass turns it into NaN: b2 * inf - a2 * inf): their cell state c
    is NaN afterwards in both forms — c' = f * c + i * g never loses a NaN — while h is not: tanh_rat's clamp answers a NaN with -1, the
    output gate comes out 0 and h = 0 * -1, a signed zero, the same in both forms. The other streams' state stays finite.

One bit is left out, and it is not the frame's: the SIGN of an output sample that is NaN in both forms. The in_skip model adds the (NaN)
input to the network's output in the two kernels' own output paths — the helper wave's Dense lanes there, the third wave here — and the two
write NaNs of opposite sign for some frames (0x7fc00000 against 0xffc00000; 128 samples of each poisoned stream in this plan). The commit
before the paired frame does exactly the same, sample for sample (measured with its test build on the same inputs), and h and c, which
are all the frame hands on, are equal to the bit, NaN payloads included. Everything else of a NaN sample — that it is one, where, and its
payload — is compared, and every sample that is no NaN bit for bit.
"""
import importlib
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ax = importlib.import_module("aidadsp-lv2_amd")
W = ax.workloads

POOLS = (4, 5, 9)
MODELS = {
    "cfg2": dict(kind="lstm", hidden=32, input_size=1, seed=32),
    "skip": dict(kind="lstm", hidden=32, input_size=1, seed=33, in_skip=1, in_gain=-3.0, out_gain=4.5),
}
# (frames, what the block holds)
PLAN = ((16, "plain"), (64, "plain"), (256, "plain"), (256, "loud"), (256, "zero"), (256, "zero"), (256, "zero"), (256, "zero"),
        (64, "tiny"), (16, "plain"), (256, "plain"), (256, "nonfinite"), (64, "plain"), (16, "plain"))
NAN_STREAM, INF_STREAM = 1, 2


def _inputs(S):
    total = sum(n for n, _ in PLAN)
    x = W.signal(S, total, seed=0x9A12 + S)
    o = 0
    for n, kind in PLAN:
        b = x[:, o:o + n]
        if kind == "loud":
            b *= np.float32(32.0)
        elif kind == "zero":
            b[:] = 0.0
        elif kind == "tiny":
            pat = np.array([0.0, -0.0, 1e-40, -1e-40, 1.4e-45, -1.4e-45, 0.0, 1.1754942e-38], np.float32)      # zeros of both signs, denormals, the largest denormal
            b[:] = np.tile(pat, n // pat.size)[None, :]
            b[0::2] = -b[0::2]                               # (every other stream mirrored)
        elif kind == "nonfinite":
            b[NAN_STREAM, 5] = np.nan
            b[INF_STREAM, 7] = np.inf
            b[INF_STREAM, 8] = -np.inf
        o += n
    return x


def _run(path, S):
    """one pool over PLAN on one state -> (outputs, h [S][32], c [S][32], kernel name)"""
    pool = ax.Pool(S, 256)
    pool.set_model(ax.Model(path))
    x = _inputs(S)
    out, o = np.empty_like(x), 0
    for n, _ in PLAN:
        out[:, o:o + n] = pool.process(np.ascontiguousarray(x[:, o:o + n]))
        o += n
    hs, cs = zip(*(pool.read_state(s, 0, 32) for s in range(S)))
    name = pool.kernel_name
    pool.close()
    return out, np.stack(hs), np.stack(cs), name


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _out_bits(a):
    """an output block's words, a NaN sample's sign bit cleared (the module docstring says whose it is)"""
    a = np.ascontiguousarray(a, np.float32)
    return np.where(np.isnan(a), a.view(np.uint32) & np.uint32(0x7FFFFFFF), a.view(np.uint32))


@pytest.mark.parametrize("S", POOLS)
@pytest.mark.parametrize("name", sorted(MODELS))
def test_paired_frame_equals_the_old_frame(tmp_path, monkeypatch, name, S):
    path = W.write_model(W.make_model(**MODELS[name]), os.path.join(str(tmp_path), f"{name}.json"))
    monkeypatch.setenv("AIDAX_PIPE4", "0")                      # (test build; read per call)
    want, want_h, want_c, old_kernel = _run(path, S)
    monkeypatch.delenv("AIDAX_PIPE4")
    got, got_h, got_c, kernel = _run(path, S)
    assert old_kernel == "k_lstm_pipe<32>" and kernel == "k_lstm_pipe4<32>"
    for what, g, w in (("output", _out_bits(got), _out_bits(want)), ("h", _bits(got_h), _bits(want_h)), ("c", _bits(got_c), _bits(want_c))):
        d = g != w
        print(f"{name} S={S} {what}: {int(d.sum())} of {d.size} words differ" + (f", first at {tuple(np.argwhere(d)[0])}" if d.any() else ""))
    print(f"{name} S={S} output: {int((_bits(got) != _bits(want)).sum())} NaN samples of opposite sign")
    assert np.array_equal(_out_bits(got), _out_bits(want))
    clean_rows = [s for s in range(S) if s not in (NAN_STREAM, INF_STREAM)]
    assert np.array_equal(_bits(got[clean_rows]), _bits(want[clean_rows]))      # (no NaN there: nothing is masked)
    assert np.array_equal(_bits(got_h), _bits(want_h))
    assert np.array_equal(_bits(got_c), _bits(want_c))
    # the inputs did what they are there for: the poisoned streams' cell state is NaN in both forms, every other stream came through finite
    clean = [s for s in range(S) if s not in (NAN_STREAM, INF_STREAM)]
    for h, c in ((got_h, got_c), (want_h, want_c)):
        for s in (NAN_STREAM, INF_STREAM):
            assert np.isnan(c[s]).all(), (s, h[s], c[s])
        assert np.isfinite(h[clean]).all() and np.isfinite(c[clean]).all()
    assert np.isfinite(got[clean]).all()
    o = np.cumsum([0] + [n for n, _ in PLAN])
    k = [kind for _, kind in PLAN].index("nonfinite")
    assert np.isfinite(got[:, :o[k]]).all()                     # (nothing is NaN before the NaN)
