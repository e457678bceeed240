"""The LSTM-32 frame keeps its bits (run with -m gpu on an MI355X).

The recurrent wave of k_lstm_pipe4<32> (and of k_lstm_pipe<32>, k_lstm_pipe_bank<32>, k_lstm<32>: the same cell) issues its frame with fewer
instructions — the LDS half of the product as one asm statement whose chains start from the inline constant 0, tanh_rat's packed Horner steps
with {u, u} as first source. It may not change a bit:

  * test_outputs_equal_the_parent_commits: every output sample against tests/golden/lstm32_frame_parent.npz, which was recorded ONCE on
    an MI355X with the SHIPPED library of the commit before this change (6f8bb39):
        AIDAX_LIB=<that commit's aidadsp-lv2_amd/lib/libaidax_hip.so> python -m tests.test_gpu_lstm32_frame --record <out.npz>
    (the __main__ block at the end of this file; the same _run as the test). cfg2's model (LSTM-32, seed 32) and an LSTM-32 with in_skip = 1,
    in / out gains that are not 1, a boosted post EQ on stream 1 and the EQ bypassed on stream 2; pools of 4, 5 and 9 streams (one whole
    workgroup; ragged last workgroups of 1 stream); blocks of 16, 256, 64, 24 and 128 frames in sequence on one state — 24 is no whole tile,
    so k_lstm_pipe<32> takes it —, the 256-frame block scaled by 8 (tanh_rat's clamp), the 64-frame block all zeros (the sign of zero).
  * test_param_targets_follow_the_three_wave_form: an unconditioned pool whose PARAM1 / PARAM2 controls move between blocks (the first-run
    snap, a move, no move, a move below FLT_EPSILON, a stream out of circuit and a disabled one): p_mem, p_step, p_tgt and `pending` of
    every stream after every block, k_lstm_pipe4<32> against AIDAX_PIPE4=0 (test build: k_lstm_pipe<32>). Both epilogues call the same
    param_targets() today, so this runs nothing the frame's change touched; it is the pin for any later change to the helper wave's tail
    (one that read those words in the prologue was measured and not kept: profiles/lstm32_frame_slots.txt).
"""
import ctypes as C
import importlib
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ax = importlib.import_module("aidadsp-lv2_amd")
W = ax.workloads

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lstm32_frame_parent.npz")
BLOCKS = (16, 256, 64, 24, 128)
POOLS = (4, 5, 9)
MODELS = {
    "cfg2": dict(kind="lstm", hidden=32, input_size=1, seed=32),
    "skip": dict(kind="lstm", hidden=32, input_size=1, seed=33, in_skip=1, in_gain=-3.0, out_gain=4.5),
}
REC = 160                      # sizeof(StreamState): [128, 152) p_mem[2] p_step[2] p_tgt[2], [152] pending (pinned by the static_asserts in aidax_layout.h)


def _model_path(tmp, name):
    return W.write_model(W.make_model(**MODELS[name]), os.path.join(str(tmp), f"{name}.json"))


def _inputs(S):
    x = W.signal(S, sum(BLOCKS), seed=0x32F + S)
    o = np.cumsum((0,) + BLOCKS)
    x[:, o[1]:o[2]] *= np.float32(8.0)
    x[:, o[2]:o[3]] = 0.0
    return x


def _run(path, name, S):
    """one pool over BLOCKS on one state -> (outputs [S][sum(BLOCKS)], the pool's kernel name: what a block of its full length runs)"""
    pool = ax.Pool(S, 256)
    pool.set_model(ax.Model(path))
    if name == "skip":
        pool.set_controls(ax.default_controls(mid_boost_db=4.0), stream=1)
        pool.set_controls(ax.default_controls(eq_bypass=1.0), stream=2)
    x = _inputs(S)
    out, o = np.empty_like(x), 0
    for n in BLOCKS:
        out[:, o:o + n] = pool.process(np.ascontiguousarray(x[:, o:o + n]))
        o += n
    name = pool.kernel_name
    pool.close()
    return out, name


@pytest.fixture(scope="module")
def parent():
    with np.load(FIXTURE) as z:
        return {k: z[k] for k in z.files}


@pytest.mark.parametrize("S", POOLS)
@pytest.mark.parametrize("name", sorted(MODELS))
def test_outputs_equal_the_parent_commits(tmp_path, parent, name, S):
    got, kernel = _run(_model_path(tmp_path, name), name, S)
    assert kernel == "k_lstm_pipe4<32>"                         # (whole tiles; the 24-frame block is k_lstm_pipe<32>'s)
    want = parent[f"{name}_{S}"]
    assert np.isfinite(got).all()
    diff = got != want
    print(f"{name} S={S}: {int(diff.sum())} of {got.size} samples differ, max |diff| {float(np.abs(got - want).max()):.3e}")
    assert np.array_equal(got, want)
    assert got.tobytes() == want.tobytes()                      # (the sign of every zero as well)


def _record(pool, s):
    buf = (C.c_uint8 * REC)()
    rc = ax.lib().aidax_test_stream_state(pool.h, C.c_uint32(s), buf, C.c_uint32(REC))
    assert rc == REC, rc
    return bytes(buf)


# in front of block b: (stream or None for all, the controls that change — a stream keeps what it was given before)
_ULP = float(np.nextafter(np.float32(0.5), np.float32(1.0)))     # 0.5 + 6e-8: closer to 0.5 than FLT_EPSILON — no move
PARAM_SCHEDULE = {
    0: [(0, dict(param1=0.3, param2=0.7)), (2, dict(net_bypass=1.0, param1=0.9)), (3, dict(enabled=0.0, param2=0.4))],      # the first-run snap
    1: [(None, dict(param1=0.5))],
    2: [],
    3: [(1, dict(param1=0.5, param2=0.25)), (0, dict(param1=_ULP))],
    4: [(0, dict(param1=0.0, param2=1.0)), (3, dict(enabled=1.0))],                                                          # (stream 3 comes back: its snap)
}


def _param_run(path, S):
    pool = ax.Pool(S, 256)
    pool.set_model(ax.Model(path))
    x = _inputs(S)
    recs, o = [], 0
    held = [dict() for _ in range(S)]
    for b, n in enumerate(BLOCKS):
        for s_, kw in PARAM_SCHEDULE[b]:
            for s in (range(S) if s_ is None else [s_]):
                held[s].update(kw)
                pool.set_controls(ax.default_controls(**held[s]), stream=s)
        pool.process(np.ascontiguousarray(x[:, o:o + n]))
        recs.append([_record(pool, s) for s in range(S)])
        o += n
    name = pool.kernel_name
    pool.close()
    return recs, name


@pytest.mark.parametrize("S", POOLS)
def test_param_targets_follow_the_three_wave_form(tmp_path, monkeypatch, S):
    path = _model_path(tmp_path, "cfg2")
    monkeypatch.setenv("AIDAX_PIPE4", "0")                      # (test build; read per call)
    ref, ref_kernel = _param_run(path, S)
    monkeypatch.delenv("AIDAX_PIPE4")
    got, kernel = _param_run(path, S)
    assert ref_kernel == "k_lstm_pipe<32>" and kernel == "k_lstm_pipe4<32>"
    for b in range(len(BLOCKS)):
        for s in range(S):
            g, r = got[b][s], ref[b][s]
            for field, lo, hi in (("p_mem", 128, 136), ("p_step", 136, 144), ("p_tgt", 144, 152), ("pending", 152, 156)):
                assert g[lo:hi] == r[lo:hi], (field, b, s, np.frombuffer(g[lo:hi], np.uint32), np.frombuffer(r[lo:hi], np.uint32))
    # what the schedule is there for did happen: the snap (mem = target, the flag gone), a step from a moved target, none from the ulp
    f = lambda rec, lo: np.frombuffer(rec[lo:lo + 8], np.float32)
    assert f(got[0][0], 128).tolist() == f(got[0][0], 144).tolist() == [np.float32(0.3), np.float32(0.7)]
    assert np.frombuffer(got[0][0][152:156], np.uint32)[0] & 2 == 0
    assert f(got[1][0], 136)[0] != 0 and f(got[1][0], 144)[0] == np.float32(0.5)
    assert f(got[3][0], 144)[0] == np.float32(0.5)              # the ulp did not move the target
    assert f(got[3][1], 144)[1] == np.float32(0.25)


if __name__ == "__main__":
    # records a fixture from whatever library AIDAX_LIB names (see the module docstring): python -m tests.test_gpu_lstm32_frame --record <out.npz>
    # (the path is required, and the committed fixture is never written over: it is the parent commit's, recorded once)
    if "--record" in sys.argv:
        import tempfile
        k = sys.argv.index("--record")
        if len(sys.argv) <= k + 1 or os.path.abspath(sys.argv[k + 1]) == FIXTURE:
            raise SystemExit("usage: python -m tests.test_gpu_lstm32_frame --record <out.npz>  (not the committed fixture)")
        out = sys.argv[k + 1]
        tmp = tempfile.mkdtemp()
        arrays = {}
        for name_ in sorted(MODELS):
            for S_ in POOLS:
                arrays[f"{name_}_{S_}"], _kernel = _run(_model_path(tmp, name_), name_, S_)
        np.savez_compressed(out, **arrays)
        print(f"recorded {len(arrays)} arrays from {ax.lib_path()} -> {out} ({os.path.getsize(out)} bytes)")
