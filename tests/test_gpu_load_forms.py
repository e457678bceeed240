"""What choose_form (csrc/aidax_pool_model.cpp, on the pure rules of csrc/aidax_load_form.h) decides for a model in a pool on the machine
(run with -m gpu on an MI355X): the kind of slot, every field of its SlotForm, the state stride and whether the slot got a hand-over ring,
next to the kernel name at the pool's block length — against the commit before the decision became functions of facts.

Loads only (START_RESET: no warm-up, no pass is launched). Each case creates a pool, loads one model, reads kernel_name and the one text
line of aidax_test_slot_form (test build only: it formats fields of the playing ModelSlot), and closes the pool before the next.
tests/golden/load_forms_parent.json was recorded ONCE on an MI355X (256 CUs) from the test-hooks library of the parent commit (65d3f83) with
that same read-only entry patched into its aidax_pool.cpp, in a scratch worktree:
    AIDAX_LIB=<that build's lib/hooks/libaidax_hip.so> python -m tests.test_gpu_load_forms --record <out.json>
(the __main__ block at the end of this file; the same _load as the test). A pool the machine refuses keeps its case: the error text is
the expectation. On the shipped library (no test entry, no hooks) the cases without a hook compare the kernel name.

  one-layer models  LSTM-16 / 32 / 40 / 64 / 80, GRU-32 / 40 / 64 / 80 at 1, 64, 1024, 4096, 8192 streams; every AIDAX_KERNEL word on LSTM-32 at 8
  stacks            LSTM-16 x 2 conditioned, LSTM-64 x 2, x 3, LSTM-80 x 2, LSTM-96 x 2, GRU-96 x 2 at 16, 2048, 4096, 8192 streams; at 2048
                    AIDAX_MFMA_LP=0 / 1, AIDAX_LP_SPLIT=0 / 9, AIDAX_LP_FUSED=0, AIDAX_KERNEL=valu; AIDAX_LP_ROUND_GROUPS=8 at 272 streams
  conv stacks       shapes 1, 6, 8 and 10 of tools/form_table.py at 16 and 4096 streams, blocks of 32, 64, 256 and 512 frames; at blocks of 64
                    AIDAX_CONV_MS=0, AIDAX_CONV_ST=0, AIDAX_CONV_FUSED=0 / 1, AIDAX_KERNEL=valu
Blocks of 64 frames unless stated.
"""
import ctypes as C
import importlib
import json
import os
import sys

import pytest

pytestmark = pytest.mark.gpu

ax = importlib.import_module("aidadsp-lv2_amd")
W = ax.workloads

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "load_forms_parent.json")
PARENT = "65d3f83"

MODELS = {f"{kind}{h}": dict(kind=kind, hidden=h, input_size=1, seed=100 + h) for kind, hs in (("lstm", (16, 32, 40, 64, 80)), ("gru", (32, 40, 64, 80))) for h in hs}
ONE_LAYER = list(MODELS)
STACKS = {
    "lstm16x2c": dict(kind="lstm", hidden=16, input_size=2, seed=1620, n_rnn=2), "lstm64x2": dict(kind="lstm", hidden=64, input_size=1, seed=642, n_rnn=2),
    "lstm64x3": dict(kind="lstm", hidden=64, input_size=1, seed=643, n_rnn=3), "lstm80x2": dict(kind="lstm", hidden=80, input_size=1, seed=802, n_rnn=2),
    "lstm96x2": dict(kind="lstm", hidden=96, input_size=1, seed=96, n_rnn=2), "gru96x2": dict(kind="gru", hidden=96, input_size=1, seed=962, n_rnn=2),
}
CONVS = {      # tools/form_table.py, shapes 1, 6, 8, 10
    "conv1_8xk3": dict(kind="conv", input_size=1, seed=1, hidden=16, conv_layers=8), "conv6_5xk3": dict(kind="conv", input_size=1, seed=1, hidden=16, conv_layers=5),
    "conv8_8xk4": dict(kind="conv", input_size=1, seed=1, hidden=16, conv_layers=8, conv_k=4), "conv10_6xk3c12": dict(kind="conv", input_size=1, seed=1, hidden=12, conv_layers=6),
}
MODELS.update(STACKS)
MODELS.update(CONVS)


def _cases():
    """(model, streams, block length, hooks) of every case"""
    out = [(m, n, 64, {}) for m in ONE_LAYER for n in (1, 64, 1024, 4096, 8192)]
    out += [("lstm32", 8, 64, {"AIDAX_KERNEL": w}) for w in ("wave", "pipe", "split", "valu", "mfma", "quad", "q4")]
    out += [(m, n, 64, {}) for m in STACKS for n in (16, 2048, 4096, 8192)]
    for m in STACKS:
        out += [(m, 2048, 64, h) for h in ({"AIDAX_MFMA_LP": "0"}, {"AIDAX_MFMA_LP": "1"}, {"AIDAX_LP_SPLIT": "0"}, {"AIDAX_LP_SPLIT": "9"}, {"AIDAX_LP_FUSED": "0"},
                                            {"AIDAX_KERNEL": "valu"})]
        out.append((m, 272, 64, {"AIDAX_LP_ROUND_GROUPS": "8"}))
    out += [(m, n, f, {}) for m in CONVS for n in (16, 4096) for f in (32, 64, 256, 512)]
    for m in CONVS:
        out += [(m, n, 64, h) for n in (16, 4096) for h in ({"AIDAX_CONV_MS": "0"}, {"AIDAX_CONV_ST": "0"}, {"AIDAX_CONV_FUSED": "0"}, {"AIDAX_CONV_FUSED": "1"},
                                                            {"AIDAX_KERNEL": "valu"})]
    return out


def _id(case):
    m, n, f, hooks = case
    return f"{m} n{n} f{f}" + "".join(f" {k[6:]}={v}" for k, v in sorted(hooks.items()))


CASES = _cases()
HOOKS = sorted({k for c in CASES for k in c[3]})


def _load(path, n_streams, max_frames):
    """one pool, one load -> {"kernel", "slot"} (slot None on a library without the test entry), or {"error"} where the machine refuses"""
    pool = None
    try:
        pool = ax.Pool(n_streams, max_frames)
        pool.set_model(ax.Model(path), ax.START_RESET)
        got = {"kernel": pool.kernel_name, "slot": None}
        if hasattr(ax.lib(), "aidax_test_slot_form"):
            buf = C.create_string_buffer(256)
            rc = ax.lib().aidax_test_slot_form(pool.h, buf, C.c_uint32(256))
            assert 0 < rc < 256, rc
            got["slot"] = buf.value.decode()
        return got
    except ax.AidaxError as e:
        return {"error": str(e)}
    finally:
        if pool is not None:
            pool.close()


@pytest.fixture(scope="module")
def parent():
    with open(FIXTURE) as f:
        fixture = json.load(f)
    assert fixture["parent"] == PARENT
    assert sorted(fixture["cases"]) == sorted(_id(c) for c in CASES)      # every case, and no other
    return fixture["cases"]


@pytest.fixture(scope="module")
def model_paths(tmp_path_factory):
    d = tmp_path_factory.mktemp("load_forms")
    return {name: W.write_model(W.make_model(**kw), os.path.join(str(d), f"{name}.json")) for name, kw in MODELS.items()}


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_the_load_decision_equals_the_parent_commits(monkeypatch, parent, model_paths, case):
    model, n_streams, max_frames, hooks = case
    for k in HOOKS:
        monkeypatch.delenv(k, raising=False)
    for k, v in hooks.items():
        monkeypatch.setenv(k, v)                                 # (test hooks: the shipped leg skips here)
    want = parent[_id(case)]
    got = _load(model_paths[model], n_streams, max_frames)
    print(f"{_id(case)}: {got}")
    if got.get("slot") is None and "error" not in got:           # the shipped library: the kernel's name is what it can tell
        assert got["kernel"] == want.get("kernel"), (got, want)
        return
    assert got == want


if __name__ == "__main__":
    # records a fixture from whatever library AIDAX_LIB names (see the module docstring); the path is required, and the committed fixture is
    # never written over: it is the parent commit's, recorded once
    if "--record" in sys.argv:
        import tempfile
        k = sys.argv.index("--record")
        if len(sys.argv) <= k + 1 or os.path.abspath(sys.argv[k + 1]) == FIXTURE:
            raise SystemExit("usage: python -m tests.test_gpu_load_forms --record <out.json>  (not the committed fixture)")
        assert hasattr(ax.lib(), "aidax_test_slot_form"), "record from a test-hooks library that has the entry"
        tmp = tempfile.mkdtemp()
        paths = {name: W.write_model(W.make_model(**kw), os.path.join(tmp, f"{name}.json")) for name, kw in MODELS.items()}
        cases = {}
        for case_ in CASES:
            for k_ in HOOKS:
                os.environ.pop(k_, None)
            os.environ.update(case_[3])
            cases[_id(case_)] = _load(paths[case_[0]], case_[1], case_[2])
            print(f"{_id(case_):44} {cases[_id(case_)]}", flush=True)
        with open(sys.argv[k + 1], "w") as f:
            json.dump({"parent": PARENT, "recorded_on": "MI355X, 256 CUs", "cases": cases}, f, indent=0, sort_keys=True)
        print(f"recorded {len(cases)} cases from {ax.lib_path()} -> {sys.argv[k + 1]} ({os.path.getsize(sys.argv[k + 1])} bytes)")
