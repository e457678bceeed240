"""The IR fade in real time (GPU, -m gpu): aidax_pool_set_ir_fade, aidax_pool_assign_ir and a commit under a fade length, the fade pass and
the pass after it, called on the audio thread, allocate, free and wait for nothing; a pass without a pending fade issues exactly one
launch_ir_append and one launch_ir_conv and no fade launch, the fade pass issues the extra ones (a second launch_ir_conv for the old IRs
and launch_ir_fade), and the pass after it none of them. Counted by the test build's per-thread table of the pool's own HIP calls, as in
tests/test_gpu_ir_bank_rt.py: test build only."""
import importlib

import pytest

from tests import modelgen
from tests.test_gpu_ir_bank_rt import ALLOC, FREE, WAIT, _Device, _ir, _quiet, calls  # noqa: F401  (calls: a fixture)

pytestmark = pytest.mark.gpu
ax = importlib.import_module("aidadsp-lv2_amd")


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    p = str(tmp_path_factory.mktemp("ir_fade_rt") / "lstm16.json")
    modelgen.write_model(modelgen.make_model(kind="lstm", hidden=16, input_size=1, seed=5), p)
    return ax.Model(p)


def _stage(c):
    return {k: c.get(k, 0) for k in ("launch_ir_append", "launch_ir_conv", "launch_ir_fade")}


PLAIN = {"launch_ir_append": 1, "launch_ir_conv": 1, "launch_ir_fade": 0}


def _pool(model, S):
    p = ax.Pool(S, 256)
    p.set_model(model)
    return p


def test_set_ir_fade_makes_no_hip_call(model, calls):
    p = _pool(model, 8)
    calls()
    p.set_ir_fade(128)
    assert p.ir_fade() == 128
    p.set_ir_fade(0)
    assert calls() == {}
    p.close()


@pytest.mark.parametrize("S", [1, 70])
def test_a_commit_under_a_fade_length_the_fade_pass_and_the_pass_after_it(model, calls, S):
    p = _pool(model, S)
    calls()
    p.set_ir_fade(200)
    assert calls() == {}
    p.set_ir(_ir(8192, 1))
    p.set_ir_slot(3, _ir(33, 2))
    dev = _Device(S, 256, seed=3)
    dev.pass_(p)                                            # (the pool's first pass: nothing to fade from)
    dev.wait()
    calls()
    dev.pass_(p)
    c = calls()
    _quiet(c, "steady pass")
    assert _stage(c) == PLAIN, c                            # no fade pending: exactly the launches of a pool without a fade length
    dev.wait()
    had_ir = True
    for taps in (_ir(1000, 4), None, _ir(17, 5), _ir(4097, 6)):
        sg = p.prepare_ir(taps)                             # (worker side)
        calls()
        p.commit_ir(sg)                                     # audio side: parks the retired fragments, hands back the ones parked before
        c = calls()
        _quiet(c, "commit_ir")
        assert _stage(c) == {"launch_ir_append": 0, "launch_ir_conv": 0, "launch_ir_fade": 0}, c
        assert c.get("hipEventRecord", 0) >= 1, c           # the fence
        p.staged_free(sg)                                   # (worker side, BEFORE the fade pass is issued)
        calls()
        dev.pass_(p)                                        # the fade pass: the new side (none after a removal), the old side (none
        c = calls()                                         # where there was no IR), the mix
        _quiet(c, "fade pass")
        assert _stage(c) == {"launch_ir_append": 1, "launch_ir_conv": (taps is not None) + had_ir, "launch_ir_fade": 1}, c
        assert c.get("hipMemcpyAsync", 0) >= 1, c           # the plan's upload, both sections in one
        dev.wait()
        calls()
        for _ in range(2):                                  # the passes after it: none of the extra launches
            dev.pass_(p)
            c = calls()
            _quiet(c, "pass after the fade pass")
            assert _stage(c) == {"launch_ir_append": 1, "launch_ir_conv": int(taps is not None), "launch_ir_fade": 0}, c
            dev.wait()
            calls()
        had_ir = taps is not None
    p.close()


def test_assign_ir_under_a_fade_length(model, calls):
    S = 70
    p = _pool(model, S)
    p.set_ir_fade(64)
    p.set_ir(_ir(4097, 7))
    p.set_ir_slot(0, _ir(33, 8))
    dev = _Device(S, 256, seed=9)
    for _ in range(2):
        dev.pass_(p)
        dev.wait()
    calls()
    for s, k, conv in ((5, 0, 2), (5, ax.IR_NONE, 2), (5, ax.IR_POOL, 1), (ax.ALL_STREAMS, ax.IR_NONE, 1), (6, 40, 0), (ax.ALL_STREAMS, 0, 1)):
        p.assign_ir(s, k)
        assert calls() == {}
        dev.pass_(p)
        c = calls()
        _quiet(c, f"fade pass after assign_ir({s}, {k})")
        fade = 0 if (s, k) == (6, 40) else 1                # from none to an empty slot: no change
        assert _stage(c) == {"launch_ir_append": 1, "launch_ir_conv": conv, "launch_ir_fade": fade}, (s, k, c)
        dev.wait()
        calls()
        dev.pass_(p)
        c = calls()
        _quiet(c, "pass after the fade pass")
        assert _stage(c)["launch_ir_fade"] == 0 and _stage(c)["launch_ir_conv"] <= 1, c
        dev.wait()
        calls()
    p.close()
