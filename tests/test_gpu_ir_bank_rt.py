"""Per-stream IRs in real time (GPU, -m gpu): aidax_pool_assign_ir and the commit of a prepared bank slot, called on the audio thread,
allocate, free and wait for nothing, and neither do the passes that follow them (include/aidax.h, "Threads"). Counted by the test build's
per-thread table of the pool's own HIP runtime calls (aidax_test_hip_calls, aidax_hip_host.h: every call site of every entry point the pool
and its IR stage use, checked or not, and the IR stage's launchers). The shipped library has no such table: these tests run on the test build only."""
import ctypes as C
import importlib

import numpy as np
import pytest

from tests import conftest, modelgen

pytestmark = pytest.mark.gpu
ax = importlib.import_module("aidadsp-lv2_amd")

ALLOC = {"hipMalloc", "hipHostMalloc", "hipHostRegister", "hipEventCreateWithFlags", "hipStreamCreateWithFlags", "hipStreamCreateWithPriority"}
FREE = {"hipFree", "hipHostFree", "hipHostUnregister", "hipEventDestroy", "hipStreamDestroy"}
WAIT = {"hipStreamSynchronize", "hipEventSynchronize", "hipDeviceSynchronize", "hipMemcpy"}
STAGE = {"launch_ir_append", "launch_ir_conv"}


@pytest.fixture
def calls():
    """read(): the calls this thread made into the pool's HIP runtime entry points since the last read, {name: count}"""
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


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    p = str(tmp_path_factory.mktemp("ir_bank_rt") / "lstm16.json")
    modelgen.write_model(modelgen.make_model(kind="lstm", hidden=16, input_size=1, seed=5), p)
    return ax.Model(p)


def _ir(L, seed):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal(L) * np.exp(-np.arange(L) / max(L / 6.0, 1.0))).astype(np.float32)


def _quiet(c, what):
    """no allocation, no free, no wait among the counted calls"""
    bad = {k: v for k, v in c.items() if k in ALLOC | FREE | WAIT}
    assert not bad, (what, bad, c)


class _Device:
    """aidax_pool_process_device on a torch stream: the library issues the pass, the wait for it is the test's own"""

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


def test_assign_ir_makes_no_hip_call(model, calls):
    S = 70
    p = ax.Pool(S, 256)
    p.set_model(model)
    p.set_ir(_ir(33, 1))
    p.set_ir_slot(3, _ir(4097, 2))
    p.process(modelgen.signal(S, 256, seed=3))
    calls()
    p.assign_ir(5, 3)
    p.assign_ir(ax.ALL_STREAMS, 3)
    p.assign_ir(6, ax.IR_NONE)
    p.assign_ir(7, ax.IR_POOL)
    p.assign_ir(8, 63)                                     # an empty slot
    assert [p.stream_ir(s) for s in (4, 5, 6, 7, 8)] == [3, 3, ax.IR_NONE, ax.IR_POOL, 63]
    assert calls() == {}
    p.close()


@pytest.mark.parametrize("slot", [0, 40])
def test_commit_of_a_prepared_slot_allocates_frees_and_waits_for_nothing(model, calls, slot):
    S = 70
    p = ax.Pool(S, 256)
    p.set_model(model)
    p.set_ir_slot(slot, _ir(8192, 4))
    p.assign_ir(ax.ALL_STREAMS, slot)
    dev = _Device(S, 256, seed=5)
    dev.pass_(p)
    dev.wait()
    for taps in (_ir(1000, 6), None, _ir(17, 7)):           # a new IR into a slot in use, emptying it, loading it again
        sg = p.prepare_ir_slot(slot, taps)                  # (worker side)
        calls()
        p.commit_ir(sg)                                     # audio side
        c = calls()
        _quiet(c, "commit_ir")
        assert not STAGE & set(c), c
        assert c.get("hipEventRecord", 0) >= 1, c           # the fence the retired fragments wait for
        dev.pass_(p)                                        # the pass behind the commit: a new plan, uploaded without a wait
        c = calls()
        _quiet(c, "pass after commit_ir")
        assert c["launch_ir_append"] == 1 and c.get("launch_ir_conv", 0) == (0 if taps is None else 1), c
        dev.wait()
        p.staged_free(sg)                                   # (worker side: the retired fragments)
        calls()
    p.close()


def test_passes_after_assign_ir_allocate_free_and_wait_for_nothing(model, calls):
    """process_device and submit passes, each behind a change of the plan: one append and at most one convolution launch, the plan's
    upload, nothing that allocates, frees or waits (aidax_pool_process and aidax_pool_collect wait for their block by design)"""
    S = 200
    p = ax.Pool(S, 256)
    p.set_model(model)
    p.set_ir(_ir(33, 8))
    for k in range(4):
        p.set_ir_slot(k, _ir(1 + 2000 * k, 9 + k))
    rng = np.random.default_rng(10)
    dev = _Device(S, 256, seed=11)
    dev.pass_(p)
    dev.wait()
    x = modelgen.signal(S, 256, seed=12)
    for _ in range(3):                                       # the submit path's staging sets: its first call allocates them
        p.submit(x)
    for _ in range(3):
        p.collect(256)
    calls()
    plans = [rng.integers(-2, 4, size=S) for _ in range(6)] + [np.full(S, ax.IR_NONE), np.full(S, 2)]
    for i, plan in enumerate(plans):
        for s, k in enumerate(plan):
            p.assign_ir(s, int(k))
        assert calls() == {}
        if i % 2 == 0:
            dev.pass_(p)
            c = calls()
            dev.wait()
        else:
            p.submit(x)
            c = calls()
            p.collect(256)
            calls()
        _quiet(c, f"pass {i}")
        assert c["launch_ir_append"] == 1, c
        assert c.get("launch_ir_conv", 0) == (0 if (plan == ax.IR_NONE).all() else 1), c
        assert c.get("hipMemcpyAsync", 0) >= 1, c           # the plan's upload
    p.close()


def test_a_pool_that_only_assigns_launches_nothing_for_the_stage(model, calls):
    S = 40
    pools = []
    for assign in (False, True):
        p = ax.Pool(S, 256)
        p.set_model(model)
        p.set_controls(ax.default_controls(pregain_db=3.0))
        if assign:
            p.assign_ir(ax.ALL_STREAMS, 5)
            p.assign_ir(0, ax.IR_NONE)
            p.assign_ir(1, ax.IR_POOL)
        pools.append(p)
    outs = []
    for p in pools:
        d = _Device(S, 256, seed=13)
        calls()
        got = []
        for _ in range(4):
            d.pass_(p)
            c = calls()
            _quiet(c, "pass")
            assert not STAGE & set(c), c
            got.append(d.wait())
        outs.append(np.concatenate(got, axis=1))
    assert [pools[1].stream_ir(s) for s in range(3)] == [ax.IR_NONE, ax.IR_POOL, 5]
    assert np.abs(outs[0]).max() > 0.01
    assert np.array_equal(outs[1], outs[0])                  # the assignments alone change nothing
    for p in pools:
        p.close()
