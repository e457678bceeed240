"""The noise gate in real time (GPU, -m gpu): once the set-up side has enabled one, aidax_pool_set_gate is a host record (plus one
asynchronous clear for streams that go from off to on), a gated pass allocates, frees and waits for nothing and issues one launch of
k_gate more (and the upload of changed records), and while no stream's gate is on a pass makes exactly the calls of a pool that never
had a gate. Counted by the test build's per-thread table of the pool's own HIP runtime calls (aidax_test_hip_calls, aidax_hip_host.h);
the shipped library has no such table: these tests run on the test build only."""
import ctypes as C
import importlib

import pytest

from tests import conftest, gatehelp as gh, modelgen

pytestmark = pytest.mark.gpu
ax = importlib.import_module("aidadsp-lv2_amd")

ALLOC = {"hipMalloc", "hipHostMalloc", "hipHostRegister", "hipEventCreateWithFlags", "hipStreamCreateWithFlags", "hipStreamCreateWithPriority"}
FREE = {"hipFree", "hipHostFree", "hipHostUnregister", "hipEventDestroy", "hipStreamDestroy"}
WAIT = {"hipStreamSynchronize", "hipEventSynchronize", "hipDeviceSynchronize", "hipMemcpy"}


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
    p = str(tmp_path_factory.mktemp("gate_rt") / "lstm16.json")
    modelgen.write_model(modelgen.make_model(kind="lstm", hidden=16, input_size=1, seed=5), p)
    return ax.Model(p)


class _Device:
    """aidax_pool_process_device on a torch stream: the library issues the pass, the wait for it is the test's own"""

    def __init__(self, S, n, seed):
        import torch
        self.torch = torch
        self.s = torch.cuda.Stream()
        self.x = torch.from_numpy(gh.signal(S, n, seed=seed)).cuda()
        self.y = torch.empty_like(self.x)
        torch.cuda.synchronize()

    def pass_(self, pool, n=None):
        with self.torch.cuda.stream(self.s):
            pool.process_device(self.x.data_ptr(), self.y.data_ptr(), self.x.shape[1] if n is None else n, self.s.cuda_stream)

    def wait(self):
        self.s.synchronize()


def test_the_first_enabling_call_allocates_and_later_ones_do_not(model, calls):
    S = 70
    p = ax.Pool(S, 256)
    p.set_model(model)
    calls()
    p.set_gate(None)                                            # off before any on: nothing at all
    assert calls() == {}
    pr = gh.params(**gh.SETS[0])
    p.set_gate(pr, 3)                                           # set-up side: records, states, side block; staging and four snapshots
    c = calls()
    assert c.get("hipMalloc") == 3 and c.get("hipHostMalloc") == 5, c
    p.set_gate(gh.params(**gh.SETS[1]), 3)                      # audio side, a change while on: a host record
    assert calls() == {}
    p.set_gate(None, 3)
    assert calls() == {}
    p.set_gate(pr, 70 - 1)                                      # off -> on: the clear of one state, asynchronously, on the pool's own stream
    c = calls()
    assert c.pop("hipMemsetAsync") == 1 and not {k: v for k, v in c.items() if k in ALLOC | FREE | WAIT}, c
    p.set_gate(pr)                                              # every stream: 0 .. 68 were off, one run and one clear; 69 is on and keeps its state
    c = calls()
    assert c.pop("hipMemsetAsync") == 1 and not {k: v for k, v in c.items() if k in ALLOC | FREE | WAIT}, c
    p.set_gate(None, 10)
    p.set_gate(None, 20)
    calls()
    p.set_gate(pr)                                              # two streams, not neighbours: two clears
    c = calls()
    assert c.pop("hipMemsetAsync") == 2 and not {k: v for k, v in c.items() if k in ALLOC | FREE | WAIT}, c
    p.close()


def test_gated_passes_allocate_free_and_wait_for_nothing(model, calls):
    S = 70
    plain, p = ax.Pool(S, 256), ax.Pool(S, 256)
    for q in (plain, p):
        q.set_model(model)
    pr = gh.params(**gh.SETS[0])
    p.set_gate(pr)
    dev = _Device(S, 256, seed=5)
    for q in (plain, p):
        dev.pass_(q)
    dev.wait()
    calls()
    # (gate on?, frames, k_gate launches, record uploads): the records go up once after a change, ahead of the next gated pass of frames
    now = True
    for on, n, launches, uploads in ((True, 256, 1, 0), (True, 0, 0, 0), (False, 256, 0, 0), (True, 100, 1, 1), (False, 0, 0, 0), (False, 64, 0, 0),
                                     (True, 256, 1, 1), (True, 256, 1, 0)):
        if on != now:
            p.set_gate(pr if on else None)
        turned_on, now = on and not now, on
        calls()
        dev.pass_(plain, n)
        base = calls()
        dev.pass_(p, n)
        c = calls()
        bad = {k: v for k, v in c.items() if k in ALLOC | FREE | WAIT}
        assert not bad, (on, n, bad, c)
        assert c.get("launch_gate", 0) == launches, (on, n, c)
        extra = {k: c.get(k, 0) - base.get(k, 0) for k in set(c) | set(base) if c.get(k, 0) != base.get(k, 0)}
        want = {"launch_gate": launches} if launches else {}
        if uploads:
            want.update(hipMemcpyAsync=1, hipEventRecord=1)
        if turned_on:
            # the clear of the states went to the pool's own stream: the pass on the caller's stream is ordered behind it by an event edge
            want["hipEventRecord"] = want.get("hipEventRecord", 0) + 1
            want["hipStreamWaitEvent"] = 1
        # what a gated pass adds to a plain pool's calls is the launch and, after a change, the upload; with every gate off, nothing
        assert extra == want, (on, n, extra, base, c)
        dev.wait()
    p.close()
    plain.close()


def test_a_gated_one_stream_pass_keeps_its_kernel_written_completion_word(model, calls):
    """the blocking path of a one-stream pool: the gate is ahead of the model's launch, so that launch still carries the pass's end marker
    and no queue-written word follows it (a metered pass, whose last launch is k_meter's, needs one)"""
    p = ax.Pool(1, 64)
    p.set_model(model)
    pr = gh.params(**gh.SETS[0])
    p.set_gate(pr)
    x = gh.signal(1, 64, seed=6)
    for _ in range(2):
        p.process(x)
    for on in (False, True, False, True):
        p.set_gate(pr if on else None)
        calls()
        p.process(x)
        c = calls()
        assert c.get("hipStreamWriteValue32", 0) == 0 and c.get("launch_gate", 0) == (1 if on else 0), (on, c)
        assert not {k: v for k, v in c.items() if k in ALLOC | FREE}, c
    p.close()
