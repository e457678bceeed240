"""Stream meters in real time (GPU, -m gpu): once the set-up side has enabled them, aidax_pool_set_metering is a host record (no HIP call
at all), and a metered pass allocates, frees and waits for nothing: two launches of k_meter more, none for a zero-length pass or while
metering is off. Counted by the test build's per-thread table of the pool's own HIP runtime calls (aidax_test_hip_calls, aidax_hip_host.h);
the shipped library has no such table: these tests run on the test build only."""
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
    p = str(tmp_path_factory.mktemp("meters_rt") / "lstm16.json")
    modelgen.write_model(modelgen.make_model(kind="lstm", hidden=16, input_size=1, seed=5), p)
    return ax.Model(p)


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

    def pass_(self, pool, n=None):
        with self.torch.cuda.stream(self.s):
            pool.process_device(self.x.data_ptr(), self.y.data_ptr(), self.x.shape[1] if n is None else n, self.s.cuda_stream)

    def wait(self):
        self.s.synchronize()


def test_the_first_enabling_call_allocates_and_later_ones_make_no_hip_call(model, calls):
    p = ax.Pool(70, 256)
    p.set_model(model)
    calls()
    p.set_metering(True)                                    # set-up side
    c = calls()
    assert c.get("hipMalloc") == 1 and c.get("hipHostMalloc") == 1, c
    for on in (False, True, True, False, True):             # audio side
        p.set_metering(on)
        assert p.metering == on
        assert calls() == {}
    p.close()


def test_metered_passes_allocate_free_and_wait_for_nothing(model, calls):
    S = 70
    p = ax.Pool(S, 256)
    p.set_model(model)
    p.set_metering(True)
    dev = _Device(S, 256, seed=5)
    dev.pass_(p)
    dev.wait()
    calls()
    for on, n, launches in ((True, 256, 2), (True, 0, 0), (False, 256, 0), (True, 100, 2), (False, 0, 0), (True, 256, 2)):
        p.set_metering(on)
        assert calls() == {}
        dev.pass_(p, n)
        c = calls()
        _quiet(c, f"pass of {n} frames, metering {on}")
        assert c.get("launch_meter", 0) == launches, (on, n, c)
        dev.wait()
    rec = p.read_meters()
    assert list(rec["passes"]) == [4] * S and list(rec["frames"]) == [256 + 256 + 100 + 256] * S
    p.close()


def test_a_metered_pass_ends_behind_the_output_side(model, calls):
    """The blocking path of a one-stream pool: unmetered, the model's kernel writes the completion word itself and no packet follows the
    pass; metered, the pass's end marker is withheld from the model's launch and the queue writes the word behind the output side's
    k_meter (one hipStreamWriteValue32), as behind the IR stage. The records alone cannot show an end marker issued too early: nothing the
    host does between two blocking passes writes the blocks the output side reads."""
    p = ax.Pool(1, 64)
    p.set_model(model)
    p.set_metering(True)
    x = np.ascontiguousarray(modelgen.signal(1, 64, seed=6))
    for _ in range(2):
        p.process(x)
    for on, words, launches in ((False, 0, 0), (True, 1, 2), (False, 0, 0), (True, 1, 2)):
        p.set_metering(on)
        calls()
        p.process(x)
        c = calls()
        assert c.get("hipStreamWriteValue32", 0) == words and c.get("launch_meter", 0) == launches, (on, c)
        assert not {k: v for k, v in c.items() if k in ALLOC | FREE}, c
    assert p.read_meters()["passes"][0] == 4
    p.close()
