"""What a pool allocates it gives back (GPU, -m gpu): one thread creates a pool, swaps two models in through prepare / commit / free,
enables every stage that allocates on first use (meters, a gate, buses, bus limiting, bus reverbs, an IR), runs one blocking pass and one
submit / collect, and destroys the pool. Over the whole sequence every allocating call of the pool's sources has its freeing call, and
the totals are the ones recorded on the commit before the owning types (DevBuf, PinnedBuf, Event: aidax_hip_host.h) replaced the
hand-written release lists. Counted by the test build's per-thread table (aidax_test_hip_calls), read as tests/test_gpu_gate_rt.py
reads it; the shipped library has no such table.

A hub's life likewise (its sources' calls are counted like the pool's): created, a model set, seats attached and detached, periods run and
closed by the launcher thread, destroyed — all the allocating calls on the creating thread, each with its freeing call."""
import ctypes as C
import importlib

import numpy as np
import pytest

from tests import conftest, gatehelp as gh, modelgen

pytestmark = pytest.mark.gpu
ax = importlib.import_module("aidadsp-lv2_amd")

S, N, BUSES = 4, 16, 2
PAIRS = ((("hipMalloc",), "hipFree"), (("hipHostMalloc",), "hipHostFree"), (("hipEventCreateWithFlags",), "hipEventDestroy"),
         (("hipStreamCreateWithFlags", "hipStreamCreateWithPriority"), "hipStreamDestroy"))
# the sequence's totals on the parent commit (recorded there with this test; AIDAX_KEEP_WARM_US unset: its thread counts elsewhere)
RECORDED = {"hipMalloc": 33, "hipHostMalloc": 38, "hipEventCreateWithFlags": 38, "hipStreamCreateWithFlags": 2, "hipStreamCreateWithPriority": 2}


def read_calls():
    fn = ax.lib().aidax_test_hip_calls
    fn.argtypes = [C.c_char_p, C.c_uint32]
    fn.restype = C.c_int
    buf = C.create_string_buffer(4096)
    n = fn(buf, len(buf))
    out = {}
    for line in buf.value.decode().splitlines():
        name, k = line.split()
        out[name] = int(k)
    assert len(out) == n, (n, out)
    return out


def test_every_allocation_of_a_pools_life_is_freed(tmp_path, monkeypatch):
    if conftest.SHIP_LEG:
        pytest.skip("aidax_test_hip_calls: a test hook — the shipped library has none")
    monkeypatch.delenv("AIDAX_KEEP_WARM_US", raising=False)
    models = []
    for seed in (5, 6):
        path = str(tmp_path / f"lstm16_{seed}.json")
        modelgen.write_model(modelgen.make_model(kind="lstm", hidden=16, input_size=1, seed=seed), path)
        models.append(ax.Model(path))
    x = gh.signal(S, N, seed=7)
    read_calls()

    p = ax.Pool(S, N)
    for m in models:                                            # the first swap retires the empty slot, the second the first model
        sg = p.prepare_model(m)
        p.commit_model(sg)
        p.staged_free(sg)
    p.set_metering(True)
    p.set_gate(gh.params(**gh.SETS[0]))
    p.set_buses(BUSES)
    for s in range(S):
        p.set_send(s, 0, s % BUSES)
    p.set_bus_limiting(True)
    p.set_bus_limiter(ax.BusLimitParams(-6.0, 1.0, 0.0))
    p.set_bus_reverbs(True)
    p.set_bus_reverb(ax.BusReverbParams(1.0, 0.05, 0.3, 0.5, 1.0, 0))
    p.set_ir(np.linspace(1.0, 0.0, 64, dtype=np.float32))
    y = p.process(x)
    p.submit(x)
    y2 = p.collect(N)
    assert np.isfinite(y).all() and np.isfinite(y2).all()
    p.close()

    c = read_calls()
    print("alloc balance:", {k: c.get(k, 0) for k in sorted(set(RECORDED) | {free for _, free in PAIRS})})
    for allocs, free in PAIRS:
        assert sum(c.get(a, 0) for a in allocs) == c.get(free, 0), (allocs, free, c)
    assert {k: c.get(k, 0) for k in RECORDED} == RECORDED, c
    assert c.get("hipHostRegister", 0) == 0 and c.get("hipHostUnregister", 0) == 0, c
    for m in models:
        m.close()


def test_every_allocation_of_a_hubs_life_is_freed(tmp_path, monkeypatch):
    if conftest.SHIP_LEG:
        pytest.skip("aidax_test_hip_calls: a test hook — the shipped library has none")
    monkeypatch.delenv("AIDAX_KEEP_WARM_US", raising=False)
    path = str(tmp_path / "lstm8.json")
    modelgen.write_model(modelgen.make_model(kind="lstm", hidden=8, input_size=1, seed=1), path)
    m = ax.Model(path)
    seats, n = 4, 64
    x = gh.signal(2, 4 * n, seed=8)
    read_calls()

    h = ax.Hub(seats, n)
    h.set_deadline_us(0)                                        # a period closes when every attached seat has submitted
    h.set_model(m)
    a, b = h.attach(), h.attach()
    got = []
    for k in range(3):
        got.append([h.run(s, x[i, k * n:(k + 1) * n]) for i, s in enumerate((a, b))])
    h.detach(b)
    got.append([h.run(a, x[0, 3 * n:])])
    assert h.launches >= 3 and all(np.isfinite(y).all() for row in got for y in row)
    h.close()

    c = read_calls()
    print("hub alloc balance:", {k: c.get(k, 0) for k in sorted(set(RECORDED) | {free for _, free in PAIRS})})
    for allocs, free in PAIRS:
        assert sum(c.get(a_, 0) for a_ in allocs) == c.get(free, 0), (allocs, free, c)
    # the hub's own: two device blocks, two pinned staging blocks per rotating buffer and the peek record, an event per buffer and the
    # peek's, one stream — on top of whatever its pool makes
    assert c.get("hipMalloc", 0) >= 2 and c.get("hipHostMalloc", 0) >= 9 and c.get("hipEventCreateWithFlags", 0) >= 5, c
    assert c.get("hipStreamCreateWithFlags", 0) >= 1, c
    m.close()
