"""A census of the pool's host-buffer paths: a fixed script of API calls on the smallest pool of each path, and for every step the test
build's table of HIP runtime calls (aidax_test_hip_calls, aidax_hip_host.h) and the sha256 of every array the step returned. Recorded
once on the commit before the pool's sources were split (tests/golden/pool_census.json) and held against every later build by
tests/test_gpu_pool_census.py: the same calls, the same bits.

    AIDAX_LIB=<a test build's libaidax_hip.so> python -m tests.pool_census --record OUT.json      one recording
    python -m tests.pool_census --merge A.json B.json C.json --out tests/golden/pool_census.json  what all recordings agree on

The pools (streams x frames, environment at creation):
    zc_kernel_word   1 x 64                        zero-copy, the pass writes the completion word itself
    zc_queue_word    1 x 64   AIDAX_KERNEL_WORD=0  ... the queue writes it
    zc_no_word       1 x 64   AIDAX_SPIN_WAIT=0    ... no word: the caller waits for the stream
    zc_five          5 x 64                        zero-copy, one launch for five streams, word by the queue
    zc_multi_launch  4 x 64   AIDAX_KERNEL=quad    a pass of several launches: zero-copy in, the device block and a download out
    staged           70 x 256                      71 680 bytes, over the zero-copy limit: pinned staging, copies both ways
(a seventh, `staged` with AIDAX_ZEROCOPY=0, would be `staged` again — its size alone keeps it off the zero-copy path — and is left out.)

A step's call counts may differ from run to run only in what the 2 ms poll of a completion adds when it runs out (hipEventQuery,
hipStreamSynchronize, hipEventSynchronize in `process` and `collect` steps): --merge drops such entries, names each one in the file, and
refuses anything else that differs."""
import argparse
import ctypes as C
import hashlib
import importlib
import json
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

POOLS = (("zc_kernel_word", 1, 64, {}), ("zc_queue_word", 1, 64, {"AIDAX_KERNEL_WORD": "0"}), ("zc_no_word", 1, 64, {"AIDAX_SPIN_WAIT": "0"}),
         ("zc_five", 5, 64, {}), ("zc_multi_launch", 4, 64, {"AIDAX_KERNEL": "quad"}), ("staged", 70, 256, {}))
MAY_VARY = ("hipEventQuery", "hipStreamSynchronize", "hipEventSynchronize")      # what a poll that runs out of its 2 ms adds ...
MAY_VARY_IN = ("process", "collect")                                             # ... and the steps that poll


def _sha(a):
    a = np.ascontiguousarray(a)
    return hashlib.sha256(str((a.dtype.str, a.shape)).encode() + a.tobytes()).hexdigest()


def _calls_reader(ax):
    fn = ax.lib().aidax_test_hip_calls
    fn.argtypes = [C.c_char_p, C.c_uint32]
    fn.restype = C.c_int
    buf = C.create_string_buffer(4096)

    def read():
        n = fn(buf, len(buf))
        out = {name: int(k) for name, k in (line.split() for line in buf.value.decode().splitlines())}
        assert len(out) == n, (n, out)
        return out
    return read


def _walk(ax, gh, model, read, name, S, n, env):
    """the script on one pool -> [{"step", "calls", "out"}]"""
    steps = []

    def step(label, fn):
        read()
        got = fn()
        got = [] if got is None else [got] if isinstance(got, np.ndarray) else list(got)
        steps.append({"step": f"{len(steps):02d} {label}", "calls": dict(sorted(read().items())), "out": [_sha(a) for a in got]})
        return got

    saved = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        pool = []
        step("create", lambda: pool.append(ax.Pool(S, n)))
    finally:
        for k, v in saved.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)
    p = pool[0]
    x = [gh.signal(S, n, seed=20 + k) for k in range(12)]
    step("set_model", lambda: p.set_model(model))
    for k in (0, 1):
        p.process(x[k])                                     # (warm-ups: not recorded)
    step("process", lambda: p.process(x[2]))
    step("process of 0 frames", lambda: p.process(x[2][:, :0]))
    for k in range(4):                                      # the first submit allocates the pipeline; sync ahead of collect: nothing to poll for
        step("submit", lambda: p.submit(x[3 + k]))
        step("sync", p.sync)
        step("collect", lambda: p.collect(n))
    xin, out = x[7].copy(), np.zeros((S, n), np.float32)
    step("register_host", lambda: (p.register_host(xin), p.register_host(out)) and None)
    step("submit_to", lambda: p.submit_to(xin, out))
    step("sync", p.sync)
    step("collect", lambda: p.collect(n, out))
    step("unregister_host", lambda: (p.unregister_host(xin), p.unregister_host(out)) and None)
    step("set_metering(1)", lambda: p.set_metering(True))
    step("process", lambda: p.process(x[8]))
    step("read_meters with clear", lambda: p.read_meters(clear=True))
    step("set_gate(params, stream 0)", lambda: p.set_gate(gh.params(**gh.SETS[0]), 0))
    step("process", lambda: p.process(x[9]))
    step("set_gate(None)", lambda: p.set_gate(None))
    step("process", lambda: p.process(x[10]))
    step("read_gate", p.read_gate)
    step("sync", p.sync)
    step("close", p.close)
    return steps


def run():
    """-> {pool name: its steps}, on whatever library AIDAX_LIB names (a test build: the shipped library keeps no call table)"""
    ax = importlib.import_module("aidadsp-lv2_amd")
    from tests import gatehelp as gh, modelgen
    path = os.path.join(tempfile.mkdtemp(prefix="pool_census_"), "lstm16.json")
    modelgen.write_model(modelgen.make_model(kind="lstm", hidden=16, input_size=1, seed=5), path)
    model = ax.Model(path)
    read = _calls_reader(ax)
    return {name: _walk(ax, gh, model, read, name, S, n, env) for name, S, n, env in POOLS}


def merge(recordings):
    """what every recording agrees on, plus the list of entries dropped; anything unstable beyond MAY_VARY raises"""
    first, dropped, pools = recordings[0], [], {}
    for name, steps in first.items():
        pools[name] = []
        for i, st in enumerate(steps):
            others = [r[name][i] for r in recordings[1:]]
            assert all(o["step"] == st["step"] for o in others), (name, st["step"])
            assert all(o["out"] == st["out"] for o in others), f"{name} / {st['step']}: an output digest differs between recordings"
            calls = {}
            for k in sorted(set(st["calls"]).union(*(o["calls"] for o in others))):
                counts = [r["calls"].get(k, 0) for r in [st] + others]
                if len(set(counts)) == 1:
                    calls[k] = counts[0]
                    continue
                assert k in MAY_VARY and st["step"].split(" ", 1)[1].split(" of ")[0] in MAY_VARY_IN, f"{name} / {st['step']}: {k} differs between recordings: {counts}"
                dropped.append({"pool": name, "step": st["step"], "call": k, "seen": counts, "why": "the 2 ms poll of the pass's end ran out in some recordings"})
            pools[name].append({"step": st["step"], "calls": calls, "out": st["out"], "not_compared": [d["call"] for d in dropped if d["pool"] == name and d["step"] == st["step"]]})
    return {"recordings": len(recordings), "dropped": dropped, "pools": pools}


def differences(golden, got):
    """every committed entry that `got` (run()'s result) does not reproduce, as text"""
    bad = []
    for name, steps in golden["pools"].items():
        if [s["step"] for s in steps] != [s["step"] for s in got.get(name, [])]:
            bad.append(f"{name}: the steps differ")
            continue
        for want, have in zip(steps, got[name]):
            if want["out"] != have["out"]:
                bad.append(f"{name} / {want['step']}: output digests {have['out']} != {want['out']}")
            have_calls = {k: v for k, v in have["calls"].items() if k not in want["not_compared"]}
            if have_calls != want["calls"]:
                bad.append(f"{name} / {want['step']}: calls {have_calls} != {want['calls']}")
    return bad


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--record")
    ap.add_argument("--merge", nargs="+")
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.record:
        with open(a.record, "w") as f:
            json.dump(run(), f, indent=1)
    if a.merge:
        with open(a.out, "w") as f:
            json.dump(merge([json.load(open(p)) for p in a.merge]), f, indent=1)
            f.write("\n")
