"""Cost of the noise gate (aidax_pool_set_gate, k_gate) on the shipped library: writes profiles/gate.txt.

One process, one pool per case, every stream's gate switched off and on in alternating legs (off, on, off, on, ...), so that both sides
see the same clocks and the same neighbours on the box:

  cfg2          1024 streams of the LSTM-32 amp model, 256-frame blocks, device-resident: aidax_pool_process_device back to back on one
                torch stream, device events around --steps blocks per leg. us per block off and on; their difference is what the
                k_gate launch of a pass adds to it (kernel time and the gaps around it).
  one_stream    the LV2 instance's case, one stream of the bundled LSTM-12 model through the blocking aidax_pool_process at 64 and 256
                frames (the zero-copy path: k_gate reads its block from pinned host memory, the model's kernel reads the side block and
                still writes the completion word itself): p50 and p99 of --calls round trips per leg.

The input is bursts over a noise bed, so that the gates open and close while the legs run. k_gate's own time, launch by launch, is not
in here: run the tool under `rocprofv3 --kernel-trace --stats` with --no-write for that (a run of its own: tracing slows the host side).

    python3 tools/gate_bench.py [--steps 1000] [--warmup 100] [--legs 3] [--calls 1000] [--out FILE] [--no-write]
"""
import argparse
import importlib
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(torch, s, steps, warmup, call):
    """us per call of `call()`, issued back to back on torch stream s between two events"""
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        for _ in range(warmup):
            call()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(s)
        for _ in range(steps):
            call()
        e1.record(s)
    s.synchronize()
    return e0.elapsed_time(e1) * 1000.0 / steps


def round_trips(fn, x, calls):
    for _ in range(50):
        fn(x)
    t = np.empty(calls)
    for i in range(calls):
        t0 = time.perf_counter()
        fn(x)
        t[i] = time.perf_counter() - t0
    return float(np.percentile(t, 50)) * 1e6, float(np.percentile(t, 99)) * 1e6


def bursts(S, n, seed):
    """the guitar-level test signal, every other 32-frame stretch turned down to a noise bed 60 dB below it"""
    W = importlib.import_module("aidadsp-lv2_amd").workloads
    x = W.signal(S, n, seed=seed)
    quiet = (np.arange(n) // 32) % 2 == 1
    x[:, quiet] *= np.float32(0.001)
    return np.ascontiguousarray(x)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--warmup", type=int, default=100)
    ap.add_argument("--legs", type=int, default=3)
    ap.add_argument("--calls", type=int, default=1000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gate.txt"))
    ap.add_argument("--no-write", action="store_true")
    a = ap.parse_args()
    import torch
    ax = importlib.import_module("aidadsp-lv2_amd")
    W = ax.workloads
    gate = ax.GateParams(-40.0, -46.0, -60.0, 0.1, 0.25, 0.5)         # short times: the gates open and close inside every block
    lines = ["The noise gate (aidax_pool_set_gate, k_gate): tools/gate_bench.py on an MI355X.",
             f"library {os.path.relpath(ax.lib_path(), ROOT)}; {a.legs} legs each way, alternating off / on in one process; "
             f"{a.steps} blocks per cfg2 leg after {a.warmup} of warm-up, {a.calls} round trips per one-stream leg", ""]

    d = tempfile.mkdtemp(prefix="gate_bench_")
    S, n = 1024, 256
    pool = ax.Pool(S, n)
    pool.set_model(ax.Model(W.write_model(W.make_model("lstm", 32, 1, seed=32), os.path.join(d, "lstm32.json"))))
    pool.set_gate(gate)                                         # set-up side: records, states and the side block exist before the first leg
    s = torch.cuda.Stream()
    x = torch.from_numpy(bursts(S, n, seed=5)).cuda()
    y = torch.empty_like(x)
    legs = {False: [], True: []}
    for _ in range(a.legs):
        for on in (False, True):
            pool.set_gate(gate if on else None)
            legs[on].append(timed(torch, s, a.steps, a.warmup, lambda: pool.process_device(x.data_ptr(), y.data_ptr(), n, s.cuda_stream)))
    st = pool.read_gate()
    off, on = float(np.median(legs[False])), float(np.median(legs[True]))
    lines += [f"cfg2: {S} streams x LSTM-32 x {n} frames, aidax_pool_process_device, device events ({pool.kernel_name})",
              "   us per block, gate off: " + "  ".join(f"{v:7.2f}" for v in legs[False]) + f"   median {off:7.2f}",
              "   us per block, gate on:  " + "  ".join(f"{v:7.2f}" for v in legs[True]) + f"   median {on:7.2f}",
              f"   the k_gate launch of a pass adds {on - off:.2f} us per block ({100.0 * (on - off) / off:.1f} %) "
              f"({S * n * 4 / 1e6:.2f} MB read and {S * n * 4 / 1e6:.2f} MB written per pass)",
              f"   after the run: {int((st['hold_left'] > 0).sum())} streams open, {int((st['atten'] == 1 << 24).sum())} fully closed, "
              f"{int(((st['atten'] > 0) & (st['atten'] < 1 << 24)).sum())} on a ramp", ""]
    pool.close()

    lv2 = os.path.join(ROOT, "tests", "golden", "models", "tw40_california_clean_deerinkstudios.json")
    lines.append("one stream x LSTM-12 (the bundled model), blocking aidax_pool_process round trip on the host clock, us")
    for n in (64, 256):
        pool = ax.Pool(1, n)
        pool.set_model(ax.Model(lv2))
        pool.set_gate(gate)
        blk = bursts(1, n, seed=6)
        legs = {False: [], True: []}
        for _ in range(a.legs):
            for on in (False, True):
                pool.set_gate(gate if on else None)
                legs[on].append(round_trips(pool.process, blk, a.calls))
        for on in (False, True):
            p50 = [v[0] for v in legs[on]]
            p99 = [v[1] for v in legs[on]]
            lines.append(f"   {n:3d} frames, gate {'on: ' if on else 'off:'} p50 " + "  ".join(f"{v:7.2f}" for v in p50) + f"   median {np.median(p50):7.2f}"
                         "     p99 " + "  ".join(f"{v:7.2f}" for v in p99))
        lines.append(f"   {n:3d} frames: the gate adds {np.median([v[0] for v in legs[True]]) - np.median([v[0] for v in legs[False]]):.2f} us to the p50 round trip ({pool.kernel_name})")
        pool.close()
    text = "\n".join(lines) + "\n"
    print(text)
    if not a.no_write:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
