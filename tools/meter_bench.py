"""Cost of the stream meters (aidax_pool_set_metering, k_meter) on the shipped library: writes profiles/meters.txt.

One process, one pool per case, metering switched off and on in alternating legs (off, on, off, on, ...), so that both sides see the same
clocks and the same neighbours on the box:

  cfg2          1024 streams of the LSTM-32 amp model, 256-frame blocks, device-resident: aidax_pool_process_device back to back on one
                torch stream, device events around --steps blocks per leg. us per block off and on; their difference is what the two
                k_meter launches of a pass add to it (kernel time and the gaps around them; one launch: half of that).
  one_stream    the LV2 instance's case, one stream of the bundled LSTM-12 model through the blocking aidax_pool_process at 64 and 256
                frames (the zero-copy path: a metered pass gives up the kernel-written completion word, and k_meter reads its two
                blocks from pinned host memory): p50 and p99 of --calls round trips per leg.

k_meter's own time, launch by launch, is not in here: run the tool under `rocprofv3 --kernel-trace --stats` with --no-write for that
(a run of its own: tracing slows the host side).

    python3 tools/meter_bench.py [--steps 1000] [--warmup 100] [--legs 3] [--calls 1000] [--out FILE] [--no-write]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--warmup", type=int, default=100)
    ap.add_argument("--legs", type=int, default=3)
    ap.add_argument("--calls", type=int, default=1000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "meters.txt"))
    ap.add_argument("--no-write", action="store_true")
    a = ap.parse_args()
    import torch
    ax = importlib.import_module("aidadsp-lv2_amd")
    W = ax.workloads
    lines = ["The stream meters (aidax_pool_set_metering, k_meter): tools/meter_bench.py on an MI355X.",
             f"library {os.path.relpath(ax.lib_path(), ROOT)}; {a.legs} legs each way, alternating off / on in one process; "
             f"{a.steps} blocks per cfg2 leg after {a.warmup} of warm-up, {a.calls} round trips per one-stream leg", ""]

    d = tempfile.mkdtemp(prefix="meter_bench_")
    S, n = 1024, 256
    pool = ax.Pool(S, n)
    pool.set_model(ax.Model(W.write_model(W.make_model("lstm", 32, 1, seed=32), os.path.join(d, "lstm32.json"))))
    pool.set_metering(True)                                     # set-up side: the records exist before the first leg
    s = torch.cuda.Stream()
    x = torch.from_numpy(W.signal(S, n, seed=5)).cuda()
    y = torch.empty_like(x)
    legs = {False: [], True: []}
    for _ in range(a.legs):
        for on in (False, True):
            pool.set_metering(on)
            legs[on].append(timed(torch, s, a.steps, a.warmup, lambda: pool.process_device(x.data_ptr(), y.data_ptr(), n, s.cuda_stream)))
    rec = pool.read_meters(0, 1)[0]
    off, on = float(np.median(legs[False])), float(np.median(legs[True]))
    lines += [f"cfg2: {S} streams x LSTM-32 x {n} frames, aidax_pool_process_device, device events ({pool.kernel_name})",
              "   us per block, metering off: " + "  ".join(f"{v:7.2f}" for v in legs[False]) + f"   median {off:7.2f}",
              "   us per block, metering on:  " + "  ".join(f"{v:7.2f}" for v in legs[True]) + f"   median {on:7.2f}",
              f"   the two k_meter launches of a pass add {on - off:.2f} us per block ({100.0 * (on - off) / off:.1f} %), {0.5 * (on - off):.2f} us a launch "
              f"(2 x {S * n * 4 / 1e6:.2f} MB read per pass)",
              f"   stream 0 after the run: {int(rec['passes'])} passes, {int(rec['frames'])} frames metered "
              f"(= {a.legs} legs x {a.steps + a.warmup} blocks x {n})", ""]
    pool.close()

    lv2 = os.path.join(ROOT, "tests", "golden", "models", "tw40_california_clean_deerinkstudios.json")
    lines.append("one stream x LSTM-12 (the bundled model), blocking aidax_pool_process round trip on the host clock, us")
    for n in (64, 256):
        pool = ax.Pool(1, n)
        pool.set_model(ax.Model(lv2))
        pool.set_metering(True)
        blk = np.ascontiguousarray(W.signal(1, n, seed=6))
        legs = {False: [], True: []}
        for _ in range(a.legs):
            for on in (False, True):
                pool.set_metering(on)
                legs[on].append(round_trips(pool.process, blk, a.calls))
        for on in (False, True):
            p50 = [v[0] for v in legs[on]]
            p99 = [v[1] for v in legs[on]]
            lines.append(f"   {n:3d} frames, metering {'on: ' if on else 'off:'} p50 " + "  ".join(f"{v:7.2f}" for v in p50) + f"   median {np.median(p50):7.2f}"
                         "     p99 " + "  ".join(f"{v:7.2f}" for v in p99))
        lines.append(f"   {n:3d} frames: metering adds {np.median([v[0] for v in legs[True]]) - np.median([v[0] for v in legs[False]]):.2f} us to the p50 round trip ({pool.kernel_name})")
        pool.close()
    text = "\n".join(lines) + "\n"
    print(text)
    if not a.no_write:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
