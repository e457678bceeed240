"""Cost of the stream tuners (aidax_pool_set_tuning, k_tune) on the shipped library: writes profiles/tuner.txt.

One process, one pool per case, the cases taken in turn in every leg (never, off, hop 1024, hop 256, never, ...), so that all of them see
the same clocks and the same neighbours on the box:

  cfg2          1024 streams of the LSTM-32 amp model, 256-frame blocks, device-resident: aidax_pool_process_device back to back on one
                torch stream, device events around --steps blocks per leg, us per block.
                  never     a pool that never enabled the stage
                  off       a pool that set it up (window 2048) and switched it off
                  hop 1024  every stream's tuner on: one pass in four analyses all 1024 streams, the other three append
                  hop 256   every pass analyses all 1024 streams
  one_stream    the LV2 instance's case, one stream of the bundled LSTM-12 model through the blocking aidax_pool_process at 64 and 256
                frames: p50 and p99 of --calls round trips per leg, the same four cases.

With AIDAX_LIB naming a library from before the stage (the parent commit's build) only the `never` case exists: that run gives the
parent's own figures and their spread, which the never and off figures of this commit are held against (--label names the run in the
file, --append adds it to the file instead of replacing it).

    python3 tools/tuner_bench.py [--steps 1000] [--warmup 100] [--legs 3] [--calls 1000] [--out FILE] [--no-write] [--append] [--label TEXT]
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

CASES = ("never", "off", "hop 1024", "hop 256")


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


def dress(ax, pool, case):
    """the pool of one case"""
    if case == "never":
        return pool
    pool.set_tuning(ax.tuner_params(window=2048, hop=256 if case == "hop 256" else 1024))
    if case == "off":
        pool.set_tuning(None)
    else:
        pool.set_tuner(True)
    return pool


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--warmup", type=int, default=100)
    ap.add_argument("--legs", type=int, default=3)
    ap.add_argument("--calls", type=int, default=1000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tuner.txt"))
    ap.add_argument("--no-write", action="store_true")
    ap.add_argument("--append", action="store_true")
    ap.add_argument("--label", default="this commit")
    a = ap.parse_args()
    import torch
    ax = importlib.import_module("aidadsp-lv2_amd")
    W = ax.workloads
    cases = CASES if hasattr(ax.lib(), "aidax_pool_set_tuning") else CASES[:1]
    lines = [f"The stream tuners (aidax_pool_set_tuning, k_tune): tools/tuner_bench.py on an MI355X, {a.label}.",
             f"library {os.path.relpath(ax.lib_path(), ROOT)}; {a.legs} legs per case, the cases in turn in one process; "
             f"{a.steps} blocks per cfg2 leg after {a.warmup} of warm-up, {a.calls} round trips per one-stream leg", ""]

    d = tempfile.mkdtemp(prefix="tuner_bench_")
    S, n = 1024, 256
    model = ax.Model(W.write_model(W.make_model("lstm", 32, 1, seed=32), os.path.join(d, "lstm32.json")))
    pools = {}
    for case in cases:
        pools[case] = ax.Pool(S, n)
        pools[case].set_model(model)
        dress(ax, pools[case], case)
    s = torch.cuda.Stream()
    x = torch.from_numpy(W.signal(S, n, seed=5)).cuda()
    y = torch.empty_like(x)
    legs = {case: [] for case in cases}
    for _ in range(a.legs):
        for case in cases:
            pool = pools[case]
            legs[case].append(timed(torch, s, a.steps, a.warmup, lambda: pool.process_device(x.data_ptr(), y.data_ptr(), n, s.cuda_stream)))
    med = {case: float(np.median(legs[case])) for case in cases}
    lines.append(f"cfg2: {S} streams x LSTM-32 x {n} frames, aidax_pool_process_device, device events ({pools['never'].kernel_name}), us per block")
    for case in cases:
        lines.append(f"   {case:9s} " + "  ".join(f"{v:7.2f}" for v in legs[case]) + f"   median {med[case]:7.2f}   spread {max(legs[case]) - min(legs[case]):5.2f}"
                     + ("" if case == "never" else f"   {med[case] - med['never']:+7.2f} us against never ({100.0 * (med[case] - med['never']) / med['never']:+.2f} %)"))
    for case in cases[2:]:
        rd = pools[case].read_tuners(0, 1)[0]
        lines.append(f"   {case}: stream 0 after the run: {int(rd['analyses'])} analyses, the last at frame {int(rd['frame'])} "
                     f"(= {a.legs} legs x {a.steps + a.warmup} blocks x {n})")
    if len(cases) > 2:
        # a pass of hop 1024 analyses one time in four: per analysing pass, against the appending ones
        lines.append(f"   an analysing pass of {S} streams (window 2048, lags to 687, 3 tiles) costs {med['hop 256'] - med['never']:.2f} us; "
                     f"an appending pass about {(4.0 * (med['hop 1024'] - med['never']) - (med['hop 256'] - med['never'])) / 3.0:.2f} us")
    lines.append("")
    for pool in pools.values():
        pool.close()

    lv2 = os.path.join(ROOT, "tests", "golden", "models", "tw40_california_clean_deerinkstudios.json")
    lines.append("one stream x LSTM-12 (the bundled model), blocking aidax_pool_process round trip on the host clock, us")
    for n in (64, 256):
        pools = {}
        for case in cases:
            pools[case] = ax.Pool(1, n)
            pools[case].set_model(ax.Model(lv2))
            dress(ax, pools[case], case)
        blk = np.ascontiguousarray(W.signal(1, n, seed=6))
        legs = {case: [] for case in cases}
        for _ in range(a.legs):
            for case in cases:
                legs[case].append(round_trips(pools[case].process, blk, a.calls))
        base = float(np.median([v[0] for v in legs["never"]]))
        for case in cases:
            p50 = [v[0] for v in legs[case]]
            p99 = [v[1] for v in legs[case]]
            lines.append(f"   {n:3d} frames, {case:9s} p50 " + "  ".join(f"{v:7.2f}" for v in p50) + f"   median {np.median(p50):7.2f}"
                         "     p99 " + "  ".join(f"{v:7.2f}" for v in p99) + ("" if case == "never" else f"   {np.median(p50) - base:+6.2f} us against never"))
        for pool in pools.values():
            pool.close()
    text = "\n".join(lines) + "\n"
    print(text)
    if not a.no_write:
        with open(a.out, "a" if a.append else "w") as f:
            f.write(("\n" if a.append else "") + text)


if __name__ == "__main__":
    main()
