"""Cost of the mix buses (aidax_pool_set_buses, k_mix) on the shipped library: writes profiles/mix_buses.txt.

  stage     1024 streams of the LSTM-32 amp model, 256-frame blocks, device-resident: aidax_pool_process_device back to back on one torch
            stream, device events around --steps blocks per leg. Four pools in one process — buses never enabled, 512 buses x 2 entries,
            64 buses x 16 entries, 1 bus x 1024 entries — measured in alternating legs (never, 512x2, 64x16, 1x1024, never, ...), so that
            all of them see the same clocks and the same neighbours on the box. us per block each; the difference to "never" is what the
            k_mix launch of a pass adds (kernel time and the gaps around it).
  parent    with --parent-lib FILE (a build of the parent commit's library): the "never" case alone, in child processes that alternate
            between that library and this one (AIDAX_LIB), --legs legs each. "Buses never enabled changes nothing" is the claim that this
            build's figures sit inside the parent's run-to-run spread.
  host      all 1024 streams into 64 buses through the blocking host calls, on the host clock: aidax_pool_process (2 x 1 MB moved),
            aidax_pool_process_buses (1 MB up, 64 KB down), aidax_pool_process followed by aidax_pool_read_buses. p50 and p99 of --calls
            round trips per leg, the three in alternating legs.

k_mix's own time, launch by launch, is not measured in here: run the tool under `rocprofv3 --kernel-trace --stats` with --no-write --only
long for that (a run of its own: tracing slows the host side), and write what it shows into the profile by hand, from a line that
starts with "kernel trace" to the file's end. A run that writes the profile carries that section over from the file it replaces.

    python3 tools/mix_bench.py [--steps 1000] [--warmup 100] [--legs 3] [--calls 300] [--parent-lib FILE] [--only stage|long|host|never] [--out FILE] [--no-write]
"""
import argparse
import importlib
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
S, N = 1024, 256


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


def round_trips(fn, calls):
    for _ in range(30):
        fn()
    t = np.empty(calls)
    for i in range(calls):
        t0 = time.perf_counter()
        fn()
        t[i] = time.perf_counter() - t0
    return float(np.percentile(t, 50)) * 1e6, float(np.percentile(t, 99)) * 1e6


def make_pool(ax, model, buses, per_bus):
    """a cfg2 pool whose `buses` buses have `per_bus` entries each. The buses * per_bus entries are dealt out in the order of the
    sends, send 0 of every stream first, then send 1 and so on; entry e goes to bus e * buses // total, so every bus gets a run of
    per_bus consecutive entries"""
    pool = ax.Pool(S, N)
    pool.set_model(model)
    if buses:
        pool.set_buses(buses)
        total = buses * per_bus                                 # entries in all: a multiple of S, or fewer than S
        for e in range(total):
            s, j = e % S, e // S
            pool.set_send(s, j, (e * buses) // total, 0.25 + 0.5 * (e % 7) / 7.0, 0)
    return pool


def trace_section(path):
    """the hand-written kernel-trace section of the profile at `path` (from its line that starts with "kernel trace" on), or nothing"""
    try:
        with open(path) as f:
            old = f.read().splitlines()
    except OSError:
        return ""
    at = [i for i, line in enumerate(old) if line.startswith("kernel trace")]
    return "\n".join(old[at[0]:]) + "\n" if at else ""


def fmt(vals):
    return "  ".join(f"{v:7.2f}" for v in vals) + f"   median {np.median(vals):7.2f}  spread {max(vals) - min(vals):5.2f}"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--warmup", type=int, default=100)
    ap.add_argument("--legs", type=int, default=3)
    ap.add_argument("--calls", type=int, default=300)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--only", default=None, choices=("stage", "long", "host", "never"))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mix_buses.txt"))
    ap.add_argument("--no-write", action="store_true")
    a = ap.parse_args()
    import torch
    ax = importlib.import_module("aidadsp-lv2_amd")
    W = ax.workloads
    d = tempfile.mkdtemp(prefix="mix_bench_")
    try:
        model = ax.Model(W.write_model(W.make_model("lstm", 32, 1, seed=32), os.path.join(d, "lstm32.json")))
    finally:
        shutil.rmtree(d, ignore_errors=True)                    # (the model is loaded: the file has served)
    s = torch.cuda.Stream()
    x_host = W.signal(S, N, seed=5)
    x = torch.from_numpy(x_host).cuda()
    y = torch.empty_like(x)

    if a.only == "never":                                       # a child of the parent comparison: one JSON line
        pool = make_pool(ax, model, 0, 0)
        legs = [timed(torch, s, a.steps, a.warmup, lambda: pool.process_device(x.data_ptr(), y.data_ptr(), N, s.cuda_stream)) for _ in range(a.legs)]
        print(json.dumps({"lib": ax.lib_path(), "kernel": pool.kernel_name, "us": legs}))
        pool.close()
        return

    lines = ["The mix buses (aidax_pool_set_buses, k_mix): tools/mix_bench.py on an MI355X.",
             f"library {os.path.relpath(ax.lib_path(), ROOT)}; {a.legs} legs per case, alternating in one process; {a.steps} blocks per leg after {a.warmup} of warm-up, "
             f"{a.calls} round trips per host leg", ""]

    if a.only in (None, "stage", "long"):
        cases = [("never enabled", 0, 0), ("512 buses x 2", 512, 2), ("64 buses x 16", 64, 16), ("1 bus x 1024", 1, 1024)]
        if a.only == "long":
            cases = cases[-1:]
        pools = [make_pool(ax, model, b, n) for _, b, n in cases]
        legs = [[] for _ in cases]
        for _ in range(a.legs):
            for k, pool in enumerate(pools):
                legs[k].append(timed(torch, s, a.steps, a.warmup, lambda: pool.process_device(x.data_ptr(), y.data_ptr(), N, s.cuda_stream)))
        lines.append(f"stage: {S} streams x LSTM-32 x {N} frames, aidax_pool_process_device, device events ({pools[0].kernel_name}), us per block")
        base = float(np.median(legs[0])) if cases[0][1] == 0 else None
        for (name, b, n), v in zip(cases, legs):
            extra = "" if base is None or b == 0 else f"   k_mix's launch adds {np.median(v) - base:6.2f} us ({100.0 * (np.median(v) - base) / base:.1f} %)"
            lines.append(f"   {name:15s} " + fmt(v) + extra)
        lines.append(f"   (a pass's stream block is {S * N * 4 / 1e6:.2f} MB; k_mix reads entries x {N * 4} B and writes buses x {N * 4} B)")
        lines.append("")
        for pool in pools:
            pool.close()

    if a.parent_lib and a.only is None:
        runs = {"parent": [], "this": []}
        me = os.path.abspath(__file__)
        for _ in range(2):
            for who, lib in (("parent", os.path.abspath(a.parent_lib)), ("this", ax.lib_path())):
                r = subprocess.run([sys.executable, me, "--only", "never", "--steps", str(a.steps), "--warmup", str(a.warmup), "--legs", str(a.legs), "--no-write"],
                                   env=dict(os.environ, AIDAX_LIB=lib), capture_output=True, text=True, timeout=600)
                if r.returncode != 0:
                    raise SystemExit(f"the {who} leg failed: {r.stderr[-2000:]}")
                runs[who].append(json.loads(r.stdout.strip().splitlines()[-1]))
        lines.append("parent: buses never enabled, this build against a build of the parent commit, alternating child processes (parent, this, parent, this), us per block")
        for who in ("parent", "this"):
            v = [u for r in runs[who] for u in r["us"]]
            lines.append(f"   {who:7s} ({runs[who][0]['kernel']}) " + fmt(v))
        p = [u for r in runs["parent"] for u in r["us"]]
        t = [u for r in runs["this"] for u in r["us"]]
        inside = min(p) <= np.median(t) <= max(p)
        lines.append(f"   this build's median {np.median(t):.2f} lies {'inside' if inside else 'OUTSIDE'} the parent's range {min(p):.2f} .. {max(p):.2f}")
        lines.append("")

    if a.only in (None, "host"):
        pool = make_pool(ax, model, 64, 16)
        legs = {"process": [], "process_buses": [], "process + read_buses": []}
        fns = {"process": lambda: pool.process(x_host), "process_buses": lambda: pool.process_buses(x_host),
               "process + read_buses": lambda: (pool.process(x_host), pool.read_buses())}
        for _ in range(a.legs):
            for name, fn in fns.items():
                legs[name].append(round_trips(fn, a.calls))
        lines.append(f"host: {S} streams -> 64 buses x 16 entries, {N} frames, blocking calls through the ctypes binding, host clock, us per round trip")
        for name, v in legs.items():
            lines.append(f"   {name:22s} p50 " + fmt([q[0] for q in v]) + "     p99 " + "  ".join(f"{q[1]:7.2f}" for q in v))
        lines.append("")
        pool.close()

    text = "\n".join(lines)
    print(text)
    if not a.no_write:
        text += trace_section(a.out)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
