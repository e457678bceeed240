"""Cost of the stream delays (aidax_pool_set_delays, k_delay) on the shipped library: writes profiles/stream_delay.txt.

  stage     1024 streams of the LSTM-32 amp model, 256-frame blocks, device-resident: aidax_pool_process_device back to back on one torch
            stream, device events around --steps blocks per leg. No buses. Six pools in one process, measured in alternating legs so
            that all of them see the same clocks and the same neighbours on the box:
              the stage never enabled | on, every delay off | every delay on at m = 300 (one chunk per block) | at m = 64 (four chunks) |
              m = 300 modulated (depth 20 frames, 3 Hz) | the same with a crossfade in progress through the whole leg (300 <-> 400)
            us per block each; the difference to "never enabled" is what the k_delay launch of a pass adds (kernel time and the gaps
            around it).
  parent    with --parent-lib FILE (a build of the parent commit's library): the stage never enabled, in child processes that alternate
            between that library and this one (AIDAX_LIB), --legs legs each. "A pool that does not ask for the stage pays nothing" is
            the claim that this build's figures sit inside the parent's own run-to-run spread, which is measured here, not assumed.
  one       the LV2 instance's case: one stream of the bundled LSTM-12 model through the blocking aidax_pool_process at 64 and 256
            frames, with and without a delay, on the host clock.

k_delay's own time, launch by launch, is not measured in here: run the tool under `rocprofv3 --kernel-trace --stats` with --no-write
--only long (or short, fade) for that (a run of its own: tracing slows the host side), and write what it shows into the profile by hand,
from a line that starts with "kernel trace" to the file's end. A run that writes the profile carries that section over from the file it
replaces.

    python3 tools/delay_bench.py [--steps 1000] [--warmup 100] [--legs 3] [--calls 300] [--parent-lib FILE] [--only stage|long|short|fade|one|never] [--out FILE] [--no-write]
"""
import argparse
import importlib
import json
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools.mix_bench import S, N, fmt, make_pool, round_trips, timed, trace_section  # noqa: E402

CAPACITY = 4096
FADE = 1 << 20                                                   # (a fade that outlasts every leg)


def ring_row(capacity, max_frames):
    """floats of a stream's ring row: the power of two at or above capacity + 3 + max_frames (include/aidax.h, aidax_pool_set_delays)"""
    row = 1
    while row < capacity + 3 + max_frames:
        row <<= 1
    return row


def rec(ax, m, depth=0.0, hz=0.0, fade=0):
    return ax.DelayRec(m, int(round(depth * 65536.0)), int(round(hz / 48000.0 * 2.0 ** 32)), fade, 0.6, 0.2, 0.5, 1.0, 0)


def delay_pool(ax, model, kind):
    """make_pool's pool without buses; kind: never | off | long | short | mod | fade"""
    pool = make_pool(ax, model, 0, 0)
    if kind != "never":
        pool.set_delays(True, CAPACITY)
    if kind == "long":
        pool.set_delay_rec(rec(ax, 300))
    if kind == "short":
        pool.set_delay_rec(rec(ax, 64))
    if kind in ("mod", "fade"):
        pool.set_delay_rec(rec(ax, 300, 20.0, 3.0, FADE))
    return pool


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--warmup", type=int, default=100)
    ap.add_argument("--legs", type=int, default=3)
    ap.add_argument("--calls", type=int, default=300)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--only", default=None, choices=("stage", "long", "short", "fade", "one", "never"))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stream_delay.txt"))
    ap.add_argument("--no-write", action="store_true")
    a = ap.parse_args()
    import torch
    ax = importlib.import_module("aidadsp-lv2_amd")
    W = ax.workloads
    d = tempfile.mkdtemp(prefix="delay_bench_")
    try:
        model = ax.Model(W.write_model(W.make_model("lstm", 32, 1, seed=32), os.path.join(d, "lstm32.json")))
    finally:
        shutil.rmtree(d, ignore_errors=True)                    # (the model is loaded: the file has served)
    s = torch.cuda.Stream()
    x = torch.from_numpy(W.signal(S, N, seed=5)).cuda()
    y = torch.empty_like(x)

    def leg(pool):
        return timed(torch, s, a.steps, a.warmup, lambda: pool.process_device(x.data_ptr(), y.data_ptr(), N, s.cuda_stream))

    if a.only == "never":                                       # a child of the parent comparison: one JSON line
        pool = make_pool(ax, model, 0, 0)
        print(json.dumps({"lib": ax.lib_path(), "kernel": pool.kernel_name, "us": [leg(pool) for _ in range(a.legs)]}))
        pool.close()
        return

    lines = ["The stream delays (aidax_pool_set_delays, k_delay): tools/delay_bench.py on an MI355X.",
             f"library {os.path.relpath(ax.lib_path(), ROOT)}; {a.legs} legs per case, alternating in one process; {a.steps} blocks per leg after {a.warmup} of warm-up, "
             f"{a.calls} round trips per host leg; delay capacity {CAPACITY} frames", ""]

    if a.only in (None, "stage", "long", "short", "fade"):
        cases = [("never enabled", "never"), ("on, every delay off", "off"), ("every delay on, m 300 (1 chunk)", "long"), ("every delay on, m 64 (4 chunks)", "short"),
                 ("m 300, depth 20 at 3 Hz", "mod"), ("the same, a crossfade in progress", "fade")]
        if a.only in ("long", "short", "fade"):
            cases = [c for c in cases if c[1] == a.only]
        pools = [delay_pool(ax, model, kind) for _, kind in cases]
        legs = [[] for _ in cases]
        for k in range(a.legs):
            for i, (pool, (_, kind)) in enumerate(zip(pools, cases)):
                if kind == "fade":                              # another delay ahead of every leg: the fade it starts outlasts the leg
                    pool.set_delay_rec(rec(ax, 400 if k % 2 == 0 else 300, 20.0, 3.0, FADE))
                legs[i].append(leg(pool))
        lines.append(f"stage: {S} streams x LSTM-32 x {N} frames, no buses, aidax_pool_process_device, device events ({pools[0].kernel_name}), us per block")
        base = float(np.median(legs[0])) if cases[0][1] == "never" else None
        for (name, kind), v in zip(cases, legs):
            extra = "" if base is None or kind == "never" else f"   adds {np.median(v) - base:6.2f} us ({100.0 * (np.median(v) - base) / base:.1f} %)"
            lines.append(f"   {name:36s} " + fmt(v) + extra)
        for pool, (_, kind) in zip(pools, cases):
            if kind == "fade":
                st = pool.read_delays()
                lines.append(f"   (after the run the fading pool's lines stand at frame {int(st['pos'][0])}, {int((st['fade_left'] > 0).sum())} of {S} in a fade, {int(st['fade_left'][0])} frames of it left)")
        lines.append(f"   (k_delay reads and writes the pass's block, {S * N * 4 / 1e6:.2f} MB each way, writes {S * N * 4 / 1e6:.2f} MB into the ring rows and reads three taps per frame out "
                     f"of them, six while a fade runs, a workgroup per stream; a ring row is {ring_row(CAPACITY, N)} floats at this capacity)")
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
        lines.append("parent: the stage never enabled, this build against a build of the parent commit, alternating child processes (parent, this, parent, this), us per block")
        for who in ("parent", "this"):
            v = [u for r in runs[who] for u in r["us"]]
            lines.append(f"   {who:7s} ({runs[who][0]['kernel']}) " + fmt(v))
        p = [u for r in runs["parent"] for u in r["us"]]
        t = [u for r in runs["this"] for u in r["us"]]
        inside = min(p) <= np.median(t) <= max(p)
        lines.append(f"   this build's median {np.median(t):.2f} lies {'inside' if inside else 'OUTSIDE'} the parent's range {min(p):.2f} .. {max(p):.2f}")
        lines.append("")

    if a.only in (None, "one"):
        lv2 = os.path.join(ROOT, "tests", "golden", "models", "tw40_california_clean_deerinkstudios.json")
        lines.append("one stream x LSTM-12 (the bundled model), blocking aidax_pool_process round trip on the host clock, us")
        for n in (64, 256):
            pool = ax.Pool(1, n)
            pool.set_model(ax.Model(lv2))
            pool.set_delays(True, CAPACITY)
            blk = W.signal(1, n, seed=6)
            legs = {False: [], True: []}
            for _ in range(a.legs):
                for on in (False, True):
                    pool.set_delay_rec(rec(ax, 300, 20.0, 3.0) if on else None)
                    legs[on].append(round_trips(lambda: pool.process(blk), a.calls))
            for on in (False, True):
                p50, p99 = [v[0] for v in legs[on]], [v[1] for v in legs[on]]
                lines.append(f"   {n:3d} frames, delay {'on: ' if on else 'off:'} p50 " + fmt(p50) + "     p99 " + "  ".join(f"{v:7.2f}" for v in p99))
            lines.append(f"   {n:3d} frames: the delay adds {np.median([v[0] for v in legs[True]]) - np.median([v[0] for v in legs[False]]):.2f} us to the p50 round trip "
                         f"({pool.kernel_name}; the pass's block is pinned host memory, k_delay works on it in place and the queue writes the completion word)")
            pool.close()
        lines.append("")

    text = "\n".join(lines)
    print(text)
    if not a.no_write:
        text += trace_section(a.out)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
