"""Cost of the bus reverbs (aidax_pool_set_bus_reverbs, k_bus_reverb) on the shipped library: writes profiles/bus_reverb.txt.

  stage     1024 streams of the LSTM-32 amp model, 256-frame blocks, device-resident: aidax_pool_process_device back to back on one torch
            stream, device events around --steps blocks per leg. 64 buses x 16 entries, five pools in one process, measured in
            alternating legs so that all of them see the same clocks and the same neighbours on the box:
              the stage never enabled | on, every reverb off | every bus on at m_min = 64 (four chunks per block) | every bus on as
              designed at size 1 (one chunk) | no reverb, the bus limiters on at L = 64, H = 0 (k_bus_limit's launch, for scale)
            us per block each; the difference to "never enabled" is what the k_bus_reverb launch of a pass adds (kernel time and the
            gaps around it).
  parent    with --parent-lib FILE (a build of the parent commit's library): the stage never enabled, in child processes that alternate
            between that library and this one (AIDAX_LIB), --legs legs each. "A pool that does not ask for the stage pays nothing" is
            the claim that this build's figures sit inside the parent's own run-to-run spread, which is measured here, not assumed.

k_bus_reverb's own time, launch by launch, is not measured in here: run the tool under `rocprofv3 --kernel-trace --stats` with --no-write
--only small (or designed, or limit for k_bus_limit's launch next to it) for that (a run of its own: tracing slows the host side), and write what it shows into the profile by
hand, from a line that starts with "kernel trace" to the file's end. A run that writes the profile carries that section over from the
file it replaces.

    python3 tools/reverb_bench.py [--steps 1000] [--warmup 100] [--legs 3] [--parent-lib FILE] [--only stage|small|designed|limit|never] [--out FILE] [--no-write]
"""
import argparse
import ctypes as C
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
from tools.mix_bench import S, N, fmt, make_pool, timed, trace_section  # noqa: E402

CAPACITY = 4096


def small_rec(ax):
    """every delay in 64 .. 79 frames, the shortest 64: the chunk is 64 frames, four to a block of 256"""
    gq = [0.93 * (1.0 - 0.01 * i) / 8.0 ** 0.5 for i in range(8)]
    return ax.BusReverbRec((C.c_uint32 * 8)(64, 65, 67, 69, 71, 73, 77, 79), (C.c_float * 8)(*gq), 0.15, 0.5, 1.0, 0, 0)


def reverb_pool(ax, model, kind):
    """make_pool's pool of 64 buses x 16 entries; kind: never | off | small | designed | limit"""
    pool = make_pool(ax, model, 64, 16)
    if kind in ("off", "small", "designed"):
        pool.set_bus_reverbs(True, CAPACITY)
    if kind == "small":
        pool.set_bus_reverb_rec(small_rec(ax))
    if kind == "designed":
        for b in range(64):
            pool.set_bus_reverb(ax.BusReverbParams(1.5, 1.0, 0.3, 0.3, 1.0, b % 4), b)
        assert pool.bus_reverb(0)[2] and min(pool.bus_reverb(0)[1].m) >= 256
    if kind == "limit":
        pool.set_bus_limiting(True, ax.BUS_LOOKAHEAD_MAX, ax.BUS_HOLD_MAX)
        pool.set_bus_limiter(ax.BusLimitParams(-30.0, 64 * 1000.0 / 48000.0, 0.0))
    return pool


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--warmup", type=int, default=100)
    ap.add_argument("--legs", type=int, default=3)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--only", default=None, choices=("stage", "small", "designed", "limit", "never"))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bus_reverb.txt"))
    ap.add_argument("--no-write", action="store_true")
    a = ap.parse_args()
    import torch
    ax = importlib.import_module("aidadsp-lv2_amd")
    W = ax.workloads
    d = tempfile.mkdtemp(prefix="reverb_bench_")
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
        pool = make_pool(ax, model, 64, 16)
        print(json.dumps({"lib": ax.lib_path(), "kernel": pool.kernel_name, "us": [leg(pool) for _ in range(a.legs)]}))
        pool.close()
        return

    lines = ["The bus reverbs (aidax_pool_set_bus_reverbs, k_bus_reverb): tools/reverb_bench.py on an MI355X.",
             f"library {os.path.relpath(ax.lib_path(), ROOT)}; {a.legs} legs per case, alternating in one process; {a.steps} blocks per leg after {a.warmup} of warm-up; "
             f"delay capacity {CAPACITY} frames", ""]

    if a.only in (None, "stage", "small", "designed", "limit"):
        # (name, kind, the case it is compared with)
        cases = [("never enabled", "never", None), ("on, every reverb off", "off", 0), ("every bus on, m_min 64 (4 chunks)", "small", 0),
                 ("every bus on, designed, size 1 (1 chunk)", "designed", 0), ("no reverb; limiters on, L 64, H 0", "limit", 0)]
        if a.only in ("small", "designed", "limit"):
            cases = [(n, k, None) for n, k, _ in cases if k == a.only]
        pools = [reverb_pool(ax, model, kind) for _, kind, _ in cases]
        legs = [[] for _ in cases]
        for _ in range(a.legs):
            for k, pool in enumerate(pools):
                legs[k].append(leg(pool))
        lines.append(f"stage: {S} streams x LSTM-32 x {N} frames, 64 buses x 16 entries, aidax_pool_process_device, device events ({pools[0].kernel_name}), us per block")
        for (name, kind, base), v in zip(cases, legs):
            extra = ""
            if base is not None:
                ref = float(np.median(legs[base]))
                extra = f"   the {'k_bus_limit' if kind == 'limit' else 'k_bus_reverb'} launch adds {np.median(v) - ref:6.2f} us ({100.0 * (np.median(v) - ref) / ref:.1f} %)"
            lines.append(f"   {name:42s} " + fmt(v) + extra)
        lines.append(f"   (k_bus_reverb reads and writes buses x {N * 4} B of the block per pass and, per frame, 16 taps out of and 8 values into the bus's eight ring rows, "
                     f"a workgroup per bus; a ring row is {8192} floats at this capacity)")
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
        lines.append("parent: 64 buses x 16 entries, the stage never enabled, this build against a build of the parent commit, alternating child processes (parent, this, parent, this), us per block")
        for who in ("parent", "this"):
            v = [u for r in runs[who] for u in r["us"]]
            lines.append(f"   {who:7s} ({runs[who][0]['kernel']}) " + fmt(v))
        p = [u for r in runs["parent"] for u in r["us"]]
        t = [u for r in runs["this"] for u in r["us"]]
        inside = min(p) <= np.median(t) <= max(p)
        lines.append(f"   this build's median {np.median(t):.2f} lies {'inside' if inside else 'OUTSIDE'} the parent's range {min(p):.2f} .. {max(p):.2f}")
        lines.append("")

    text = "\n".join(lines)
    print(text)
    if not a.no_write:
        text += trace_section(a.out)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
