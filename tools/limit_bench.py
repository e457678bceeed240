"""Cost of the bus limiters (aidax_pool_set_bus_limiting, k_bus_limit) on the shipped library: writes profiles/bus_limiter.txt.

  stage     1024 streams of the LSTM-32 amp model, 256-frame blocks, device-resident: aidax_pool_process_device back to back on one torch
            stream, device events around --steps blocks per leg. Eight pools in one process, measured in alternating legs so that all of
            them see the same clocks and the same neighbours on the box:
              64 buses x 16 entries   the stage never enabled | on, every limiter off | L = 64, H = 0 | L = 64, H = 4096
              1 bus x 1024 entries    never enabled | L = 64, H = 0
              512 buses x 2 entries   never enabled | L = 64, H = 0
            us per block each; the difference to "never enabled" on the same buses is what the k_bus_limit launch of a pass adds (kernel
            time and the gaps around it). Every limiter has its ceiling at --ceiling-db; how many frames it limited is printed next to it.
  parent    with --parent-lib FILE (a build of the parent commit's library): 64 buses x 16 entries, the stage never enabled, in child
            processes that alternate between that library and this one (AIDAX_LIB), --legs legs each. "A pool that does not ask for the
            stage pays nothing" is the claim that this build's figures sit inside the parent's own run-to-run spread, which is measured
            here, not assumed.

k_bus_limit's own time, launch by launch, is not measured in here: run the tool under `rocprofv3 --kernel-trace --stats` with --no-write
--only hold for that (a run of its own: tracing slows the host side), and write what it shows into the profile by hand, from a line that
starts with "kernel trace" to the file's end. A run that writes the profile carries that section over from the file it replaces.

    python3 tools/limit_bench.py [--steps 1000] [--warmup 100] [--legs 3] [--parent-lib FILE] [--only stage|hold|never] [--ceiling-db -30] [--out FILE] [--no-write]
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
from tools.mix_bench import S, N, fmt, make_pool, timed, trace_section  # noqa: E402


def limited_pool(ax, model, buses, per_bus, stage, rec, ceiling_db):
    """make_pool's pool; stage: the limiter stage enabled with the full capacities; rec: (L, H) for every bus's limiter, None: all off"""
    pool = make_pool(ax, model, buses, per_bus)
    if stage:
        pool.set_bus_limiting(True, ax.BUS_LOOKAHEAD_MAX, ax.BUS_HOLD_MAX)
        if rec is not None:
            pool.set_bus_limiter(ax.BusLimitParams(ceiling_db, rec[0] * 1000.0 / 48000.0, rec[1] * 1000.0 / 48000.0))
            assert pool.bus_limiter(0)[1:] == (True, rec[0])
    return pool


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--warmup", type=int, default=100)
    ap.add_argument("--legs", type=int, default=3)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--only", default=None, choices=("stage", "hold", "never"))
    ap.add_argument("--ceiling-db", type=float, default=-30.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bus_limiter.txt"))
    ap.add_argument("--no-write", action="store_true")
    a = ap.parse_args()
    import torch
    ax = importlib.import_module("aidadsp-lv2_amd")
    W = ax.workloads
    d = tempfile.mkdtemp(prefix="limit_bench_")
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

    lines = ["The bus limiters (aidax_pool_set_bus_limiting, k_bus_limit): tools/limit_bench.py on an MI355X.",
             f"library {os.path.relpath(ax.lib_path(), ROOT)}; {a.legs} legs per case, alternating in one process; {a.steps} blocks per leg after {a.warmup} of warm-up; "
             f"every limiter's ceiling at {a.ceiling_db:g} dB", ""]

    if a.only in (None, "stage", "hold"):
        # (name, buses, entries per bus, stage enabled?, (L, H) or None, the case it is compared with)
        cases = [("64 x 16   never enabled", 64, 16, False, None, None), ("64 x 16   on, limiters off", 64, 16, True, None, 0),
                 ("64 x 16   L 64, H 0", 64, 16, True, (64, 0), 0), ("64 x 16   L 64, H 4096", 64, 16, True, (64, 4096), 0),
                 ("1 x 1024  never enabled", 1, 1024, False, None, None), ("1 x 1024  L 64, H 0", 1, 1024, True, (64, 0), 4),
                 ("512 x 2   never enabled", 512, 2, False, None, None), ("512 x 2   L 64, H 0", 512, 2, True, (64, 0), 6)]
        if a.only == "hold":
            cases = [cases[3][:5] + (None,)]
        pools = [limited_pool(ax, model, b, n, stage, rec, a.ceiling_db) for _, b, n, stage, rec, _ in cases]
        legs = [[] for _ in cases]
        for _ in range(a.legs):
            for k, pool in enumerate(pools):
                legs[k].append(leg(pool))
        lines.append(f"stage: {S} streams x LSTM-32 x {N} frames, aidax_pool_process_device, device events ({pools[0].kernel_name}), us per block")
        for k, ((name, b, n, stage, rec, base), v) in enumerate(zip(cases, legs)):
            extra = ""
            if base is not None:
                ref = float(np.median(legs[base]))
                extra = f"   k_bus_limit's launch adds {np.median(v) - ref:6.2f} us ({100.0 * (np.median(v) - ref) / ref:.1f} %)"
            if rec is not None:
                m = pools[k].read_bus_meters()
                extra += f"   [{100.0 * m['limited'].sum() / max(1, m['frames'].sum()):.0f} % of the frames limited, lowest gain {m['min_gain'].min():.3f}]"
            lines.append(f"   {name:27s} " + fmt(v) + extra)
        lines.append(f"   (k_bus_limit reads and writes buses x {N * 4} B per pass, a workgroup per bus; its ring row is 8192 floats per bus at these capacities)")
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
