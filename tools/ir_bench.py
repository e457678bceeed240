"""Cost of the cabinet IR stage (aidax_pool_set_ir, k_ir_conv) on the shipped library: one JSON line.

  cfg2          1024 streams of the LSTM-32 amp model x 256-frame blocks, device-resident, aidax_pool_process_device back to back on one
                torch stream, timed with torch events over --steps blocks: us per block without an IR and with an 8192-tap IR
  one_stream    the LV2 instance's pool (one stream, the bundled LSTM-12 model): aidax_pool_process round trip (host in, host out),
                median and p99 of --calls calls, without and with the IR, at 64 and 256 frames

  --irs K,...   per-stream IRs (aidax_pool_set_ir_slot / aidax_pool_assign_ir): cfg2 with K distinct IRs in bank slots, assigned once
                in contiguous runs of streams and once round-robin ("cfg2_bank": us per block and the stage's cost against the pool IR's),
                and the one-stream round trip with the IR in a bank slot ("one_stream_bank")

  --fade F      the IR fade (aidax_pool_set_ir_fade): cfg2's steady state with the fade length set against without ("cfg2_fade_steady":
                the launches are the same), the cost of ONE fade pass against a plain pass timed the same way (events around a single
                pass) with all 1024 streams fading (a pool-IR commit), with 16 of 1024 fading (assign_ir), and the round trip of a
                one-stream pool whose every pass is a fade pass, at 64 and 256 frames

  --taps N      the IR's length (default 8192); above 8192 every pool's IR capacity is raised to N (aidax_pool_set_ir_capacity), and the
                arithmetic floor scales with N

  --rate R      a pool at host rate R playing a 48 kHz cabinet of 8192 frames brought to R by aidax_ir_resample ("rate": the host time
                of the conversion, the taps it gives, cfg2 and the one-stream round trip with them; the capacity is raised as needed)

  --blend       the IR blend (aidax_pool_assign_ir_b / aidax_pool_set_ir_mix): cfg2 with an 8192-tap IR in slot 0 and another in slot 1,
                every stream on slot 0, and no stream, 64 of 1024 streams and all streams blended at a mix of 0.5 ("cfg2_blend": us per
                block of each, --rounds times in turn, and the medians). With --parent-lib PATH (the library of the commit before the
                blend) the unblended pool IR of that build and of this one, alternating, each in a child process of its own
                ("cfg2_vs_parent")

The IR is seeded exponentially decaying noise of 8192 taps (the length of the reference's cabinet IRs) unless --taps says otherwise. Under rocprofv3 --kernel-trace
--stats the k_ir_conv / k_ir_reduce / k_ir_append rows are the stage's kernels alone.

    python3 tools/ir_bench.py [--steps 400] [--warmup 50] [--calls 400] [--irs 1,4,16,64] [--fade 256] [--taps 65536] [--rate 96000]
                               [--blend [--rounds 5] [--parent-lib PATH]]
"""
import argparse
import importlib
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FLOOR_US = 10.5          # cfg2 at 8192 taps: 2.15e9 MACs as six bf16 products on 16x16x32 MFMAs at 16 cycles per SIMD, 2.4 GHz
TAPS = 8192              # --taps: the length of cabinet_ir(), and above 8192 the capacity every pool here is given
IR = None                # --rate: the taps every pool here plays instead of cabinet_ir()
SR = 48000.0             # ... and the pools' host rate


def cabinet_ir(L=None, seed=8192):
    if IR is not None:
        return IR
    L = L or TAPS
    rng = np.random.default_rng(seed)
    t = np.arange(L)
    return (rng.standard_normal(L) * np.exp(-t / (L / 6.0)) * 0.05).astype(np.float32)


def new_pool(ax, S, n):
    pool = ax.Pool(S, n, SR)
    if TAPS > 8192:
        pool.set_ir_capacity(TAPS)
    return pool


def load_bank(pool, S, K, pattern):
    """K distinct IRs in bank slots 0 .. K-1, stream s on slot s * K // S (runs) or s % K (round_robin)"""
    for k in range(K):
        pool.set_ir_slot(k, cabinet_ir(seed=8192 + k))
    for s in range(S):
        pool.assign_ir(s, s * K // S if pattern == "runs" else s % K)


def cfg2_us(ax, W, torch, path, with_ir, steps, warmup, bank=None, fade=0, blend=None):
    S, n = 1024, 256
    pool = new_pool(ax, S, n)
    pool.set_model(ax.Model(path))
    if fade:
        pool.set_ir_fade(fade)
    if with_ir:
        pool.set_ir(cabinet_ir())
    if bank:
        load_bank(pool, S, *bank)
    if blend is not None:
        # two IRs in the bank, every stream through slot 0 and every (S // blend)-th one half way over to slot 1
        load_bank(pool, S, 1, "runs")
        pool.set_ir_slot(1, cabinet_ir(seed=8193))
        pool.assign_ir_b(ax.ALL_STREAMS, 1)
        for k in range(blend):
            pool.set_ir_mix(k * (S // blend), 0.5, 0)
    x = torch.from_numpy(W.signal(S, n, seed=5)).cuda()
    y = torch.empty_like(x)
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        for _ in range(warmup):
            pool.process_device(x.data_ptr(), y.data_ptr(), n, s.cuda_stream)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(s)
        for _ in range(steps):
            pool.process_device(x.data_ptr(), y.data_ptr(), n, s.cuda_stream)
        e1.record(s)
    s.synchronize()
    us = e0.elapsed_time(e1) * 1000.0 / steps
    pool.close()
    return us


def cfg2_fade_pass(ax, W, torch, path, fade, reps, warmup, which):
    """us of single passes, each between two events: (plain passes, fade passes). which: "commit" (a pool-IR commit before every fade
    pass: all 1024 streams fade, 8192 taps on both sides) or "assign" (16 streams moved between the pool IR and a slot)"""
    S, n = 1024, 256
    pool = new_pool(ax, S, n)
    pool.set_model(ax.Model(path))
    pool.set_ir_fade(fade)
    pool.set_ir(cabinet_ir())
    pool.set_ir_slot(0, cabinet_ir(seed=1))
    staged = [pool.prepare_ir(cabinet_ir(seed=100 + i)) for i in range(reps)] if which == "commit" else []
    x = torch.from_numpy(W.signal(S, n, seed=5)).cuda()
    y = torch.empty_like(x)
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    times = {"plain": [], "fade": []}
    with torch.cuda.stream(s):
        for _ in range(warmup):
            pool.process_device(x.data_ptr(), y.data_ptr(), n, s.cuda_stream)
        s.synchronize()
        for i in range(reps):
            for kind in ("plain", "fade"):
                if kind == "fade" and which == "commit":
                    pool.commit_ir(staged[i])
                elif kind == "fade":
                    for k in range(16):
                        pool.assign_ir(64 * k, 0 if i % 2 == 0 else ax.IR_POOL)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(s)
                pool.process_device(x.data_ptr(), y.data_ptr(), n, s.cuda_stream)
                e1.record(s)
                s.synchronize()
                times[kind].append(e0.elapsed_time(e1) * 1000.0)
    for sg in staged:
        pool.staged_free(sg)
    pool.close()
    return {k: round(float(np.median(v)), 2) for k, v in times.items()}


def one_stream_fade(ax, W, path, frames, calls, fade):
    """aidax_pool_process round trip of a one-stream pool: plain passes, then passes that each follow an assign_ir (every one a fade pass)"""
    pool = new_pool(ax, 1, frames)
    pool.set_model(ax.Model(path))
    pool.set_ir_fade(fade)
    pool.set_ir(cabinet_ir())
    pool.set_ir_slot(0, cabinet_ir(seed=1))
    x = np.ascontiguousarray(W.signal(1, frames, seed=6))
    for _ in range(50):
        pool.process(x)
    out = {}
    for kind in ("plain", "fade"):
        t = np.empty(calls)
        for i in range(calls):
            if kind == "fade":
                pool.assign_ir(0, 0 if i % 2 == 0 else ax.IR_POOL)
            t0 = time.perf_counter()
            pool.process(x)
            t[i] = time.perf_counter() - t0
        out[kind] = {"p50_us": round(float(np.percentile(t, 50)) * 1e6, 2), "p99_us": round(float(np.percentile(t, 99)) * 1e6, 2)}
    pool.close()
    return out


def one_stream(ax, W, path, with_ir, frames, calls, bank=False):
    pool = new_pool(ax, 1, frames)
    pool.set_model(ax.Model(path))
    if with_ir:
        pool.set_ir(cabinet_ir())
    if bank:
        load_bank(pool, 1, 1, "runs")
    x = np.ascontiguousarray(W.signal(1, frames, seed=6))
    for _ in range(50):
        pool.process(x)
    t = np.empty(calls)
    for i in range(calls):
        t0 = time.perf_counter()
        pool.process(x)
        t[i] = time.perf_counter() - t0
    pool.close()
    return {"p50_us": round(float(np.percentile(t, 50)) * 1e6, 2), "p99_us": round(float(np.percentile(t, 99)) * 1e6, 2)}


def blend_report(ax, W, torch, path, a):
    rounds = {"none": [], "64_of_1024": [], "all_1024": []}
    dry = cfg2_us(ax, W, torch, path, False, a.steps, a.warmup)
    for _ in range(a.rounds):
        for name, k in (("none", 0), ("64_of_1024", 64), ("all_1024", 1024)):
            rounds[name].append(round(cfg2_us(ax, W, torch, path, False, a.steps, a.warmup, blend=k), 2))
    med = {k: round(float(np.median(v)), 2) for k, v in rounds.items()}
    stage = med["none"] - dry
    return {"us_per_block_no_ir": round(dry, 2), "rounds": rounds, "median_us_per_block": med, "ir_stage_us": round(stage, 2),
            "extra_us": {k: round(v - med["none"], 2) for k, v in med.items() if k != "none"},
            "all_blended_over_ir_stage": round((med["all_1024"] - dry) / stage, 3)}


def vs_parent(a):
    """cfg2 with the pool IR, no stream blended, on the parent's library and on this one in turn: every measurement a fresh process"""
    libs = {"parent": os.path.abspath(a.parent_lib), "new": os.path.join(ROOT, "aidadsp-lv2_amd", "lib", "libaidax_hip.so")}
    rounds = {k: [] for k in libs}
    for _ in range(a.rounds):
        for name, lib in libs.items():
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--steps", str(a.steps), "--warmup", str(a.warmup), "--cfg2-only"],
                               env=dict(os.environ, AIDAX_LIB=lib), capture_output=True, text=True, timeout=300, check=True)
            rounds[name].append(json.loads(r.stdout.strip().splitlines()[-1])["us_per_block_ir"])
    med = {k: round(float(np.median(v)), 2) for k, v in rounds.items()}
    return {"rounds": rounds, "median_us_per_block_ir": med, "new_minus_parent_us": round(med["new"] - med["parent"], 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=400)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--calls", type=int, default=400)
    ap.add_argument("--irs", default="", help="comma-separated K: cfg2 with K distinct IRs in bank slots (e.g. 1,4,16,64)")
    ap.add_argument("--fade", type=int, default=0, help="fade length in frames: the IR fade's steady state and the cost of one fade pass")
    ap.add_argument("--taps", type=int, default=8192, help="IR length; above 8192 the pools' IR capacity is raised to it")
    ap.add_argument("--rate", type=int, default=0, help="host rate of the pools: a 48 kHz cabinet of 8192 frames converted to it")
    ap.add_argument("--blend", action="store_true", help="the IR blend: cfg2 with no, 64 and all 1024 streams blended, in turn")
    ap.add_argument("--rounds", type=int, default=5, help="--blend: how often each variant is measured")
    ap.add_argument("--parent-lib", default="", help="--blend: the library of the commit before the blend, for the unblended stage against it")
    ap.add_argument("--cfg2-only", action="store_true", help="(what --parent-lib runs in a child: cfg2 with the pool IR, one JSON line)")
    a = ap.parse_args()
    if a.blend and a.parent_lib:
        against = vs_parent(a)                      # (ahead of this process's own use of the device)
    import torch
    ax = importlib.import_module("aidadsp-lv2_amd")
    global TAPS, IR, SR
    TAPS = a.taps
    rate = None
    if a.rate:
        src = cabinet_ir(8192)
        t = []
        for _ in range(5):
            t0 = time.perf_counter()
            taps, n_full = ax.resample_ir(src, 48000, a.rate)
            t.append(time.perf_counter() - t0)
        IR, SR, TAPS = taps, float(a.rate), max(8192, int(n_full))
        rate = {"host_rate": a.rate, "taps": int(n_full), "resample_ms_best_of_5": round(min(t) * 1e3, 3)}
    W = ax.workloads
    d = tempfile.mkdtemp(prefix="ir_bench_")
    cfg2 = W.write_model(W.make_model("lstm", 32, 1, seed=32), os.path.join(d, "lstm32.json"))
    lv2 = os.path.join(ROOT, "tests", "golden", "models", "tw40_california_clean_deerinkstudios.json")
    out = {"lib": os.path.relpath(ax.lib_path(), ROOT), "ir_taps": int(cabinet_ir().size), "steps": a.steps}
    if a.cfg2_only:
        print(json.dumps({"lib": out["lib"], "us_per_block_ir": round(cfg2_us(ax, W, torch, cfg2, True, a.steps, a.warmup), 2)}))
        return
    if a.blend:
        out["cfg2_blend"] = blend_report(ax, W, torch, cfg2, a)
        if a.parent_lib:
            out["cfg2_vs_parent"] = against
        print(json.dumps(out))
        return
    if rate:
        out["rate"] = rate
    floor_us = FLOOR_US * cabinet_ir().size / 8192
    dry = cfg2_us(ax, W, torch, cfg2, False, a.steps, a.warmup)
    wet = cfg2_us(ax, W, torch, cfg2, True, a.steps, a.warmup)
    out["cfg2"] = {"us_per_block_no_ir": round(dry, 2), "us_per_block_ir": round(wet, 2), "ir_stage_us": round(wet - dry, 2),
                   "ir_stage_over_floor": round((wet - dry) / floor_us, 2), "floor_us": round(floor_us, 2)}
    out["one_stream"] = {}
    for frames in (64, 256):
        out["one_stream"][str(frames)] = {"no_ir": one_stream(ax, W, lv2, False, frames, a.calls),
                                          "ir": one_stream(ax, W, lv2, True, frames, a.calls)}
    if a.irs:
        out["cfg2_bank"] = {}
        for K in (int(k) for k in a.irs.split(",")):
            for pattern in ("runs", "round_robin"):
                us = cfg2_us(ax, W, torch, cfg2, False, a.steps, a.warmup, bank=(K, pattern))
                out["cfg2_bank"][f"K{K}_{pattern}"] = {"us_per_block": round(us, 2), "ir_stage_us": round(us - dry, 2),
                                                        "over_pool_ir_stage": round((us - dry) / (wet - dry), 3)}
        out["one_stream_bank"] = {str(f): one_stream(ax, W, lv2, False, f, a.calls, bank=True) for f in (64, 256)}
    if a.fade:
        steady = cfg2_us(ax, W, torch, cfg2, True, a.steps, a.warmup, fade=a.fade)
        again = cfg2_us(ax, W, torch, cfg2, True, a.steps, a.warmup)
        out["cfg2_fade_steady"] = {"fade_frames": a.fade, "us_per_block_fade_set": round(steady, 2), "us_per_block_fade_0": round(wet, 2),
                                   "us_per_block_fade_0_again": round(again, 2), "ir_stage_us_fade_set": round(steady - dry, 2)}
        out["cfg2_fade_pass"] = {}
        for which, name in (("commit", "all_1024_fading"), ("assign", "16_of_1024_fading")):
            t = cfg2_fade_pass(ax, W, torch, cfg2, a.fade, 40, a.warmup, which)
            out["cfg2_fade_pass"][name] = {"plain_pass_us": t["plain"], "fade_pass_us": t["fade"], "extra_us": round(t["fade"] - t["plain"], 2),
                                           "extra_over_ir_stage": round((t["fade"] - t["plain"]) / (wet - dry), 3)}
        out["one_stream_fade"] = {str(f): one_stream_fade(ax, W, lv2, f, a.calls, min(a.fade, f)) for f in (64, 256)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
