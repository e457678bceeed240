"""Cost of the model bank (aidax_pool_set_model_slot / aidax_pool_assign_model, k_*_pipe_bank) on the library AIDAX_LIB names (default:
the shipped one): one JSON line per run. One process, one GPU; run it once per library to put two builds side by side.

  pool_model    S streams of the amp model x n-frame blocks, device-resident, aidax_pool_process_device back to back on one torch
                stream, timed with torch events over --steps blocks: us per block and the kernel's name, no stream on a slot (what
                the parent commit runs; with AIDAX_PIPE4=0 on the test-hooks build that is k_*_pipe)
  bank          the same pool with K distinct models in slots 0 .. K-1 and every stream assigned, once in contiguous runs of streams
                and once round-robin (--models K,...): us per block of k_*_pipe_bank
  assign        one aidax_pool_assign_model with AIDAX_START_WARMUP between two passes: us from an event in front of the call to the end
                of the next pass, minus a plain pass timed the same way (median of --calls)

A library without the bank (the parent commit's) gives the pool_model rows only.

    python3 tools/model_bank_bench.py [--cell lstm32] [--streams 1024] [--frames 256,128,64] [--models 1,4,16,64] [--steps 400]
                                      [--warmup 50] [--calls 40]
"""
import argparse
import importlib
import json
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def models(W, d, kind, hidden, count):
    """`count` model files of one architecture: seed k, its own gains, every fourth with in_skip"""
    out = []
    for k in range(count):
        kw = dict(in_gain=-3.0 + 0.1 * k, out_gain=2.0 - 0.05 * k)
        if k % 4 == 3:
            kw["in_skip"] = 1
        out.append(W.write_model(W.make_model(kind, hidden, 1, seed=3200 + k, **kw), os.path.join(d, f"{kind}{hidden}_{k}.json")))
    return out


def make_pool(ax, files, S, n, K=0, pattern="runs"):
    pool = ax.Pool(S, n)
    pool.set_model(ax.Model(files[0]))
    for k in range(K):
        pool.set_model_slot(k, ax.Model(files[1 + k]))
    for s in range(S if K else 0):
        pool.assign_model(s, s * K // S if pattern == "runs" else s % K, ax.START_RESET)
    return pool


def us_per_block(torch, W, pool, S, n, steps, warmup):
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
    return e0.elapsed_time(e1) * 1000.0 / steps


def assign_us(torch, ax, W, pool, S, n, calls, warmup):
    x = torch.from_numpy(W.signal(S, n, seed=5)).cuda()
    y = torch.empty_like(x)
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    t = {"plain": [], "assign": []}
    with torch.cuda.stream(s):
        for _ in range(warmup):
            pool.process_device(x.data_ptr(), y.data_ptr(), n, s.cuda_stream)
        s.synchronize()
        for i in range(calls):
            for kind in ("plain", "assign"):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(s)
                if kind == "assign":
                    pool.assign_model((17 * i) % S, i % 2, ax.START_WARMUP)
                pool.process_device(x.data_ptr(), y.data_ptr(), n, s.cuda_stream)
                e1.record(s)
                s.synchronize()
                t[kind].append(e0.elapsed_time(e1) * 1000.0)
    plain, withit = float(np.median(t["plain"])), float(np.median(t["assign"]))
    return {"plain_pass_us": round(plain, 2), "assign_and_pass_us": round(withit, 2), "assign_us": round(withit - plain, 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cell", default="lstm32", help="lstm32, lstm12, gru8, ...")
    ap.add_argument("--streams", type=int, default=1024)
    ap.add_argument("--frames", default="256", help="comma-separated block lengths")
    ap.add_argument("--models", default="1,4,16,64", help="comma-separated K: distinct models in the bank")
    ap.add_argument("--steps", type=int, default=400)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--calls", type=int, default=40)
    a = ap.parse_args()
    import torch
    ax = importlib.import_module("aidadsp-lv2_amd")
    W = ax.workloads
    kind, hidden = a.cell.rstrip("0123456789"), int(a.cell[len(a.cell.rstrip("0123456789")):])
    Ks = [int(k) for k in a.models.split(",") if k]
    has_bank = hasattr(ax.lib(), "aidax_pool_assign_model")
    d = tempfile.mkdtemp(prefix="model_bank_bench_")
    files = models(W, d, kind, hidden, 1 + (max(Ks) if Ks and has_bank else 0))
    S = a.streams
    out = {"lib": os.path.relpath(ax.lib_path(), ROOT), "pipe4_hook": os.environ.get("AIDAX_PIPE4"), "cell": a.cell, "streams": S, "steps": a.steps,
           "rows": {}}
    for n in (int(f) for f in a.frames.split(",")):
        row = {}
        pool = make_pool(ax, files, S, n)
        row["pool_model"] = {"kernel": pool.kernel_name, "us_per_block": round(us_per_block(torch, W, pool, S, n, a.steps, a.warmup), 2)}
        pool.close()
        if has_bank:
            row["bank"] = {}
            for K in Ks:
                for pattern in ("runs", "round_robin"):
                    pool = make_pool(ax, files, S, n, K, pattern)
                    name = pool.kernel_name
                    row["bank"][f"K{K}_{pattern}"] = {"kernel": name, "us_per_block": round(us_per_block(torch, W, pool, S, n, a.steps, a.warmup), 2)}
                    pool.close()
            if a.calls:
                pool = make_pool(ax, files, S, n, 2, "round_robin")
                row["assign"] = assign_us(torch, ax, W, pool, S, n, a.calls, a.warmup)
                pool.close()
        out["rows"][str(n)] = row
    print(json.dumps(out))


if __name__ == "__main__":
    main()
