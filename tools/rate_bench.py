"""Cost of the rate adapter (aidax_rate_create, k_resample) on the shipped library: one JSON line.

  cfg2          1024 streams of the LSTM-32 amp model at 48 kHz behind an adapter at 44.1 kHz: 256-frame host blocks, device-resident,
                aidax_rate_process_device back to back on one torch stream, timed with torch events over --steps blocks, against the
                same pool fed 279-frame blocks directly (the bare pass: what the pool costs per host block without the adapter).
                Each stage alone, a bare aidax_resampler with the adapter's delays fed the same blocks the same way (A: 256 in, 278 or
                279 out; B: 279 in, 256 out), beside the launch floor: the stage's smallest launch, one workgroup appending one frame.
  one_stream    the LV2 instance's case, one stream of the bundled LSTM-12 model at 64 host frames: aidax_rate_process round trip
                (host in, host out), median and p99 of --calls calls, against aidax_pool_process of the same pool at 70 frames; and
                the stages and the floor as above, device-resident.

The stages are launch- and latency-bound (about 36 MFLOP and 2 MB per cfg2 block): read them against the floor, not against a roofline.

    python3 tools/rate_bench.py [--steps 400] [--warmup 50] [--calls 400] [--host-rate 44100]
"""
import argparse
import importlib
import json
import os
import sys
import tempfile
import time
from math import gcd

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

POOL_RATE = 48000


def timed(torch, s, steps, warmup, call):
    """us per call of `call(k)`, issued back to back on torch stream s between two events"""
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        for k in range(warmup):
            call(k)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(s)
        for k in range(warmup, warmup + steps):
            call(k)
        e1.record(s)
    s.synchronize()
    return e0.elapsed_time(e1) * 1000.0 / steps


def device_case(ax, W, torch, path, S, n, host, steps, warmup):
    g = gcd(host, POOL_RATE)
    La, Ma = POOL_RATE // g, host // g                                   # pool_rate / host_rate in lowest terms
    m_max = -(-n * La // Ma)
    s = torch.cuda.Stream()
    x = torch.from_numpy(W.signal(S, n, seed=5)).cuda()
    y = torch.empty_like(x)
    xp = torch.from_numpy(W.signal(S, m_max, seed=6)).cuda()
    yp = torch.empty_like(xp)
    model = ax.Model(path)
    out = {"streams": S, "host_frames": n, "pool_frames": m_max}

    pool = ax.Pool(S, m_max, float(POOL_RATE))
    pool.set_model(model)
    out["bare_pass_us"] = round(timed(torch, s, steps, warmup, lambda k: pool.process_device(xp.data_ptr(), yp.data_ptr(), m_max, s.cuda_stream)), 2)
    ad = ax.RateAdapter(pool, float(host), n)
    out["adapter_us"] = round(timed(torch, s, steps, warmup, lambda k: ad.process_device(x.data_ptr(), y.data_ptr(), n, s.cuda_stream)), 2)
    out["latency_frames"] = ad.latency_frames
    ad.close()
    pool.close()

    H_A = (ax.resampler_row(float(host), float(POOL_RATE), 0).size - 1) // 2          # stage A: d_in = H_A; stage B: d_out = d_B
    d_B = ax.rate_latency(float(host), float(POOL_RATE)) - H_A
    m_of = lambda k: (k + 1) * n * La // Ma - k * n * La // Ma
    A = ax.Resampler(S, float(host), float(POOL_RATE), H_A, 0, n)
    out["stage_a_us"] = round(timed(torch, s, steps, warmup, lambda k: A.process_device(x.data_ptr(), n, yp.data_ptr(), m_of(k), s.cuda_stream)), 2)
    A.close()
    B = ax.Resampler(S, float(POOL_RATE), float(host), 0, d_B, m_max)
    out["stage_b_us"] = round(timed(torch, s, steps, warmup, lambda k: B.process_device(xp.data_ptr(), m_of(k), y.data_ptr(), n, s.cuda_stream)), 2)
    B.close()
    # the floor: one workgroup, one frame appended, no output (a fresh stage per 2^20 calls would be needed beyond; steps stay far below)
    F = ax.Resampler(1, float(POOL_RATE), float(POOL_RATE), 0, 0, 1)
    taken = [0]

    def floor_call(k):
        # take the ready outputs now and then, so that the ring never refuses the append
        if F.ready >= 16:
            F.process_device(0, 0, y.data_ptr(), 16, s.cuda_stream)
            taken[0] += k >= warmup
        F.process_device(x.data_ptr(), 1, 0, 0, s.cuda_stream)
    us = timed(torch, s, steps, warmup, floor_call)
    out["launch_floor_us"] = round(us * steps / (steps + taken[0]), 2)
    F.close()
    out["stages_over_bare_pass"] = round((out["adapter_us"] - out["bare_pass_us"]) / out["bare_pass_us"], 3)
    return out


def round_trip(fn, x, calls):
    for _ in range(50):
        fn(x)
    t = np.empty(calls)
    for i in range(calls):
        t0 = time.perf_counter()
        fn(x)
        t[i] = time.perf_counter() - t0
    return {"p50_us": round(float(np.percentile(t, 50)) * 1e6, 2), "p99_us": round(float(np.percentile(t, 99)) * 1e6, 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=400)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--calls", type=int, default=400)
    ap.add_argument("--host-rate", type=int, default=44100)
    a = ap.parse_args()
    import torch
    ax = importlib.import_module("aidadsp-lv2_amd")
    W = ax.workloads
    d = tempfile.mkdtemp(prefix="rate_bench_")
    cfg2 = W.write_model(W.make_model("lstm", 32, 1, seed=32), os.path.join(d, "lstm32.json"))
    lv2 = os.path.join(ROOT, "tests", "golden", "models", "tw40_california_clean_deerinkstudios.json")
    out = {"lib": os.path.relpath(ax.lib_path(), ROOT), "host_rate": a.host_rate, "pool_rate": POOL_RATE, "steps": a.steps}
    out["cfg2"] = device_case(ax, W, torch, cfg2, 1024, 256, a.host_rate, a.steps, a.warmup)
    one = device_case(ax, W, torch, lv2, 1, 64, a.host_rate, a.steps, a.warmup)
    m = one["pool_frames"]
    pool = ax.Pool(1, m, float(POOL_RATE))
    pool.set_model(ax.Model(lv2))
    one["pool_process_round_trip"] = round_trip(pool.process, np.ascontiguousarray(W.signal(1, m, seed=6)), a.calls)
    ad = ax.RateAdapter(pool, float(a.host_rate), 64)
    one["rate_process_round_trip"] = round_trip(ad.process, np.ascontiguousarray(W.signal(1, 64, seed=6)), a.calls)
    ad.close()
    pool.close()
    out["one_stream"] = one
    print(json.dumps(out))


if __name__ == "__main__":
    main()
