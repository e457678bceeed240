"""What tests/test_gpu_rate.py and tests/test_gpu_rate_wide.py share: noise, a resampler with its spec, the ragged feeding loop, and the
adapter next to its hand composition. No assertion about the arithmetic lives here."""
import importlib

import numpy as np

from tests import modelgen, rateref as rr

ax = importlib.import_module("aidadsp-lv2_amd")


def noise(S, n, seed):
    return np.random.default_rng(seed).uniform(-1.0, 1.0, (S, n)).astype(np.float32)


def stage(S, ri, ro, d_in, d_out, max_in):
    rs = ax.Resampler(S, float(ri), float(ro), d_in, d_out, max_in)
    rs.spec = (ri, ro, d_in, d_out)
    return rs


def feed(rs, x, cuts, reset=None, cap=None, at=0, taken=0):
    """x through the resampler in calls of `cuts` frames, every ready output taken after each call; reset = (stream, frames received
    when it happens). Calls alternate between append-then-ask (two launches, the first without outputs) and one call for both.
    cap: no call takes more than `cap` outputs (the blocking call's limit); what is ready beyond it goes in further calls without frames.
    at, taken: the frames the stage has received and the outputs it has given before (x is the whole input)."""
    got = []
    for k, n in enumerate(cuts):
        if reset is not None and at == reset[1]:
            rs.reset_stream(reset[0])
        blk = np.ascontiguousarray(x[:, at:at + n])
        at += n
        ready = rr.ready(at, *rs.spec) - taken - sum(g.shape[1] for g in got)
        if cap is not None:
            first = 0 if k % 2 == 0 else min(ready, cap)
            got.append(rs.process(blk, first))
            for a in range(first, ready, cap):
                got.append(rs.process(blk[:, :0], min(cap, ready - a)))
        elif k % 2 == 0:
            got.append(rs.process(blk))
        else:
            got.append(rs.process(blk, ready))
        assert rs.ready == 0
    return np.concatenate(got, axis=1)


def pool(model, S, max_frames, controls, ir=None, rate=48000):
    p = ax.Pool(S, max_frames, float(rate))
    p.set_model(model)
    p.set_controls(controls)
    if ir is not None:
        p.set_ir(ir)
    return p


def adapter_and_its_parts(model, ir, blocks, S=5, host=44100, pool_rate=48000, max_frames=256, pool_max=288):
    """(adapter's output, hand composition's output, the adapter's pool and adapter, the twin pool): the model with the EQ and the gains
    on, S streams at the host's rate around pools at theirs, the host blocks as given (n = 1 and n = 0 among them), everything on one
    torch stream"""
    import torch
    ctl = ax.default_controls(eq_bypass=0.0, bass_boost_db=4.0, mid_boost_db=-3.0, treble_boost_db=2.5, pregain_db=3.0, master_db=-2.0)
    p1, p2 = pool(model, S, pool_max, ctl, ir, pool_rate), pool(model, S, pool_max, ctl, ir, pool_rate)
    ad = ax.RateAdapter(p1, float(host), max_frames)
    H_A, d_B = rr.delays(host, pool_rate)
    A = ax.Resampler(S, float(host), float(pool_rate), H_A, 0, max_frames)
    B = ax.Resampler(S, float(pool_rate), float(host), 0, d_B, pool_max)
    x = modelgen.signal(S, sum(blocks), seed=77)
    s = torch.cuda.Stream()
    got, want, at = [], [], 0
    with torch.cuda.stream(s):
        for n, m in zip(blocks, rr.pool_frames(blocks, host, pool_rate)):
            d_x = torch.from_numpy(np.ascontiguousarray(x[:, at:at + n])).cuda()
            at += n
            y1, y2 = torch.empty((S, n), dtype=torch.float32, device="cuda"), torch.empty((S, n), dtype=torch.float32, device="cuda")
            ya, yb = torch.empty((S, m), dtype=torch.float32, device="cuda"), torch.empty((S, m), dtype=torch.float32, device="cuda")
            ad.process_device(d_x.data_ptr() if n else 0, y1.data_ptr() if n else 0, n, s.cuda_stream)
            if n == 0:
                p2.process_device(0, 0, 0, s.cuda_stream)                   # the pre-run, and nothing else
            else:
                A.process_device(d_x.data_ptr(), n, ya.data_ptr() if m else 0, m, s.cuda_stream)
                p2.process_device(ya.data_ptr() if m else 0, yb.data_ptr() if m else 0, m, s.cuda_stream)
                B.process_device(yb.data_ptr() if m else 0, m, y2.data_ptr(), n, s.cuda_stream)
            s.synchronize()
            got.append(y1.cpu().numpy())
            want.append(y2.cpu().numpy())
    A.close()
    B.close()
    return np.concatenate(got, axis=1), np.concatenate(want, axis=1), p1, ad, p2
