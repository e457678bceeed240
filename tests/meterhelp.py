"""What the stream-meter tests share: the numpy record of the blocks a test handed in and got back, and its comparison with
aidax_pool_read_meters. The reference is the blocks themselves, not the oracle: the meters' claim is that the records describe them."""
import math

import numpy as np

EXACT = ("frames", "passes", "in_nonfinite", "out_nonfinite", "out_over", "in_peak", "out_peak")


class Running:
    """per stream: the exact counts and peaks, and every finite sample's fp64 square (an fp32 squared is exact in fp64) for math.fsum"""

    def __init__(self, S):
        self.S = S
        self.n = {k: np.zeros(S, np.uint64) for k in EXACT[:5]}
        self.peak = {k: np.zeros(S, np.float32) for k in ("in", "out")}
        self.sq = {k: [[] for _ in range(S)] for k in ("in", "out")}

    def clear(self, streams):
        """what aidax_pool_read_meters(..., clear) does to these streams' records"""
        for s in streams:
            for k in self.n:
                self.n[k][s] = 0
            for k in ("in", "out"):
                self.peak[k][s] = 0
                self.sq[k][s] = []

    def add(self, x, y):
        """one metered pass of n_frames > 0: x the block handed in, y the block returned"""
        assert x.shape == y.shape and x.shape[0] == self.S and x.shape[1] > 0 and x.dtype == y.dtype == np.float32
        self.n["frames"] += np.uint64(x.shape[1])
        self.n["passes"] += np.uint64(1)
        for side, blk in (("in", x), ("out", y)):
            fin = np.isfinite(blk)
            self.n[side + "_nonfinite"] += (~fin).sum(axis=1).astype(np.uint64)
            for s in range(self.S):
                v = blk[s][fin[s]]
                if v.size:
                    self.peak[side][s] = max(self.peak[side][s], np.abs(v).max())
                    self.sq[side][s].append(v.astype(np.float64) ** 2)
        self.n["out_over"] += (np.isfinite(y) & (np.abs(y) > np.float32(1.0))).sum(axis=1).astype(np.uint64)

    def energy(self, side, s):
        return math.fsum(np.concatenate(self.sq[side][s])) if self.sq[side][s] else 0.0

    def check(self, rec, first=0, what=""):
        """rec: read_meters(first, len(rec)). Counts, frames and peaks exact; an energy within frames x 2^-52 relative of the exact sum
        (sequential fp64 addition of n non-negative terms is within (n - 1) 2^-53 relative, whatever the order), 0 where that is 0."""
        for i, r in enumerate(rec):
            s = first + i
            for k in EXACT[:5]:
                assert int(r[k]) == int(self.n[k][s]), (what, s, k, int(r[k]), int(self.n[k][s]))
            for side in ("in", "out"):
                got, want = r[side + "_peak"], self.peak[side][s]
                assert got.dtype == np.float32 and got == want, (what, s, side + "_peak", got, want)
                got, exact = float(r[side + "_energy"]), self.energy(side, s)
                if exact == 0.0:
                    assert got == 0.0, (what, s, side + "_energy", got)
                else:
                    rel = abs(got - exact) / exact
                    assert rel <= int(self.n["frames"][s]) * 2.0 ** -52, (what, s, side + "_energy", got, exact, rel)
