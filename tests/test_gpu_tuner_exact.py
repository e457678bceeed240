"""The stream tuners bit for bit (GPU, -m gpu): k_tune on the windows of tests/tunedata.py.

Term families: sparse windows whose marks put exactly one product of a rich value (22 or 11 significant bits) on every lag 1 .. tmax + 1,
so that the true autocorrelation is an fp32 number there, every partial sum of the kernel's six term products is one too, and m[t] is
exact in fp64 in any summation order. The NSDF at those lags is then ONE correctly rounded value: the comparison is equality of bits, and
tests/test_tune_arith.py shows that a kernel which drops a product of term 1 or 2, reads one of their planes a frame off or splits the
window in two terms changes those bits on every lag. Lag 0 is the sum of the squares, no fp32 number: it keeps the project's bound.

Pick edges: windows of integers / 8 that sit on the edges of rules 5 and 6 (ties, the bar itself, tmin and tmax, a lobe open at the row's
end, lobes over chunk and tile edges); each is held to its edge on the CPU (tunedata.check_case) and to the restatement's bits here.

Also every count of lag tiles the other tests leave out, and the tightest history ring (R = W + max_frames exactly)."""
import importlib

import numpy as np
import pytest

from tests import errlog, modelgen, tunedata, tunehelp as th

pytestmark = pytest.mark.gpu
ax = importlib.import_module("aidadsp-lv2_amd")

SR = tunedata.SR
TAU = 4e-6                                      # tests/test_gpu_tuner.py's bound on the six-product arithmetic


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    p = str(tmp_path_factory.mktemp("tuner_exact") / "lstm16.json")
    modelgen.write_model(modelgen.make_model(kind="lstm", hidden=16, input_size=1, seed=5), p)
    return ax.Model(p)


def _design(**kw):
    """(the library's TunerParams, the restatement's record) of the same parameters"""
    rec = th.design(SR, **kw)
    assert rec is not None
    got = ax.tuner_design(SR, ax.tuner_params(**kw))
    assert (got.window, got.hop, got.tmin, got.tmax) == (rec["window"], rec["hop"], rec["tmin"], rec["tmax"])
    assert (np.float32(got.threshold), np.float32(got.clarity_min), np.float32(got.level_min)) == (rec["threshold"], rec["clarity_min"], rec["level_min"])
    return ax.tuner_params(**kw), rec


def _analysed(model, x, params, blocks, max_frames=1024):
    """a pool of x's streams fed x in `blocks`: (the readings, the curves)"""
    p = ax.Pool(x.shape[0], max_frames)
    p.set_model(model)
    p.set_tuning(params)
    p.set_tuner(True)
    at = 0
    for n in blocks:
        p.process(np.ascontiguousarray(x[:, at:at + n]))
        at += n
    assert at == x.shape[1]
    got = p.read_tuners()
    curves = np.stack([p.read_tuner_curve(s) for s in range(x.shape[0])])
    p.close()
    return got, curves


def _bits(v):
    return np.asarray(v, np.float32).view(np.uint32)


def _same_curve(curve, n, what, first=0):
    bad = np.flatnonzero(_bits(curve[first:]) != _bits(n[first:])) + first
    assert bad.size == 0, (what, "first lags that differ", bad[:8], curve[bad[:8]], n[bad[:8]])


def _same_reading(got, want, what, level_bits=True):
    assert int(got["lag"]) == int(want["lag"]), (what, got, want)
    for f in ("hz", "period", "clarity") + (("level",) if level_bits else ()):
        assert _bits(got[f]) == _bits(want[f]), (what, f, got, want)
    if not level_bits:
        assert abs(float(got["level"]) - float(want["level"])) <= 2.0 ** -23 * float(want["level"]), (what, got, want)


def _sparse_reference(x, r, rec):
    """the restatement on a family's window and its exact autocorrelation: (the reading, the NSDF row, lag 0 of the row in fp64)"""
    n, cW = th.nsdf(x, r, rec["tmax"])
    return th.reading(n, cW, rec), n, (2.0 * r[0]) / (cW + cW)


def _check_family(fam, got, curves, rec, what, tag):
    worst = 0.0
    for s, x in enumerate(fam["x"]):
        want, n, n0 = _sparse_reference(x, fam["r"][s], rec)
        _same_curve(curves[s], n, (what, s), first=1)
        worst = max(worst, abs(float(curves[s][0]) - n0))
        assert (int(got["frame"][s]), int(got["analyses"][s])) == (rec["window"], 1)
        _same_reading(got[s], want, (what, s), level_bits=False)
    print(f"{what}: worst |n_gpu[0] - n_fp64[0]| = {worst:.3e} (bound {TAU + 2.0 ** -23:.3e})")
    errlog.bound(worst, TAU + 2.0 ** -23, tag)


@pytest.mark.parametrize("f,W", [("A", 1024), ("B", 1024), ("C", 1024), ("C", 2048)])
def test_term_families_bit_for_bit(model, f, W):
    tmax = W // 2 - 1
    fam = tunedata.family(f, W, tmax)
    params, rec = _design(window=W, hop=1024, f_min=tunedata.f_min_for(tmax), f_max=12000.0, clarity_min=0.0)
    assert rec["tmax"] == tmax and rec["tmin"] == 4                        # rules 5 - 7 never read n[0]
    got, curves = _analysed(model, fam["x"], params, [1024] * (W // 1024))
    assert curves.shape == (fam["x"].shape[0], tmax + 2)
    _check_family(fam, got, curves, rec, f"family {f}, W = {W}", "gpu_tuner_nsdf:families_lag0")


@pytest.mark.parametrize("name", list(tunedata.DESIGNS))
def test_pick_edges_bit_for_bit(model, name):
    cases = tunedata.cases_of(name)
    params, rec = _design(**tunedata.pick_design(name))
    x = np.stack([c["x"] for c in cases])
    got, curves = _analysed(model, x, params, [1024])
    for s, c in enumerate(cases):
        want, n = tunedata.check_case(c)
        _same_curve(curves[s], n, c["name"])
        assert (int(got["frame"][s]), int(got["analyses"][s])) == (1024, 1)
        _same_reading(got[s], want, c["name"])
        assert int(got["lag"][s]) == c["lag"], c["name"]


@pytest.mark.parametrize("W,tmax,tiles", [(1024, 254, 1), (1024, 255, 2), (2048, 767, 4), (2048, 900, 4), (4096, 1279, 6), (4096, 1535, 7),
                                          (4096, 1791, 8)])
def test_every_count_of_lag_tiles(model, W, tmax, tiles):
    """1, 2 with a lone last lag, 4 (with and without one), 6, 7 and 8 lag tiles: a pattern of integers / 8 whose period is tmax (its peak
    is the last lag in range) and one window of family C at this W and tmax"""
    assert (tmax + 1) // 256 + 1 == tiles
    params, rec = _design(window=W, hop=1024, f_min=tunedata.f_min_for(tmax), f_max=12000.0, clarity_min=0.0)
    assert rec["tmax"] == tmax
    rng = np.random.default_rng([W, tmax])
    pattern = (np.tile(rng.integers(-8, 9, tmax), W // tmax + 1)[:W] / 8.0).astype(np.float32)
    fam = tunedata.family("C", W, tmax, streams=1)
    got, curves = _analysed(model, np.stack([pattern, fam["x"][0]]), params, [1024] * (W // 1024))
    assert curves.shape == (2, tmax + 2)
    want, n = th.analyse(pattern, rec, exact=True)
    assert want["lag"] == tmax
    _same_curve(curves[0], n, (W, tmax, "pattern"))
    _same_reading(got[0], want, (W, tmax, "pattern"))
    want, n, n0 = _sparse_reference(fam["x"][0], fam["r"][0], rec)
    _same_curve(curves[1], n, (W, tmax, "family C"), first=1)
    _same_reading(got[1], want, (W, tmax, "family C"), level_bits=False)
    errlog.bound(abs(float(curves[1][0]) - n0), TAU + 2.0 ** -23, "gpu_tuner_nsdf:families_lag0")
    assert [int(v) for v in got["frame"]] == [W, W] and [int(v) for v in got["analyses"]] == [1, 1]


def test_the_tight_ring(model):
    """W = 1024, max_frames = 1024, hop 1024: the ring has exactly W + max_frames = 2048 slots. Blocks of 1023, 1024 and 1024 frames give
    two analyses whose boundary lies one frame above the pass's first frame: the window reaches back to the oldest slot the pass left
    alone. Family B's rows, then the same rows one stream on, then as many frames that no window holds"""
    W, tmax = 1024, 511
    fam = tunedata.family("B", W, tmax)
    S = fam["x"].shape[0]
    params, rec = _design(window=W, hop=1024, f_min=tunedata.f_min_for(tmax), f_max=12000.0, clarity_min=0.0)
    x = np.concatenate([fam["x"], np.roll(fam["x"], 1, axis=0), np.roll(fam["x"], 2, axis=0)[:, :1023]], axis=1)
    p = ax.Pool(S, 1024)
    p.set_model(model)
    p.set_tuning(params)
    p.set_tuner(True)
    trackers = [th.Tracker(rec) for _ in range(S)]
    at, seen = 0, 0
    for n in (1023, 1024, 1024):
        blk = np.ascontiguousarray(x[:, at:at + n])
        p.process(blk)
        at += n
        fired = [tr.feed(blk[s]) for s, tr in enumerate(trackers)]
        got = p.read_tuners()
        if not any(fired):
            assert at == 1023 and not got.tobytes().strip(b"\0")
            continue
        seen += 1
        assert all(fired)
        for s, tr in enumerate(trackers):
            src = (s - (seen - 1)) % S
            assert np.array_equal(tr.window, fam["x"][src]) and (tr.frame, tr.analyses) == (1024 * seen, seen)
            want, n_row, _ = _sparse_reference(tr.window, fam["r"][src], rec)
            _same_curve(p.read_tuner_curve(s), n_row, (seen, s), first=1)
            assert (int(got["frame"][s]), int(got["analyses"][s])) == (tr.frame, tr.analyses)
            _same_reading(got[s], want, (seen, s), level_bits=False)
    p.close()
    assert seen == 2 and at == 3071
