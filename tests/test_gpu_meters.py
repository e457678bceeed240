"""Stream meters on the GPU (-m gpu): the records aidax_pool_read_meters returns describe the blocks the test handed in and the blocks
the pool handed back (tests/meterhelp.py: counts, frames and peaks exact, energies within frames x 2^-52 of math.fsum over the fp64
squares), on every path a pass can take, and a metered pool's audio is an unmetered pool's bit for bit."""
import importlib

import numpy as np
import pytest

from tests import meterhelp, modelgen, rateref as rr

pytestmark = pytest.mark.gpu
ax = importlib.import_module("aidadsp-lv2_amd")

ERR_ARG, ERR_STATE = -1, -6
PLAN = [1, 3, 0, 63, 64, 65, 257, 4] * 2       # five streams: a lone wave in the second workgroup; 1, 3, 63, 65, 257: unaligned rows, every tail around the wave width


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    p = str(tmp_path_factory.mktemp("meters") / "lstm16.json")
    modelgen.write_model(modelgen.make_model(kind="lstm", hidden=16, input_size=1, seed=5), p)
    return ax.Model(p)


def _pool(model, S, max_frames, metered=True, **controls):
    p = ax.Pool(S, max_frames)
    p.set_model(model)
    if controls:
        p.set_controls(ax.default_controls(**controls))
    if metered:
        p.set_metering(True)
    return p


def _ragged_pool(model, metered):
    """five streams, stream 0 driven hot and turned up (overs), stream 1 turned down (none)"""
    p = _pool(model, 5, 257, metered)
    p.set_controls(ax.default_controls(pregain_db=12.0, master_db=40.0), 0)
    p.set_controls(ax.default_controls(pregain_db=-6.0, master_db=-20.0), 1)
    return p


def _cuts(x, plan):
    at = 0
    for n in plan:
        yield np.ascontiguousarray(x[:, at:at + n])
        at += n


def test_ragged_passes(model):
    p = _ragged_pool(model, True)
    assert p.metering
    run = meterhelp.Running(5)
    run.check(p.read_meters(), what="before any pass")
    outs = []
    for k, blk in enumerate(_cuts(modelgen.signal(5, sum(PLAN), seed=21), PLAN)):
        y = p.process(blk)
        outs.append(y)
        if blk.shape[1]:
            run.add(blk, y)                                     # (a zero-length pass is not counted)
        run.check(p.read_meters(), what=f"pass {k} of {blk.shape[1]} frames")
    rec = p.read_meters()
    p.close()
    assert list(rec["frames"]) == [sum(PLAN)] * 5 and list(rec["passes"]) == [sum(1 for n in PLAN if n)] * 5
    y = np.concatenate(outs, axis=1)
    over = (np.abs(y) > np.float32(1.0)).sum(axis=1)
    print("out_over per stream:", list(rec["out_over"]), "out_peak:", list(rec["out_peak"]))
    assert over.max() > 0 and over.min() == 0 and list(rec["out_over"]) == list(over)


def test_nonfinite_samples_on_disabled_streams(model):
    p = _pool(model, 2, 130, enabled=0.0)                       # a raw copy: nothing is poisoned
    run = meterhelp.Running(2)
    x = modelgen.signal(2, 1, seed=22)
    x[0, 0] = np.nan
    y = p.process(x)
    run.add(x, y)
    rec = p.read_meters()
    run.check(rec, what="n = 1")
    assert (rec["in_nonfinite"][0], rec["out_nonfinite"][0], rec["in_peak"][0], rec["out_peak"][0], rec["in_energy"][0], rec["out_energy"][0],
            rec["frames"][0]) == (1, 1, 0.0, 0.0, 0.0, 0.0, 1)
    x = modelgen.signal(2, 130, seed=23)
    placed = {0: np.nan, 63: np.inf, 64: -np.inf, 129: np.nan}
    for t, v in placed.items():
        x[0, t] = v
    y = p.process(x)
    run.add(x, y)
    rec = p.read_meters()
    p.close()
    run.check(rec, what="n = 130")
    assert rec["in_nonfinite"][0] == rec["out_nonfinite"][0] == 1 + len(placed)
    assert rec["in_nonfinite"][1] == rec["out_nonfinite"][1] == 0
    fin = np.delete(x[0], list(placed))
    assert rec["in_peak"][0] == rec["out_peak"][0] == np.abs(fin).max() > 0 and rec["out_energy"][0] > 0


@pytest.fixture(scope="module")
def skip_model(tmp_path_factory):
    """LSTM-16 with in_skip = 1, the residual form amp captures are usually trained in: output = net(x) + x"""
    p = str(tmp_path_factory.mktemp("meters") / "lstm16_skip.json")
    modelgen.write_model(modelgen.make_model(kind="lstm", hidden=16, input_size=1, seed=5, in_skip=1), p)
    return ax.Model(p)


def _poisoned_run(model):
    """two streams, three passes of 64 frames, one NaN in stream 0's input in the first: the records checked against the blocks after
    every pass and stream 1 against a twin pool that never saw the NaN. Returns the pools, the running record, stream 0's
    (in_nonfinite, out_nonfinite) after each pass and both pools' blocks."""
    p, twin = _pool(model, 2, 64), _pool(model, 2, 64, metered=False)
    run = meterhelp.Running(2)
    seen, outs = [], []
    for k, blk in enumerate(_cuts(modelgen.signal(2, 64 * 3, seed=24), [64] * 3)):
        clean = blk.copy()
        if k == 0:
            blk[0, 10] = np.nan
        y, y_twin = p.process(blk), twin.process(clean)
        outs.append((y, y_twin))
        run.add(blk, y)
        rec = p.read_meters()
        run.check(rec, what=f"pass {k}")
        assert np.array_equal(y[1].view(np.uint32), y_twin[1].view(np.uint32))
        seen.append((int(rec["in_nonfinite"][0]), int(rec["out_nonfinite"][0])))
        assert rec["in_nonfinite"][1] == rec["out_nonfinite"][1] == 0
    print("(in_nonfinite, out_nonfinite) of the poisoned stream after passes 1, 2, 3:", seen)
    assert [a for a, _ in seen] == [1, 1, 1]
    return p, twin, run, seen, outs


def test_the_stuck_stream_signature(skip_model):
    """one NaN in a stream's input: its output stays non-finite, pass after pass, until aidax_pool_reset_stream; its neighbour hears
    nothing. (A model with in_skip = 1: the NaN that the input filter's memory now holds reaches the output through the skip path.
    Without one the recurrent kernels absorb it, see the next test.)"""
    p, twin, run, seen, _ = _poisoned_run(skip_model)
    assert 0 < seen[0][1] < seen[1][1] < seen[2][1]
    p.reset_stream(0)
    p.read_meters(clear=True)
    run.clear(range(2))
    blk = modelgen.signal(2, 64, seed=31)
    y = p.process(blk)
    run.add(blk, y)
    rec = p.read_meters()
    run.check(rec, what="after the reset")
    assert rec["out_nonfinite"][0] == 0 and np.isfinite(y).all()
    p.close()
    twin.close()


def test_a_stuck_stream_whose_model_absorbs_the_nan(model):
    """The same run on a model WITHOUT a skip path. The stream is just as stuck, its input filter's fp64 memory is NaN and every later
    sample reaches the cell as NaN, but the LSTM kernels clamp their tanh arguments with v_max / v_min, which return the other operand
    for a NaN (tanh_rat_clamp, aidax_device.h): the cell turns NaN into saturated, finite values and the stream plays finite garbage.
    Measured on an MI355X (k_lstm_pipe<16>): (in_nonfinite, out_nonfinite) = (1, 0), (1, 0), (1, 0) after the three passes. So
    out_nonfinite cannot show this stream; in_nonfinite does, which is why the host's rule resets on either. What is
    asserted here is only what the meters promise: the records describe the blocks, and the clean passes of the stuck stream are not
    the twin's."""
    p, twin, run, seen, outs = _poisoned_run(model)
    for y, y_twin in outs[1:]:
        assert not np.array_equal(y[0].view(np.uint32), y_twin[0].view(np.uint32))
    p.close()
    twin.close()


def test_clear_and_ranges(model):
    p = _pool(model, 5, 64)
    run = meterhelp.Running(5)
    x = modelgen.signal(5, 64 * 3, seed=25)
    blocks = list(_cuts(x, [64, 33, 64]))
    for blk in blocks[:2]:
        run.add(blk, p.process(blk))
    a, b = p.read_meters(), p.read_meters()
    assert a.tobytes() == b.tobytes()
    run.check(a)
    got = p.read_meters(2, 2, clear=True)
    assert got.tobytes() == a[2:4].tobytes()
    after = p.read_meters()
    assert after[2:4].tobytes() == bytes(128) and after[:2].tobytes() == a[:2].tobytes() and after[4:].tobytes() == a[4:].tobytes()
    run.clear([2, 3])
    run.add(blocks[2], p.process(blocks[2]))                    # counts from zero there, goes on elsewhere
    rec = p.read_meters()
    run.check(rec, what="the pass behind the clear")
    assert list(rec["passes"]) == [3, 3, 1, 1, 3]
    run.check(p.read_meters(1, 3), first=1)
    for first, count in ((0, 0), (3, 0), (4, 2), (5, 1), (0, 6), (0xFFFFFFFF, 2)):
        for clear in (False, True):
            with pytest.raises(ax.AidaxError) as e:
                p.read_meters(first, count, clear=clear)
            assert e.value.code == ERR_ARG, (first, count)
    assert p.read_meters().tobytes() == rec.tobytes()
    p.close()


def test_off_by_default_on_and_off(model):
    plain = _ragged_pool(model, False)
    assert not plain.metering
    with pytest.raises(ax.AidaxError) as e:
        plain.read_meters()
    assert e.value.code == ERR_STATE
    plain.set_metering(False)                                   # off before it was ever on: still nothing to read
    with pytest.raises(ax.AidaxError) as e:
        plain.read_meters()
    assert e.value.code == ERR_STATE
    metered = _ragged_pool(model, True)
    assert metered.kernel_name == plain.kernel_name
    for blk in _cuts(modelgen.signal(5, sum(PLAN), seed=21), PLAN):
        assert np.array_equal(metered.process(blk).view(np.uint32), plain.process(blk).view(np.uint32))
    assert metered.kernel_name == plain.kernel_name
    plain.close()
    before = metered.read_meters()
    x = modelgen.signal(5, 128, seed=26)
    metered.set_metering(False)
    assert not metered.metering
    metered.process(np.ascontiguousarray(x[:, :64]))
    assert metered.read_meters().tobytes() == before.tobytes()  # not counted, and the records from before are kept
    metered.set_metering(True)
    assert metered.metering
    blk = np.ascontiguousarray(x[:, 64:])
    y = metered.process(blk)
    rec = metered.read_meters()
    metered.close()
    assert list(rec["passes"]) == [int(v) + 1 for v in before["passes"]] and list(rec["frames"]) == [int(v) + 64 for v in before["frames"]]
    assert np.array_equal(rec["in_peak"], np.maximum(before["in_peak"], np.abs(blk).max(axis=1)))
    assert np.array_equal(rec["out_peak"], np.maximum(before["out_peak"], np.abs(y).max(axis=1)))


def test_behind_the_ir_stage(model):
    S = 3
    wet, dry = _pool(model, S, 64), _pool(model, S, 64)
    wet.set_ir(np.array([0.5, 0.25], np.float32))
    run_wet, run_dry = meterhelp.Running(S), meterhelp.Running(S)
    blocks = list(_cuts(modelgen.signal(S, 64 * 4, seed=27), [64, 64, 64, 64]))
    for blk in blocks[:3]:
        run_wet.add(blk, wet.process(blk))
        run_dry.add(blk, dry.process(blk))
    rw, rd = wet.read_meters(), dry.read_meters()
    run_wet.check(rw, what="wet")
    run_dry.check(rd, what="dry")
    assert np.array_equal(rw["in_peak"], rd["in_peak"]) and np.array_equal(rw["in_energy"], rd["in_energy"])
    assert (rw["out_peak"] != rd["out_peak"]).all() and (rw["out_energy"] != rd["out_energy"]).all()
    # the pass behind a commit of another IR, with a fade: metered on what it returned
    wet.set_ir_fade(32)
    wet.set_ir(np.array([0.25, -0.5, 0.125], np.float32))
    run_wet.add(blocks[3], wet.process(blocks[3]))
    run_wet.check(wet.read_meters(), what="the fade pass")
    wet.close()
    dry.close()


def test_submit_and_collect_with_two_blocks_in_flight(model):
    S = 6
    p = _pool(model, S, 64)
    run = meterhelp.Running(S)
    blocks = list(_cuts(modelgen.signal(S, 64 * 2 + 37 + 64, seed=28), [64, 64, 37, 64]))
    p.submit(blocks[0])
    p.submit(blocks[1])
    outs = [p.collect(64)]
    p.submit(blocks[2])
    p.submit(blocks[3])
    rec = p.read_meters()                                       # behind every pass issued so far: all four
    outs += [p.collect(64), p.collect(37), p.collect(64)]
    for blk, y in zip(blocks, outs):
        run.add(blk, y)
    run.check(rec, what="two in flight")
    run.check(p.read_meters())
    p.close()


def test_under_a_rate_adapter(model):
    """44.1 kHz around a 48 kHz pool: the records are over the pool's blocks, those of a twin pool fed by the adapter's first stage by hand"""
    S, host, rate = 3, 44100, 48000
    blocks = (64, 1, 0, 255, 17, 256)
    p, twin = _pool(model, S, 288), _pool(model, S, 288)
    ad = ax.RateAdapter(p, float(host), 256)
    A = ax.Resampler(S, float(host), float(rate), rr.delays(host, rate)[0], 0, 256)
    run = meterhelp.Running(S)
    frames = rr.pool_frames(blocks, host, rate)
    for blk, m in zip(_cuts(modelgen.signal(S, sum(blocks), seed=29), blocks), frames):
        ad.process(blk)
        ya = A.process(blk, m) if blk.shape[1] else np.empty((S, 0), np.float32)
        yb = twin.process(ya)
        if m:
            run.add(ya, yb)
    rec = p.read_meters()
    run.check(rec, what="the adapter's pool")
    run.check(twin.read_meters(), what="the twin")
    assert list(rec["frames"]) == [sum(frames)] * S and list(rec["passes"]) == [sum(1 for m in frames if m)] * S
    ad.close()
    A.close()
    p.close()
    twin.close()


def test_a_one_stream_pool_through_the_blocking_path(model):
    """the zero-copy path: both sides read their block in pinned host memory, and the completion word that the model's kernel writes
    itself in an unmetered pool comes from the queue, behind the output side's launch (whose order tests/test_gpu_meters_rt.py holds: the
    records cannot show an end marker issued early, nothing the host does between two blocking passes writes the block that launch reads)"""
    p = _pool(model, 1, 64)
    run = meterhelp.Running(1)
    for k, blk in enumerate(_cuts(modelgen.signal(1, 64 * 50, seed=30), [64] * 50)):
        run.add(blk, p.process(blk))
        run.check(p.read_meters(), what=f"block {k}")
    p.close()
