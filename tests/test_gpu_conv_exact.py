"""The conv stacks bit for bit (GPU, -m gpu): every conv kernel form on the exact-arithmetic stacks of tests/convdata.py, where the
correct output is the true one to the last bit whatever the order of the additions (tests/test_conv_arith.py shows that, that the
oracle's network computes exactly that truth, and that a kernel which drops, doubles or misplaces any one of its six term products at
any one tap of any one layer changes output bits). So every comparison here is np.array_equal, against the oracle's full run — pre
gain, network, the master gain's fade-in — under controls that leave nothing else in circuit (in_lpf_pc=0, dc_blocker=0, eq_bypass=1).

Layer 0 of every stack is a saturating quantiser (|z| >= 127 under tanh or sigmoid): each of these runs also holds the conv epilogues'
tanh_exp_pre and fast_sigmoid to exactly +-1 and 1 / 0 there, on every form. The mixed families (T3, T2: linear and relu layers) carry
the term products; the all-tanh family (SIGN) is a routing test of the instantiation BASELINE cfg4 runs (see tests/convdata.py).

Forms, by the asserted pool.kernel_name: no switch — k_conv_st (the five compiled geometries: blocks of 64 / 128 / 256 frames streamed,
every other block through k_conv_ms on the same state), k_conv_ms (the corners k_conv_st has no geometry for), k_conv_mfma (twelve and
eight channels, zero-padded); AIDAX_CONV_ST=0 — k_conv_ms for every block; AIDAX_CONV_FUSED=0 — k_chain + k_conv_ms / k_conv_mfma;
AIDAX_CONV_MS=0 — k_conv_mfma (fp32 MFMAs); AIDAX_KERNEL=valu — k_conv. The tests that set no switch ask for no hook, so the ship leg
runs them on the shipped library."""
import importlib
import json

import numpy as np
import pytest

from oracle import oracle as O
from tests import convdata as cd

pytestmark = pytest.mark.gpu
ax = importlib.import_module("aidadsp-lv2_amd")

RAGGED = [256, 100, 1, 255, 0, 64, 256, 17, 128, 130, 3, 256, 64, 128, 64, 256]      # tests/test_gpu_parity.py's _MS_SIZES: k_conv_st and k_conv_ms on one state
T = sum(RAGGED)
LONG = [2048, 1000, 513, 256, 300, 1, 0, 257]                                        # a pool with max_frames 2048: long blocks go through in slices
CONTROLS = dict(in_lpf_pc=0.0, dc_blocker=0.0, eq_bypass=1.0)
CASES = [(st, f) for st in cd.STACKS for f in cd.FAMILIES]
IDS = [f"{st}-{f}" for st, f in CASES]
FORCED = (("AIDAX_CONV_ST", "0"), ("AIDAX_CONV_FUSED", "0"), ("AIDAX_CONV_MS", "0"), ("AIDAX_KERNEL", "valu"))
_WANT = {}


def kernel_name(stack, switch=None, max_frames=256):
    if switch == "AIDAX_KERNEL":
        return "k_conv"
    if stack in cd.MFMA_STACKS or switch == "AIDAX_CONV_MS":
        return "k_chain+k_conv_mfma" if switch == "AIDAX_CONV_FUSED" else "k_conv_mfma"
    if switch == "AIDAX_CONV_FUSED":
        return "k_chain+k_conv_ms"
    return "k_conv_st" if stack in cd.ST_STACKS and switch is None and max_frames >= 64 else "k_conv_ms"


def _case(stack, family, S, frames=T):
    """(model text, x, the oracle's full run): computed once per case, shared by every form's test, read-only"""
    key = (stack, family, S, frames)
    if key not in _WANT:
        j = cd.make_stack(stack, family)[0]
        x = cd.signal(S, frames, seed=41 + S)
        want = O.run_streams(O.parse_model(j), O.default_controls(**CONTROLS), x, 256)
        assert np.isfinite(want).all() and np.unique(want).size > 50
        # the guarantees on THIS run's data (tests/test_conv_arith.py shows them on a signal of its own): the oracle's run is the numpy
        # truth times the master gain, every sum fits 24 bits, the dropped products are zero and the family's claimed ones are exercised
        y, acts = cd.truth(j, cd.pre_chain(x))
        assert np.array_equal(want, y * cd.gain_ramps(frames)[1][None, :])
        if family in cd.MIXED:
            assert max(cd.budget(j, acts)) < 24.0 and cd.claims_hold(j, family, acts)
        for a in (x, want):
            a.setflags(write=False)
        _WANT[key] = (json.dumps(j), x, want)
    return _WANT[key]


def _run(text, S, x, sizes, name, max_frames=256):
    pool = ax.Pool(S, max_frames)
    pool.set_model(ax.Model(text=text))
    assert pool.kernel_name == name, (pool.kernel_name, name)
    pool.set_controls(ax.default_controls(**CONTROLS))
    got = np.zeros((S, sum(sizes)), np.float32)
    pos = 0
    for n in sizes:
        got[:, pos:pos + n] = pool.process(np.ascontiguousarray(x[:, pos:pos + n]))
        pos += n
    pool.close()
    return got


def _mismatch(tag, got, want):
    want = want[:, :got.shape[1]]
    bad = np.argwhere(got != want)
    if bad.size == 0:
        return []
    s, t = (int(i) for i in bad[0])
    return [(tag, bad.shape[0], (s, t), float(got[s, t]), float(want[s, t]))]


@pytest.mark.parametrize("stack,family", CASES, ids=IDS)
def test_exact_as_the_pool_runs_it(stack, family):
    """no switch set: six streams on the ragged plan, and runs of pure 64-, 128- and 256-frame blocks"""
    text, x, want = _case(stack, family, 6)
    name = kernel_name(stack)
    m = ax.Model(text=text)
    assert m.conv_form == (4 if stack in cd.ST_STACKS else 3 if stack in cd.MS_STACKS else 2)
    bad = _mismatch("ragged", _run(text, 6, x, RAGGED, name), want)
    for nf in (64, 128, 256):
        bad += _mismatch(f"{nf}", _run(text, 6, x, [nf] * (T // nf), name), want)
    assert not bad, bad


@pytest.mark.parametrize("stack,family", CASES, ids=IDS)
def test_exact_on_one_stream_and_on_thirty_seven(stack, family):
    bad = []
    for S in (1, 37):
        text, x, want = _case(stack, family, S)
        bad += _mismatch(f"S={S}", _run(text, S, x, RAGGED, kernel_name(stack)), want)
    assert not bad, bad


@pytest.mark.parametrize("stack,family", CASES, ids=IDS)
def test_exact_on_a_pool_with_long_blocks(stack, family):
    """max_frames 2048: a long block goes through in slices of 256 frames — full slices as a stream of tiles where the geometry is compiled,
    the ragged rest through k_conv_ms"""
    text, x, want = _case(stack, family, 6, sum(LONG))
    got = _run(text, 6, x, LONG, kernel_name(stack, max_frames=2048), max_frames=2048)
    assert not _mismatch("long", got, want)


@pytest.mark.parametrize("stack,family", CASES, ids=IDS)
def test_exact_on_every_forced_form(stack, family, monkeypatch):
    """AIDAX_CONV_ST=0, AIDAX_CONV_FUSED=0, AIDAX_CONV_MS=0, AIDAX_KERNEL=valu: the ragged plan and a run of full 256-frame blocks each"""
    text, x, want = _case(stack, family, 6)
    bad = []
    for switch, value in FORCED:
        for k, _ in FORCED:
            monkeypatch.delenv(k, raising=False)
        monkeypatch.setenv(switch, value)
        name = kernel_name(stack, switch)
        bad += _mismatch(f"{switch} ragged", _run(text, 6, x, RAGGED, name), want)
        bad += _mismatch(f"{switch} 256", _run(text, 6, x, [256] * (T // 256), name), want)
    assert not bad, bad


def _bare(stack):
    j = cd.make_stack(stack, "T3", quantiser=False)[0]
    x = cd.grid_signal(1500, seed=17)
    y, acts = cd.truth(j, x, warm=False)
    assert max(cd.budget(j, acts)) < 24.0
    return json.dumps(j), x, y[0]


@pytest.mark.parametrize("stack", cd.STACKS)
def test_bare_model_launch_is_exact(stack):
    """Model.forward(unit_gains=True): reset state, no chain, no quantiser — layer 0 linear on inputs in {-1, 0, 1} — against the numpy truth.
    The launch builds a pool of its own, one stream and four frames a block, so no kernel name can be asserted here and neither k_conv_st
    nor a full-block instantiation is reached: k_conv_ms's ragged form (k_conv_mfma for the twelve- and eight-channel stacks), asserted
    through conv_form; the forced forms below likewise."""
    text, x, y = _bare(stack)
    m = ax.Model(text=text)
    assert m.conv_form == (4 if stack in cd.ST_STACKS else 3 if stack in cd.MS_STACKS else 2)
    got = m.forward(x[:, None], unit_gains=True)
    assert np.array_equal(got, y), _mismatch("bare", got[None, :], y[None, :])


@pytest.mark.parametrize("stack", cd.STACKS)
def test_bare_model_launch_is_exact_on_every_forced_form(stack, monkeypatch):
    """the same under each switch (the launch's own four-frame pool: k_conv_ms ragged, k_chain + k_conv_ms, k_conv_mfma, k_conv; no name to assert)"""
    text, x, y = _bare(stack)
    bad = []
    for switch, value in FORCED:
        for k, _ in FORCED:
            monkeypatch.delenv(k, raising=False)
        monkeypatch.setenv(switch, value)
        got = ax.Model(text=text).forward(x[:, None], unit_gains=True)
        bad += _mismatch(switch, got[None, :], y[None, :])
    assert not bad, bad
