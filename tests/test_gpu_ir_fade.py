"""The IR fade on the GPU (-m gpu): aidax_pool_set_ir_fade, the pool's fade-out plan and k_ir_fade (include/aidax.h, "IR fade").

Every case drives three pools with the same model, seed and input: the pool under test (fade length F), and two twins with F == 0, one
that never sees the change ("old all along") and one that gets it at the same block boundary ("new all along": the stage works on the
stream's whole dry history, so from that boundary on it returns what a pool that always had the new IR returns). As in
tests/test_gpu_ir_bank.py the pools run a real model with every stream disabled, so the stage's input is the test's input bit for bit
(a twin without an IR is held to that), and the fp64 truth of tests/irfade.py is computed from the input itself.

The fade pass of a stream whose effective IR changed is held per sample to TAU * E[t], TAU = 4e-6 being tests/test_gpu_ir.py's bound for
one convolution (measured there 4.3e-7): the two sides enter with weights that sum to one, and the mix adds three fp32 roundings, below
2e-7 * E. Everything else is compared with np.array_equal: frames past the fade, later passes, unchanged streams."""
import importlib

import numpy as np
import pytest

from tests import errlog, irfade, modelgen
from tests.test_gpu_ir import TAU

pytestmark = pytest.mark.gpu
ax = importlib.import_module("aidadsp-lv2_amd")
ERR_ARG = -1


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    p = str(tmp_path_factory.mktemp("ir_fade") / "lstm16.json")
    modelgen.write_model(modelgen.make_model(kind="lstm", hidden=16, input_size=1, seed=5), p)
    return ax.Model(p)


def _ir(L, seed, sign=1.0):
    rng = np.random.default_rng(seed)
    return (sign * rng.standard_normal(L) * np.exp(-np.arange(L) / max(L / 6.0, 1.0))).astype(np.float32)


def _pool(model, S, max_frames, F):
    p = ax.Pool(S, max_frames)
    p.set_model(model)
    p.set_controls(ax.default_controls(enabled=0.0))
    if F:
        p.set_ir_fade(F)
        assert p.ir_fade() == F
    return p


class Rig:
    """The pool under test, its two twins, and a host record of every stream's effective IR (the taps array, or None)"""

    def __init__(self, model, S, max_frames, F):
        self.S, self.F = S, F
        self.fade = _pool(model, S, max_frames, F)
        self.new = _pool(model, S, max_frames, 0)
        self.old = _pool(model, S, max_frames, 0)
        self.live = [self.fade, self.new, self.old]
        self.assign = [ax.IR_POOL] * S
        self.bank = {}
        self.pool_ir = None
        self.staged = []
        self.x = np.zeros((S, 0), np.float32)

    def freeze(self):
        """from here on the "old" twin sees no change; returns the effective IRs as they stand"""
        self.live = [self.fade, self.new]
        return self.effective()

    def effective(self):
        return [self.pool_ir if a == ax.IR_POOL else self.bank.get(a) if a >= 0 else None for a in self.assign]

    def set_ir(self, h):
        for p in self.live:
            p.set_ir(h)
        self.pool_ir = h

    def set_ir_slot(self, k, h):
        for p in self.live:
            p.set_ir_slot(k, h)
        self.bank[k] = h

    def commit(self, k, h, free="later"):
        """prepare + commit of the pool IR (k == IR_POOL) or a slot; free: "now" (before the next pass is issued) or "later" (close)"""
        for p in self.live:
            sg = p.prepare_ir(h) if k == ax.IR_POOL else p.prepare_ir_slot(k, h)
            p.commit_ir(sg)
            if free == "now":
                p.staged_free(sg)
            else:
                self.staged.append((p, sg))
        if k == ax.IR_POOL:
            self.pool_ir = h
        else:
            self.bank[k] = h

    def assign_ir(self, s, k):
        for p in self.live:
            p.assign_ir(s, k)
        if s == ax.ALL_STREAMS:
            self.assign = [k] * self.S
        else:
            self.assign[s] = k

    def block(self, n, seed, via=None):
        """one block of n frames through the three pools: (fade, new, old) outputs; the input joins the history"""
        blk = modelgen.signal(self.S, n, seed=seed) if n else np.zeros((self.S, 0), np.float32)
        self.x = np.concatenate([self.x, blk], axis=1)
        run = via or (lambda p, b: p.process(b))
        return [run(p, np.ascontiguousarray(blk)) for p in (self.fade, self.new, self.old)]

    def close(self):
        for p, sg in self.staged:
            p.staged_free(sg)
        for p in (self.fade, self.new, self.old):
            p.close()


def _same(a, b):
    return a is b


def _check_fade_pass(tag, rig, before, outs, n, later=3, seed=900, via=None, expect_fading=None):
    """outs: the (fade, new, old) outputs of the first pass behind the change. Holds the fading streams to the fp64 truth, everything
    else to the twin bit for bit, then runs `later` more passes against the "new" twin. Returns the fading streams."""
    got, new, _ = outs
    after = rig.effective()
    fading = [s for s in range(rig.S) if not _same(before[s], after[s])]
    if expect_fading is not None:
        assert fading == list(expect_fading), (tag, fading)
    lf = min(rig.F, n)
    assert np.array_equal(got[:, lf:], new[:, lf:]), (tag, "frames past the fade")
    still = [s for s in range(rig.S) if s not in set(fading)]
    # (not against the "old" twin: a change of the plan's longest IR or item count moves the K split, and with it the last bit)
    assert np.array_equal(got[still], new[still]), (tag, "unchanged streams")
    worst = 0.0
    groups = {}
    for s in fading:
        groups.setdefault((id(before[s]), id(after[s])), []).append(s)
    for rows in groups.values():
        y64, E = irfade.expected(rig.x[rows], before[rows[0]], after[rows[0]], rig.F, n)
        err = np.abs(got[rows].astype(np.float64) - y64)
        floor = 1e-12 * E.max()                                        # (the FFT's noise on near-silent samples, as in test_gpu_ir.py)
        over = np.maximum(err - floor, 0.0)
        assert not over[E <= 0].any(), (tag, rows[0])
        ratio = (over / np.where(E > 0, E, 1.0)).max()
        print(f"ir_fade {tag}: streams {rows[0]}..{rows[-1]} ({len(rows)}) max |y - y64| / E = {ratio:.3e}")
        worst = max(worst, ratio)
    if fading:
        errlog.bound(worst, TAU, f"gpu_ir_fade_tau:{tag}")
    for i in range(later):
        got, new, _ = rig.block(n, seed + 1 + i, via)
        assert np.array_equal(got, new), (tag, f"pass {i + 1} after the fade pass")
    return fading


def _start(model, S, n, F, pre=3, seed=100, pool_ir=None, slots=(), assign=None, via=None):
    """a rig with its IRs loaded and `pre` blocks played: the three pools agree bit for bit so far"""
    rig = Rig(model, S, n, F)
    if pool_ir is not None:
        rig.set_ir(pool_ir)
    for k, h in slots:
        rig.set_ir_slot(k, h)
    for s, k in (assign or {}).items():
        rig.assign_ir(s, k)
    for i in range(pre):
        a, b, c = rig.block(n, seed + i, via)
        assert np.array_equal(a, b) and np.array_equal(a, c), "before any change the fade length changes nothing"
    return rig


def test_the_premise_and_the_range_check(model):
    """a pool without an IR, every stream disabled, returns its input bit for bit; frames > 8192 is refused, the value kept"""
    p = _pool(model, 5, 256, 64)
    x = modelgen.signal(5, 256, seed=1)
    assert np.array_equal(p.process(x), x)
    assert ax.lib().aidax_pool_set_ir_fade(p.h, 8193) == ERR_ARG
    assert "fade length" in ax.lib().aidax_last_error().decode()
    assert p.ir_fade() == 64
    p.set_ir_fade(8192)
    assert p.ir_fade() == 8192
    p.set_ir_fade(0)
    assert p.ir_fade() == 0
    p.close()


# ---- accuracy and "the fade is really there"

@pytest.mark.parametrize("S,n,F", [(3, 256, 256), (70, 256, 100), (1, 64, 64)])
def test_the_fade_is_really_there(model, S, n, F):
    """random decaying IRs of different length and sign: the fade pass lies between the twins, far from both on most of its frames,
    starts 1 / Lf of the way from old to new, and matches the fp64 truth"""
    h_old, h_new = _ir(1000, 1), _ir(333, 2, sign=-1.0)
    rig = _start(model, S, n, F, pre=5, pool_ir=h_old)
    before = rig.freeze()
    rig.commit(ax.IR_POOL, h_new)
    outs = rig.block(n, 200)
    got, new, old = (o.astype(np.float64) for o in outs)
    lf = min(F, n)
    _, E = irfade.expected(rig.x, h_old, h_new, F, n)
    far_old = np.abs(got - old)[:, :lf - 1] > 10 * TAU * E[:, :lf - 1]
    far_new = np.abs(got - new)[:, :lf - 1] > 10 * TAU * E[:, :lf - 1]
    assert (far_old & far_new).mean() > 0.8, (far_old.mean(), far_new.mean())
    # y[0] - old[0] = (new[0] - old[0]) / Lf. A fade that does nothing gives 0 or 1 on the left, one that runs from new to old
    # 1 - 1 / Lf, one whose weights are a frame early or late 2 / Lf or 0: held to a quarter of 1 / Lf, on the streams whose two sides
    # are far enough apart at frame 0 for the quotient to be known to half of that (each side is within TAU * E of its truth)
    step = new[:, 0] - old[:, 0]
    big = np.abs(step) > 16 * lf * TAU * E[:, 0]
    assert big.any()
    assert np.abs((got[big, 0] - old[big, 0]) / step[big] - 1.0 / lf).max() < 0.25 / lf
    # ... and monotonically on: frame t sits (t + 1) / Lf of the way
    t = lf // 2
    big = np.abs(new[:, t] - old[:, t]) > 1000 * TAU * E[:, t]
    assert big.any()
    assert np.abs((got[big, t] - old[big, t]) / (new[big, t] - old[big, t]) - (t + 1.0) / lf).max() < 0.01
    _check_fade_pass(f"there-S{S}-n{n}-F{F}", rig, before, outs, n, expect_fading=range(S))
    rig.close()


# ---- bit identity where nothing changes

def test_a_fade_length_alone_changes_nothing(model):
    S, n = 70, 256
    rig = _start(model, S, n, 128, pre=2, pool_ir=_ir(4097, 3), slots=[(2, _ir(33, 4))], assign={5: 2, 6: ax.IR_NONE})
    for i in range(4):
        a, b, c = rig.block(n, 300 + i)
        assert np.array_equal(a, b) and np.array_equal(a, c)
    rig.close()


def test_assignments_that_change_nothing_do_not_fade(model):
    """assign_ir to the value a stream already has, and A -> B -> A between two passes: bit-identical to the twin that saw nothing"""
    S, n = 40, 256
    rig = _start(model, S, n, 256, pre=3, pool_ir=_ir(1000, 5), slots=[(0, _ir(33, 6)), (1, _ir(4097, 7))], assign={3: 0, 4: 1, 5: ax.IR_NONE})
    before = rig.freeze()
    rig.assign_ir(3, 0)
    rig.assign_ir(7, ax.IR_POOL)
    rig.assign_ir(4, 0)
    rig.assign_ir(4, 1)
    rig.assign_ir(5, 1)
    rig.assign_ir(5, ax.IR_POOL)
    rig.assign_ir(5, ax.IR_NONE)
    rig.assign_ir(8, ax.IR_NONE)
    rig.assign_ir(8, ax.IR_POOL)
    outs = rig.block(n, 400)
    assert np.array_equal(outs[0], outs[2])
    _check_fade_pass("noop", rig, before, outs, n, expect_fading=[])
    rig.close()


def test_the_same_run_twice_gives_the_same_bits(model):
    runs = []
    for _ in range(2):
        rig = _start(model, 70, 256, 200, pre=3, pool_ir=_ir(8192, 8), slots=[(9, _ir(4097, 9))], assign={s: 9 for s in range(0, 70, 3)})
        rig.freeze()
        rig.commit(ax.IR_POOL, _ir(33, 10))
        rig.assign_ir(0, ax.IR_NONE)
        rig.assign_ir(1, 9)
        runs.append(np.concatenate([rig.block(256, 500 + i)[0] for i in range(3)], axis=1))
        rig.close()
    assert np.array_equal(runs[0], runs[1])


# ---- every trigger

def _trigger(model, tag, change, S=20, n=256, F=256, expect=None, **kw):
    kw.setdefault("pool_ir", _ir(1000, 11))
    kw.setdefault("slots", [(0, _ir(33, 12)), (1, _ir(4097, 13, sign=-1.0)), (7, _ir(200, 14))])
    kw.setdefault("assign", {0: 0, 1: 0, 2: 1, 3: 1, 4: ax.IR_NONE, 5: ax.IR_NONE, 6: 7, 8: 40})     # (slot 40 is empty)
    rig = _start(model, S, n, F, **kw)
    before = rig.freeze()
    change(rig)
    outs = rig.block(n, 600)
    fading = _check_fade_pass(tag, rig, before, outs, n, expect_fading=expect)
    rig.close()
    return fading


def test_trigger_slot_to_slot(model):
    _trigger(model, "slot-slot", lambda r: (r.assign_ir(0, 1), r.assign_ir(2, 7)), expect=[0, 2])


def test_trigger_slot_to_pool_ir_and_back(model):
    _trigger(model, "slot-pool", lambda r: (r.assign_ir(1, ax.IR_POOL), r.assign_ir(10, 0)), expect=[1, 10])


def test_trigger_ir_to_none_and_back(model):
    _trigger(model, "none", lambda r: (r.assign_ir(0, ax.IR_NONE), r.assign_ir(9, ax.IR_NONE), r.assign_ir(4, 1), r.assign_ir(5, ax.IR_POOL)),
             expect=[0, 4, 5, 9])


def test_trigger_assignment_to_an_empty_slot_and_away_from_it(model):
    _trigger(model, "empty", lambda r: (r.assign_ir(2, 41), r.assign_ir(8, 0), r.assign_ir(4, 41)), expect=[2, 8])


def test_trigger_commit_into_a_slot(model):
    """all of the slot's streams fade, the others are bit-identical"""
    _trigger(model, "commit-slot", lambda r: r.commit(1, _ir(777, 15)), expect=[2, 3])


def test_trigger_commit_into_an_empty_slot_and_emptying_one(model):
    _trigger(model, "commit-empty", lambda r: (r.commit(40, _ir(50, 16)), r.commit(0, None)), expect=[0, 1, 8])


def test_trigger_commit_of_the_pool_ir(model):
    _trigger(model, "commit-pool", lambda r: r.commit(ax.IR_POOL, _ir(8192, 17)), expect=[7] + list(range(9, 20)))


def test_trigger_removal_of_the_pool_ir_and_a_first_one(model):
    _trigger(model, "remove-pool", lambda r: r.commit(ax.IR_POOL, None), expect=[7] + list(range(9, 20)))
    _trigger(model, "first-pool", lambda r: r.commit(ax.IR_POOL, _ir(100, 18)), expect=[7] + list(range(9, 20)), pool_ir=None)


def test_trigger_the_blocking_forms(model):
    """set_ir and set_ir_slot free what the commit hands back before the fade pass is issued"""
    _trigger(model, "set_ir", lambda r: r.set_ir(_ir(300, 19)), expect=[7] + list(range(9, 20)))
    _trigger(model, "set_ir_slot", lambda r: r.set_ir_slot(0, _ir(300, 20)), expect=[0, 1])
    _trigger(model, "set_ir-none", lambda r: (r.set_ir(None), r.set_ir_slot(1, None)), expect=[2, 3, 7] + list(range(9, 20)))


def test_trigger_several_moves_and_a_commit_in_one_gap(model):
    def change(r):
        r.assign_ir(0, 1)                                  # slot 0 -> slot 1, whose content changes too: from 0's old to 1's new
        r.assign_ir(2, 0)                                  # slot 1 (old content) -> slot 0
        r.commit(1, _ir(64, 21))                           # stream 3 stays on slot 1: old content -> new content
        r.assign_ir(4, 7)
        r.assign_ir(4, 1)                                  # none -> 7 -> 1 collapses into none -> 1's new content
        r.assign_ir(6, ax.IR_POOL)
        r.assign_ir(6, 7)                                  # 7 -> pool -> 7: nothing
        r.assign_ir(9, 1)
    _trigger(model, "gap", change, expect=[0, 2, 3, 4, 9])


def test_a_slot_committed_twice_between_two_passes_fades_from_what_was_played(model):
    """the first commit's content is never played and goes straight back; the parked IR stays the one the streams last went through"""
    def change(r):
        r.commit(1, _ir(500, 22), free="now")
        r.commit(1, _ir(90, 23), free="now")
        r.commit(ax.IR_POOL, _ir(10, 24), free="now")
        r.commit(ax.IR_POOL, None, free="now")
        r.commit(ax.IR_POOL, _ir(2000, 25), free="now")
    _trigger(model, "twice", change, expect=[2, 3, 7] + list(range(9, 20)))


def test_fades_in_consecutive_passes(model):
    """a commit into the same slot before each of four passes in a row: every one fades from the content played just before, while the
    commits hand back the fragments parked one commit earlier"""
    S, n, F = 6, 256, 256
    rig = _start(model, S, n, F, pre=2, slots=[(3, _ir(1000, 30))], assign={s: 3 for s in range(4)})
    rig.freeze()                                           # (the "old" twin is not looked at: the old side changes every pass)
    for i in range(4):
        before = rig.effective()
        rig.commit(3, _ir((33, 4097, 1, 8192)[i], 31 + i), free="now" if i % 2 else "later")
        got, new, _ = rig.block(n, 700 + i)
        y64, E = irfade.expected(rig.x[:4], before[0], rig.effective()[0], F, n)
        err = np.abs(got[:4].astype(np.float64) - y64)
        errlog.bound((np.maximum(err - 1e-12 * E.max(), 0.0) / np.where(E > 0, E, 1.0)).max(), TAU, "gpu_ir_fade_tau:consecutive")
        assert np.array_equal(got[4:], new[4:])
        assert np.array_equal(got[:, F:], new[:, F:])
    got, new, _ = rig.block(n, 710)
    assert np.array_equal(got, new)
    rig.close()


# ---- lifetime

@pytest.mark.parametrize("L", [8192, 1000])
def test_the_old_ir_outlives_the_free_of_what_the_commit_handed_back(model, L):
    """commit, staged_free, then a PREPARE (not committed) of another IR of the same length, which gives the allocator the chance to
    hand the retired fragments' memory out again, then the pass: it still fades from the true old IR"""
    S, n, F = 70, 256, 256
    h_old = _ir(L, 40)
    rig = _start(model, S, n, F, pre=3, slots=[(5, h_old)], assign={s: 5 for s in range(0, S, 2)})
    before = rig.freeze()
    rig.commit(5, _ir(L, 41, sign=-1.0), free="now")
    decoys = [(p, p.prepare_ir_slot(5, np.full(L, 1000.0, np.float32))) for p in (rig.fade, rig.new) for _ in range(2)]
    outs = rig.block(n, 800)
    _check_fade_pass(f"lifetime-L{L}", rig, before, outs, n, expect_fading=range(0, S, 2))
    for p, sg in decoys:
        p.staged_free(sg)
    rig.close()


# ---- shapes

@pytest.mark.parametrize("S", [1, 70, 1024])
def test_pool_sizes(model, S):
    """K split (small pools) and none (1024 streams); more than 64 streams fading from one IR (several work items of the fade-out plan)"""
    n, F = 256, 192
    pre = 34 if S == 1 else 3                              # the one-stream pool plays past the IR's 8192 taps
    rig = _start(model, S, n, F, pre=pre, pool_ir=_ir(8192, 50), slots=[(0, _ir(4097, 51))], assign={s: 0 for s in range(1, S, 5)})
    before = rig.freeze()
    rig.commit(ax.IR_POOL, _ir(8192, 52, sign=-1.0))
    if S > 1:
        rig.assign_ir(1, ax.IR_POOL)                       # from the slot to the NEW pool IR
        rig.assign_ir(2, 0)                                # from the OLD pool IR to the slot
    outs = rig.block(n, 900)
    fading = _check_fade_pass(f"S{S}", rig, before, outs, n)
    assert len(fading) == (1 if S == 1 else S - len(range(1, S, 5)) + 1)
    rig.close()


@pytest.mark.parametrize("L_old,L_new", [(1, 8192), (8192, 33), (33, 4097), (4097, 1)])
def test_ir_lengths(model, L_old, L_new):
    S, n, F = 3, 256, 256
    rig = _start(model, S, n, F, pre=34, slots=[(0, _ir(L_old, 60)), (1, _ir(L_new, 61))], assign={0: 0, 1: 0, 2: 1})
    before = rig.freeze()
    rig.assign_ir(0, 1)
    rig.commit(0, _ir(L_new, 62))
    outs = rig.block(n, 1000)
    _check_fade_pass(f"L{L_old}-{L_new}", rig, before, outs, n, expect_fading=[0, 1])
    rig.close()


@pytest.mark.parametrize("n,F", [(64, 16), (64, 64), (64, 8192), (256, 1), (256, 255), (256, 256), (256, 257), (1000, 64), (1000, 1000),
                                 (1000, 4096)])
def test_block_and_fade_lengths(model, n, F):
    """F below, equal to and above n_frames, on blocks of 64, 256 and 1000 frames"""
    S = 17
    rig = _start(model, S, n, F, pre=3, pool_ir=_ir(2000, 70), slots=[(0, _ir(300, 71, sign=-1.0))], assign={s: 0 for s in range(0, S, 4)})
    before = rig.freeze()
    rig.commit(0, _ir(1500, 72))
    rig.assign_ir(1, ax.IR_NONE)
    rig.assign_ir(2, 0)
    outs = rig.block(n, 1100)
    _check_fade_pass(f"n{n}-F{F}", rig, before, outs, n, expect_fading=[0, 1, 2, 4, 8, 12, 16])
    rig.close()


def test_a_shorter_block_than_max_frames_and_an_unaligned_ring_position(model):
    S, F = 5, 100
    rig = _start(model, S, 256, F, pre=2, pool_ir=_ir(1000, 80))
    for i, n in enumerate((17, 3, 250)):
        a, b, _ = rig.block(n, 1200 + i)
        assert np.array_equal(a, b)
    before = rig.freeze()
    rig.assign_ir(1, ax.IR_NONE)
    rig.commit(ax.IR_POOL, _ir(77, 81))
    outs = rig.block(131, 1210)
    _check_fade_pass("ragged", rig, before, outs, 131, expect_fading=range(S))
    rig.close()


def test_a_pass_of_zero_frames_leaves_the_fade_pending(model):
    S, n, F = 9, 256, 256
    rig = _start(model, S, n, F, pre=3, pool_ir=_ir(1000, 90))
    before = rig.freeze()
    rig.commit(ax.IR_POOL, _ir(400, 91, sign=-1.0))
    rig.assign_ir(0, ax.IR_NONE)
    for o in rig.block(0, 0):
        assert o.shape == (S, 0)
    outs = rig.block(n, 1300)
    _check_fade_pass("zero", rig, before, outs, n, expect_fading=range(S))
    rig.close()


def test_a_fade_length_set_between_the_change_and_the_pass_counts(model):
    """the pass runs with the fade length in force when it was issued: 0 switches, and a later change fades again"""
    S, n = 4, 256
    rig = _start(model, S, n, 256, pre=3, pool_ir=_ir(1000, 95))
    rig.freeze()
    rig.commit(ax.IR_POOL, _ir(400, 96))
    rig.fade.set_ir_fade(0)
    got, new, _ = rig.block(n, 1400)
    assert np.array_equal(got, new)
    rig.fade.set_ir_fade(64)
    rig.F = 64
    before = rig.effective()
    rig.assign_ir(2, ax.IR_NONE)
    outs = rig.block(n, 1401)
    assert not np.array_equal(outs[0][2], outs[1][2])
    _check_fade_pass("late-F", rig, before, outs, n, expect_fading=[2])
    rig.close()


def test_process_device_on_a_callers_stream(model):
    import torch
    q = torch.cuda.Stream()

    def via(p, blk):
        x = torch.from_numpy(blk).cuda()
        y = torch.empty_like(x)
        torch.cuda.synchronize()
        with torch.cuda.stream(q):
            p.process_device(x.data_ptr(), y.data_ptr(), blk.shape[1], q.cuda_stream)
        q.synchronize()
        return y.cpu().numpy()
    S, n, F = 70, 256, 128
    rig = _start(model, S, n, F, pre=3, pool_ir=_ir(4097, 100), slots=[(0, _ir(33, 101))], assign={s: 0 for s in range(0, S, 3)}, via=via)
    before = rig.freeze()
    rig.commit(0, _ir(1000, 102), free="now")
    rig.assign_ir(1, ax.IR_NONE)
    outs = rig.block(n, 1500, via)
    _check_fade_pass("device", rig, before, outs, n, via=via, expect_fading=sorted([1] + list(range(0, S, 3))))
    rig.close()


def test_submit_and_collect_with_two_blocks_in_flight_and_a_change_between_the_submits(model):
    """block k is submitted, then the change, then block k + 1, then both are collected: block k plays the old plan, block k + 1 fades"""
    S, n, F = 70, 256, 256
    rig = _start(model, S, n, F, pre=3, pool_ir=_ir(4097, 110), slots=[(0, _ir(33, 111))], assign={s: 0 for s in range(0, S, 3)})
    b0, b1, b2 = (modelgen.signal(S, n, seed=1600 + i) for i in range(3))
    pools = (rig.fade, rig.new, rig.old)
    for p in pools:
        p.submit(b0)
    before = rig.freeze()
    rig.commit(0, _ir(1000, 112), free="now")
    rig.assign_ir(1, ax.IR_NONE)
    rig.assign_ir(2, 0)
    for p in pools:
        p.submit(b1)
    first = [p.collect(n) for p in pools]
    assert np.array_equal(first[0], first[1]) and np.array_equal(first[0], first[2])
    for p in pools:
        p.submit(b2)
    outs = [p.collect(n) for p in pools]
    last = [p.collect(n) for p in pools]
    assert np.array_equal(last[0], last[1])
    rig.x = np.concatenate([rig.x, b0, b1], axis=1)        # the history up to and including block k + 1
    fading = [1, 2] + list(range(0, S, 3))
    got, new, _ = outs
    lf = min(F, n)
    assert np.array_equal(got[:, lf:], new[:, lf:])
    after = rig.effective()
    for s in range(S):
        if s in fading:
            y64, E = irfade.expected(rig.x[s:s + 1], before[s], after[s], F, n)
            err = np.abs(got[s:s + 1].astype(np.float64) - y64)
            errlog.bound((np.maximum(err - 1e-12 * E.max(), 0.0) / np.where(E > 0, E, 1.0)).max(), TAU, "gpu_ir_fade_tau:submit")
            assert not np.array_equal(got[s], new[s])
        else:
            assert np.array_equal(got[s], new[s])
    rig.close()
