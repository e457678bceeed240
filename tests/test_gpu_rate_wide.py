"""k_resample beyond the audio pairs (-m gpu): the in-place form k_resample<false>, the staged form with its LDS window filled to the last
float, and the extreme ratios the public API admits, against tests/rateref.py and aidax_resampler_row. Hook-free except
test_the_two_forms_give_the_same_bits, so the ship leg runs the rest on the shipped library.

Which form runs (launch_resample: window = ceil(255 M / L) + T <= 4096 floats is staged), asserted below from tests/rateref.py:

    64 -> 5   T = 821  window 4085  staged          13 -> 1          T =   833  window   4148  in place
    77 -> 6   T = 823  window 4096  staged, full    96000 -> 7000    T =   879  window   4377  in place
    90 -> 7   T = 825  window 4104  in place        192000 -> 8000   T =  1537  window   7657  in place
                                                    640 -> 1         T = 40961  window 204161  in place

Impulses, bit for bit. The input is zeros except impulses +-2^k (k = -3 .. 3), at least T + 1 frames apart within a stream, so an
output's row sees at most one: out[j] = fp32(row_phi(j)[q(j) - p + H]) * amp, taken in fp32 (exact: a power of two), + 0.0 so that every
zero is +0 like the kernel's (its accumulators start at +0 and +0 + -0 = +0); every other output is +0. Rows come from
aidax_resampler_row (host code that tests/test_rate_host.py holds to the fp64 statement), q and phi from rateref's integers. Compared as
uint32. Since gcd(L, M) = 1, entry (phi, t) of the [L][T] table is multiplied by the impulse at p exactly when
(p - H + t) L + phi = a0 (mod M), one residue of p: impulses whose whole reach [p - H, p + H] lies in produced outputs, on every
residue mod M, touch every entry; the test counts them.

Noise against fp64. Per sample |out - ref64| <= gamma_T sum |w| |x|, gamma_T = T u / (1 - T u), u = 2^-24: the bound for T roundings
in any summation order (each product is fused into its addition, each of the at most T additions rounds once). It holds no measured
number. (The (T + 2) u of tests/test_gpu_rate.py is not a gamma at T = 40961; those tests stay as they are.) Every ratio is printed
before it is asserted and logged through tests/errlog.py; profiles/rate_adapter.txt, section 5, keeps the largest.

The last tap of every row, t = T - 1, is exactly 0 for every ratio (n = phi + H L >= Z D, outside the window's support), so the kernel's
`ii + 2 < T` tail term multiplies by zero whenever it is the last tap: no finite input can show its absence (profiles/rate_adapter.txt, section 6: the one equivalent mutant)."""
import importlib
import os
from typing import NamedTuple, Optional

import numpy as np
import pytest

from tests import errlog, modelgen, rateref as rr
from tests.ratehelp import adapter_and_its_parts, feed, noise, pool, stage

pytestmark = pytest.mark.gpu
ax = importlib.import_module("aidadsp-lv2_amd")
ERR_ARG = -1
TILE, WINDOW = 256, 4096                                                    # kRsTile, kRsWindow
# (rate_in, rate_out): T, the window in floats, staged?
TABLE = {(64, 5): (821, 4085, True), (77, 6): (823, 4096, True), (90, 7): (825, 4104, False), (13, 1): (833, 4148, False),
         (96000, 7000): (879, 4377, False), (192000, 8000): (1537, 7657, False), (640, 1): (40961, 204161, False)}
AMPS = tuple(s * 2.0 ** k for k in range(-3, 4) for s in (1.0, -1.0))


class Case(NamedTuple):
    ri: int
    ro: int
    d_in: int
    d_out: int
    max_in: int
    cap: Optional[int]          # the blocking call's limit, where a call could be asked for more
    full: bool                  # the impulses cover every residue mod M (the whole table is multiplied)

    @property
    def id(self):
        return f"{self.ri}-{self.ro}" + (f"-d{self.d_in}-{self.d_out}" if self.d_in or self.d_out else "")


CASES = (Case(64, 5, 0, 0, 8192, None, True), Case(77, 6, 0, 0, 8192, None, True), Case(90, 7, 5, 3, 8192, None, True),
         Case(13, 1, 0, 0, 8192, None, True), Case(96000, 7000, 0, 2, 8192, None, True), Case(192000, 8000, 0, 0, 8192, None, True),
         Case(640, 1, 0, 0, 16384, None, False))
# delays longer than the ring (R = 256): the staged form, every output taken in pieces of at most 143
DELAYED = Case(44100, 48000, 1000, 700, 64, 143, True)
S_IMP = 3


def ring(c):
    """slots per stream: the power of two >= T + 2 max_in + 2 ceil(M / L) + 2 (aidax_rate.cpp)"""
    L, M, D, _, H, T = rr.params(c.ri, c.ro)
    R = 64
    while R < T + 2 * c.max_in + 2 * -(-M // L) + 2:
        R *= 2
    return R


def cuts_for(N, max_in):
    """ragged calls up to N frames: single frames, full blocks, odd sizes; seven sizes in turn, so both call shapes meet every size"""
    sizes, out, k = (1, 7, max_in, max_in * 3 // 8 + 5, max_in, 17, max_in // 2 + 1), [], 0
    while sum(out) < N:
        out.append(min(sizes[k % 7], N - sum(out)))
        k += 1
    return tuple(out)


def plan(c, S=S_IMP):
    """(impulses per stream as lists of (position, amplitude), N, cuts): stream 0 starts with an impulse on frame 0 (its history is the
    zeros before the stream's start; frame 0 is also the oldest frame the ring ever holds), then impulse i sits on residue i mod M in
    stream i mod S, the first position free there: at least T + 1 after the stream's last one and at least H from the start"""
    L, M, D, _, H, T = rr.params(c.ri, c.ro)
    imps = [[] for _ in range(S)]
    imps[0].append((0, AMPS[-1]))
    for i in range(M if c.full else 9):
        s = i % S
        p = max(imps[s][-1][0] + T + 1 if imps[s] else 0, H)
        p += (i - p) % M
        imps[s].append((p, AMPS[i % len(AMPS)]))
    N = max(max(v[-1][0] for v in imps) + 2 * H + 1,                      # the last impulse's whole reach is produced
            ring(c) + 1000,                                                 # the ring wraps
            H + 300 * M // L)                                               # more than 256 outputs
    return imps, N, cuts_for(N, c.max_in)


def expected(c, imps, n_out, table):
    """the outputs as uint32-comparable fp32, and the [L][T] map of table entries an impulse with its whole reach produced multiplied"""
    L, M, D, _, H, T = rr.params(c.ri, c.ro)
    q, phi = rr.q_phi(c.ri, c.ro, c.d_in, c.d_out, 0, n_out)
    want, hit = np.zeros((len(imps), n_out), np.float32), np.zeros((L, T), bool)
    for s, row in enumerate(imps):
        for p, amp in row:
            t = q - p + H
            sel = (t >= 0) & (t < T)
            want[s, sel] = table[phi[sel], t[sel]] * np.float32(amp) + np.float32(0.0)
            if p >= H and np.count_nonzero(sel) and q[-1] >= p + H:
                hit[phi[sel], t[sel]] = True
    return want, hit


def check_the_plan(c, imps, N, cuts):
    """the conditions on the positions, from the integers alone"""
    L, M, D, _, H, T = rr.params(c.ri, c.ro)
    assert sum(cuts) == N and max(cuts) <= c.max_in <= 300000 and N > ring(c)
    ends = np.cumsum(cuts)
    outs = np.diff([0] + [rr.ready(int(e), c.ri, c.ro, c.d_in, c.d_out) for e in ends])
    assert np.any(outs % TILE != 0)                                         # a call ends in a partial tile
    if c.cap is None:
        assert outs.sum() > TILE
        if c.ri != 640:
            assert outs.max() > TILE                                       # several tiles in one call (640 -> 1: in total)
    call_of = lambda p: int(np.searchsorted(ends, p, side="right"))
    for s, row in enumerate(imps):
        pos = [p for p, _ in row]
        assert all(b - a >= T + 1 for a, b in zip(pos, pos[1:])), s         # no row sees two
        assert any(call_of(p) >= 1 for p in pos), s                         # an impulse inside a later call
        assert all(abs(a) in AMPS for _, a in row)
    assert imps[0][0][0] < H
    inner = [(p, a) for row in imps for p, a in row if p >= H and p + 2 * H < N]
    if c.full:
        assert {p % M for p, _ in inner} == set(range(M))
    else:
        assert sum(a > 0 for _, a in inner) >= 2 and sum(a < 0 for _, a in inner) >= 2 and len(inner) >= 5
        assert len({call_of(p) for p, _ in inner}) >= 5


def run_impulses(c):
    imps, N, cuts = plan(c)
    check_the_plan(c, imps, N, cuts)
    L, M, D, _, H, T = rr.params(c.ri, c.ro)
    x = np.zeros((S_IMP, N), np.float32)
    for s, row in enumerate(imps):
        for p, amp in row:
            x[s, p] = amp
    table = np.stack([ax.resampler_row(float(c.ri), float(c.ro), phase) for phase in range(L)])
    assert table.shape == (L, T) and table.dtype == np.float32
    n_out = rr.ready(N, c.ri, c.ro, c.d_in, c.d_out)
    want, hit = expected(c, imps, n_out, table)
    if c.full:
        assert hit.all(), f"{np.count_nonzero(~hit)} of {L * T} table entries are never multiplied"
    rs = stage(S_IMP, c.ri, c.ro, c.d_in, c.d_out, c.max_in)
    got = feed(rs, x, cuts, cap=c.cap)
    rs.close()
    assert got.shape == want.shape
    bad = np.argwhere(got.view(np.uint32) != want.view(np.uint32))
    assert bad.size == 0, (f"{len(bad)} outputs differ; the first: (stream, j) = {tuple(bad[0])}, got {got[tuple(bad[0])]!r}, "
                           f"want {want[tuple(bad[0])]!r}")
    assert np.count_nonzero(want) > TILE // 2


@pytest.mark.parametrize("c", CASES, ids=lambda c: c.id)
def test_impulses_bit_for_bit(c):
    L, M, D, _, H, T = rr.params(c.ri, c.ro)
    window = -(-(TILE - 1) * M // L) + T
    assert (T, window, window <= WINDOW) == TABLE[(c.ri, c.ro)]
    run_impulses(c)


# ---- noise against fp64

def bar64(x, c, n_out, chunk=None):
    """(ref64, gamma_T sum |w| |x|) for the outputs 0 .. n_out - 1, evaluated `chunk` outputs at a time"""
    T = rr.params(c.ri, c.ro)[5]
    step = chunk or max(n_out, 1)
    ref, mass = [], []
    for a in range(0, n_out, step):
        b = min(n_out, a + step)
        ref.append(rr.stage64(x, c.ri, c.ro, c.d_in, c.d_out, b, first=a))
        mass.append(rr.stage64(x, c.ri, c.ro, c.d_in, c.d_out, b, absolute=True, first=a))
    return np.concatenate(ref, axis=1), rr.gamma(T) * np.concatenate(mass, axis=1)


def against_fp64(got, x, c, tag, chunk=None):
    T = rr.params(c.ri, c.ro)[5]
    ref, bound = bar64(x, c, got.shape[1], chunk)
    diff = np.abs(got.astype(np.float64) - ref)
    ratio = float(np.max(diff / np.maximum(bound, 1e-300)))
    print(f"rate stage {c.ri} -> {c.ro} (T = {T}, d_in {c.d_in}, d_out {c.d_out}): max |out - ref64| / (gamma_T sum |w||x|) = {ratio:.5f}")
    errlog.bound(ratio, 1.0 + 1e-12, tag)
    assert np.all(diff <= bound)


@pytest.mark.parametrize("c", CASES, ids=lambda c: c.id)
def test_noise_against_fp64(c):
    S, wide = 2, c.ri == 640
    N = 190000 if wide else ring(c) + 3000
    cuts = cuts_for(N, c.max_in)
    assert N > ring(c)
    x = noise(S, N, c.ri + c.ro)
    rs = stage(S, c.ri, c.ro, c.d_in, c.d_out, c.max_in)
    got = feed(rs, x, cuts)
    rs.close()
    assert got.shape == (S, rr.ready(N, c.ri, c.ro, c.d_in, c.d_out)) and got.shape[1] > TILE
    against_fp64(got, x, c, f"rate_wide_{c.ri}_{c.ro}", chunk=32 if wide else None)


# ---- the cut and the reset, on the in-place form

CUT_RAGGED = (1, 7, 1024, 255, 1000, 17, 1024, 1024, 1024, 624)            # 6000 frames through a ring of 4096 slots


@pytest.mark.parametrize("S", [3, 65])
@pytest.mark.parametrize("c", [CASES[3], CASES[2]], ids=lambda c: c.id)
def test_the_bits_do_not_depend_on_the_cut_in_place(S, c):
    N = sum(CUT_RAGGED)
    assert not TABLE[(c.ri, c.ro)][2] and ring(c._replace(max_in=1024)) == 4096 < N
    x = noise(S, N, S)

    def run(x, cuts, max_in, reset=None):
        rs = stage(S, c.ri, c.ro, c.d_in, c.d_out, max_in)
        y = feed(rs, x, cuts, reset=reset)
        rs.close()
        return y
    whole, ragged = run(x, (N,), N), run(x, CUT_RAGGED, 1024)               # (the whole call: two tiles)
    assert whole.shape == ragged.shape and whole.shape[1] > TILE and np.array_equal(whole.view(np.uint32), ragged.view(np.uint32))
    # stream 1 reset after 2287 frames = a run whose stream 1 had zeros before that point
    at = sum(CUT_RAGGED[:5])
    with_reset = run(x, CUT_RAGGED, 1024, reset=(1, at))
    z = x.copy()
    z[1, :at] = 0.0
    zeros_before = run(z, CUT_RAGGED, 1024)
    done = rr.ready(at, c.ri, c.ro, c.d_in, c.d_out)                        # outputs taken before the reset keep the true past
    assert 0 < done < ragged.shape[1]
    assert np.array_equal(with_reset[:, :done], ragged[:, :done])
    assert np.array_equal(with_reset[:, done:].view(np.uint32), zeros_before[:, done:].view(np.uint32))
    assert not np.array_equal(with_reset[1, done:], ragged[1, done:]) and np.array_equal(with_reset[0], ragged[0])


# ---- the two forms (test build only)

RAGGED = (1, 7, 64, 255, 256, 17)                                          # 600 frames


@pytest.mark.parametrize("S", [3, 65])
@pytest.mark.parametrize("ri,ro,d_in,d_out", [(44100, 48000, 32, 0), (192000, 44100, 5, 3)])
def test_the_two_forms_give_the_same_bits(monkeypatch, S, ri, ro, d_in, d_out):
    """aidax_resample.hip: "whether a frame comes from LDS, the ring or the new block does not touch its bits". Nothing in the outputs
    tells the forms apart, so the test first makes sure that the library it runs on reads the switch at all: the name is among the
    strings of the test build and of no other (a library named through AIDAX_LIB that lacks it would pass by running one form twice)."""
    monkeypatch.setenv("AIDAX_RS_STAGED", "0")                              # (the ship leg skips here)
    with open(os.environ["AIDAX_LIB"], "rb") as f:
        assert b"AIDAX_RS_STAGED" in f.read(), "the library under test has no test hooks: the in-place form cannot be forced"
    x = noise(S, sum(RAGGED), S + ri)
    out = []
    for force in (True, False):
        if force:
            monkeypatch.setenv("AIDAX_RS_STAGED", "0")                      # k_resample<false> at a ratio whose window fits
        else:
            monkeypatch.delenv("AIDAX_RS_STAGED")
        rs = stage(S, ri, ro, d_in, d_out, 256)
        out.append(feed(rs, x, RAGGED))
        rs.close()
    assert out[0].shape == (S, rr.ready(sum(RAGGED), ri, ro, d_in, d_out)) and np.abs(out[0]).max() > 0.1
    assert np.array_equal(out[0].view(np.uint32), out[1].view(np.uint32))


# ---- edges of the launch

def test_65535_streams():
    """the largest grid.y. d_in = H = 32 (the adapter's stage A), so that 19 frames give outputs at all"""
    S, c = 65535, Case(48000, 96000, 32, 0, 8, None, False)
    src = noise(97, 19, 97)
    x = src[np.arange(S) % 97]
    rs = stage(S, c.ri, c.ro, c.d_in, c.d_out, c.max_in)
    got = feed(rs, x, (8, 3, 8))
    rs.close()
    assert got.shape == (S, 38)
    assert np.array_equal(got.view(np.uint32), got[:97][np.arange(S) % 97].view(np.uint32))
    against_fp64(got[:97], src, c, "rate_wide_65535_streams")


def test_delays_longer_than_the_ring():
    c, S = DELAYED, 3
    assert ring(c) == 256 < min(c.d_in, c.d_out)
    rest_cuts = (1, 7, 64, 33, 64, 17, 64, 64, 64, 64, 64)
    N = 64 + sum(rest_cuts)
    x = noise(S, N, 1700)
    rs = stage(S, c.ri, c.ro, c.d_in, c.d_out, c.max_in)
    assert rs.process(x[:, :64], 0).shape == (S, 0)
    ready = rs.ready
    # 1824 = d_out + ceil((64 - H + d_in) L / M) = 700 + 1124: the 700 outputs that d_out puts in front read only the zeros before the
    # stream, the next 1124 have their inputs among (or before) the 64 frames
    assert ready == rr.ready(64, c.ri, c.ro, c.d_in, c.d_out) and ready == 1824 and ready - c.d_out == 1124
    assert c.cap == -(-(c.max_in + 65) * 160 // 147) + 2 == 143
    with pytest.raises(ax.AidaxError) as e:
        rs.process(x[:, :0], c.cap + 1)
    assert e.value.code == ERR_ARG and "the blocking call takes at most 143" in str(e.value)
    assert rs.ready == ready                                                # the refused call changed nothing
    got = [rs.process(x[:, :0], min(c.cap, ready - a)) for a in range(0, ready, c.cap)]
    assert rs.ready == 0
    rest = feed(rs, x, rest_cuts, cap=c.cap, at=64, taken=ready)
    rs.close()
    got = np.concatenate(got + [rest], axis=1)
    assert got.shape == (S, rr.ready(N, c.ri, c.ro, c.d_in, c.d_out))
    against_fp64(got, x, c, "rate_wide_delays")


def test_impulses_at_delays_longer_than_the_ring():
    run_impulses(DELAYED)


# ---- the adapter with an in-place leg: a host at 8 kHz around a pool at 192 kHz

HOST, POOL_RATE = 8000, 192000
HOST_BLOCKS = (8, 1, 0, 10, 3, 10, 10)


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    p = str(tmp_path_factory.mktemp("rate_wide") / "lstm16.json")
    modelgen.write_model(modelgen.make_model(kind="lstm", hidden=16, input_size=1, seed=5), p)
    return ax.Model(p)


def test_the_adapter_with_an_in_place_leg_is_its_parts(model):
    """leg A, 8000 -> 192000 (L = 24), is staged; leg B, 192000 -> 8000, reads in place"""
    L, M, D, _, H, T = rr.params(HOST, POOL_RATE)
    assert (L, M) == (24, 1) and -(-(TILE - 1) * M // L) + T <= WINDOW and not TABLE[(POOL_RATE, HOST)][2]
    assert max(rr.pool_frames(HOST_BLOCKS, HOST, POOL_RATE)) == 240
    got, want, p1, ad, p2 = adapter_and_its_parts(model, None, HOST_BLOCKS, S=5, host=HOST, pool_rate=POOL_RATE, max_frames=10, pool_max=256)
    assert ad.latency_frames == 65 == rr.latency(HOST, POOL_RATE)
    print(f"rate adapter {HOST} -> {POOL_RATE} -> {HOST}: max |out| = {np.abs(want).max():.3e}")
    assert got.shape == (5, sum(HOST_BLOCKS)) and np.abs(want).max() > 1e-3
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    ad.close()
    p1.close()
    p2.close()


def test_the_adapter_with_an_in_place_leg_around_a_transparent_pool(model):
    S = 3
    p = pool(model, S, 256, ax.default_controls(enabled=0.0), rate=POOL_RATE)
    ad = ax.RateAdapter(p, float(HOST), 10)
    assert ad.latency_frames == 65
    x = noise(S, sum(HOST_BLOCKS), HOST)
    got, at = [], 0
    for n in HOST_BLOCKS:
        got.append(ad.process(np.ascontiguousarray(x[:, at:at + n])))
        at += n
    ad.close()
    p.close()
    got = np.concatenate(got, axis=1)
    ref, bound = rr.adapter64(x, HOST, POOL_RATE, rel=rr.gamma)
    diff = np.abs(got.astype(np.float64) - ref)
    ratio = float(np.max(diff / np.maximum(bound, 1e-300)))
    print(f"rate adapter {HOST} -> {POOL_RATE} -> {HOST}: max |out - B64(A64(x))| / bound = {ratio:.5f}")
    errlog.bound(ratio, 1.0 + 1e-12, "rate_wide_adapter_8000")
    assert np.all(diff <= bound) and np.abs(ref).max() > 0.0
