"""GPU parity tests (run with -m gpu on an MI355X): the HIP path, called through
the C ABI, against the CPU oracle on the same seeded inputs, against the
committed golden fixtures, and through size-independent properties at the
BASELINE.json sizes.

Bars (north_star):
  * biquads / smoothers / pure chain (no NN in circuit): bit-exact (fp64 IIR and
    fp32 recurrences are evaluated operation for operation like the reference);
  * anything through the NN: max-abs <= 1e-5 * max(1, downstream linear gain)
    (TEST_MODEL_THR, rt-neural-generic.h:182 — the reference applies it with
    gains forced to 1).
"""
import importlib
import json
import os

import numpy as np
import pytest

from oracle import oracle as O
from tests import errlog, modelgen

pytestmark = pytest.mark.gpu

ax = importlib.import_module("aidadsp-lv2_amd")
THR = 1.0e-5          # the reference's own bar (TEST_MODEL_THR). The bounds below sit at ~10x the errors measured on
                      # MI355X (gpurun_out/parity_errors.json via tests/errlog.py: 7e-8 .. 3.6e-7), so a 100x regression fails.


def _model_file(tmp_path, name, **kw):
    j = modelgen.make_model(**kw)
    p = str(tmp_path / f"{name}.json")
    modelgen.write_model(j, p)
    return p, O.parse_model(j)


def _ctl_pair(**kw):
    return ax.default_controls(**kw), O.default_controls(**kw)


def _canon(kernel_name):
    """Stacked models run on k_mfma_ls (contractions as bf16 term products) where their split fragments fit the register file,
    else on k_mfma_lp (fp32 MFMAs; AIDAX_LP_SPLIT=0 forces it): the same launch forms, named alike here."""
    return kernel_name.replace("k_mfma_ls", "k_mfma_lp").replace("k_conv_ms", "k_conv_mfma").replace("k_conv_st", "k_conv_mfma")      # (... and the conv stacks k_conv_ms admits run there, bf16 term products too; full blocks of the eight-layer stack as a stream of tiles: k_conv_st)


def _run_gpu(pool, x, block):
    out = np.empty_like(x)
    for b in range(0, x.shape[1], block):
        out[:, b:b + block] = pool.process(np.ascontiguousarray(x[:, b:b + block]))
    return out


# ------------------------------------------------------------- reference goldens

def test_bundled_models_self_test_on_gpu(bundled_models):
    """testModel (rt-neural-generic.cpp:900-955) on the GPU for all six bundled models."""
    for path in bundled_models:
        m = ax.Model(path)
        n_err, max_err, out = m.self_test()
        assert n_err == 0 and max_err < THR, (path, n_err, max_err)
        spec = O.load_model(path)
        ref = O.OracleModel(spec, warmup=False).test_model(spec.input_batch, spec.output_batch)[2]
        errlog.bound(np.abs(out - ref).max(), 4e-6, "gpu_parity:57")


@pytest.mark.parametrize("name", sorted(modelgen.GOLDEN_CASES))
def test_torch_goldens_on_gpu(name, golden_dir, tmp_path):
    kw = modelgen.GOLDEN_CASES[name]
    g = np.load(os.path.join(golden_dir, f"nn_{name}.npz"))
    path, spec = _model_file(tmp_path, name, **kw)
    y = ax.Model(path).forward(g["X"], unit_gains=True)
    skip = g["X"][:, 0] if kw.get("in_skip") else 0.0      # fixtures hold the bare network; applyModel adds x
    errlog.bound(np.abs(y - (g["y"] + skip)).max(), 2e-6, "gpu_parity:67")
    errlog.bound(np.abs(y - (O.net_run(spec, g["X"]) + skip)).max(), 2e-6, "gpu_parity:68")


@pytest.mark.parametrize("form", ["registers", "mfma", "quad"])
@pytest.mark.parametrize("cell", ["lstm", "gru"])
@pytest.mark.parametrize("hidden", modelgen.HIDDEN_SIZES)
def test_every_reference_variant_runs_and_matches_oracle(cell, hidden, form, tmp_path, monkeypatch):
    """All 54 architectures of model_variant.hpp, bare network, 768 samples each - on the register-resident
    kernels and on the two matrix-core kernels (16 streams per workgroup on mfma_16x16x4, zero-padded to a
    multiple of 16 units; 4 streams per workgroup on mfma_4x4x1)."""
    if form != "registers":
        monkeypatch.setenv("AIDAX_KERNEL", form)
    for isz in modelgen.INPUT_SIZES:
        kw = dict(kind=cell, hidden=hidden, input_size=isz, seed=1000 + hidden * 4 + isz)
        path, spec = _model_file(tmp_path, f"{cell}{hidden}_{isz}", **kw)
        X = modelgen.golden_inputs(f"{cell}{hidden}_{isz}", isz)[:768]
        y = ax.Model(path).forward(X, unit_gains=True)
        ref = O.net_run(spec, X)
        errlog.bound(np.abs(y - ref).max(), 2e-6, "gpu_parity:86")


# ------------------------------------------------------------------ pure DSP chain

def test_chain_without_model_is_silent_and_with_loading_cleared_is_bit_exact():
    x = modelgen.signal(5, 1024, seed=3)
    pool = ax.Pool(5, 256)
    assert np.all(_run_gpu(pool, x, 256) == 0.0)           # loading=true, master mem cleared to 0
    cg, co = _ctl_pair(bass_boost_db=4.0, mid_boost_db=-3.0, mid_freq=750.0, mid_q=1.2, treble_boost_db=2.0,
                       depth_boost_db=3.0, presence_boost_db=3.0, pregain_db=6.0, master_db=-4.5)
    pool = ax.Pool(5, 256)
    pool.set_loading(False)
    pool.set_controls(cg)
    got = _run_gpu(pool, x, 256)
    want = np.empty_like(x)
    for s in range(5):
        p = O.OraclePlugin()
        p.set_loading(False)
        for b in range(0, 1024, 256):
            want[s, b:b + 256] = p.run(co, x[s, b:b + 256])
    assert np.array_equal(got, want)                        # fp64 biquads + fp32 ramps: bit for bit


@pytest.mark.parametrize("kw", [
    dict(eq_position=1.0, bass_boost_db=-6.0, bass_freq=120.0, mid_boost_db=8.0, mid_freq=2500.0, mid_q=4.0,
         treble_boost_db=-8.0, treble_freq=3500.0, depth_boost_db=-8.0, presence_boost_db=8.0),
    dict(mid_type=1.0, mid_freq=900.0, mid_q=2.5, mid_boost_db=5.0, bass_boost_db=8.0),
    dict(eq_position=1.0, mid_type=1.0, mid_freq=400.0, mid_q=0.2),
    dict(eq_bypass=1.0, dc_blocker=0.0, in_lpf_pc=0.0),
    dict(in_lpf_pc=100.0, dc_blocker=0.0, pregain_db=-12.0, master_db=15.0),
    dict(in_lpf_pc=1.0, pregain_db=12.0, master_db=-15.0),
    dict(pregain_db=-95.0),                                   # DB_CO floor -> 0
])
def test_chain_control_corners_bit_exact(kw):
    x = modelgen.signal(3, 512, seed=11)
    cg, co = _ctl_pair(**kw)
    pool = ax.Pool(3, 128)
    pool.set_loading(False)
    pool.set_controls(cg)
    got = _run_gpu(pool, x, 128)
    want = np.empty_like(x)
    for s in range(3):
        p = O.OraclePlugin()
        p.set_loading(False)
        for b in range(0, 512, 128):
            want[s, b:b + 128] = p.run(co, x[s, b:b + 128])
    assert np.array_equal(got, want), kw


def test_ragged_and_tiny_blocks_and_prerun_bit_exact():
    """Block sizes that are not multiples of 4 or 64, single frames, and the
    n_samples == 0 pre-run (rt-neural-generic.cpp:606-609)."""
    sizes = [1, 3, 64, 0, 7, 129, 255, 256, 2, 0, 31]
    x = modelgen.signal(2, sum(sizes), seed=5)
    cg, co = _ctl_pair(bass_boost_db=3.0, pregain_db=2.0)
    pool = ax.Pool(2, 256)
    pool.set_loading(False)
    pool.set_controls(cg)
    plugs = [O.OraclePlugin() for _ in range(2)]
    for p in plugs:
        p.set_loading(False)
    pos = 0
    for n in sizes:
        blk = np.ascontiguousarray(x[:, pos:pos + n])
        got = pool.process(blk)
        for s in range(2):
            want = plugs[s].run(co, blk[s])
            assert np.array_equal(got[s], want), (n, s)
        pos += n


def test_per_stream_controls_and_disable_bypass(bundled_models):
    spec = O.load_model(bundled_models[4])
    m = ax.Model(bundled_models[4])
    S = 6
    x = modelgen.signal(S, 768, seed=21)
    pool = ax.Pool(S, 256)
    pool.set_model(m)
    kws = [dict(), dict(enabled=0.0), dict(net_bypass=1.0), dict(master_db=6.0, pregain_db=-3.0),
           dict(eq_position=1.0, bass_boost_db=5.0), dict(dc_blocker=0.0, mid_type=1.0)]
    for s, kw in enumerate(kws):
        pool.set_controls(ax.default_controls(**kw), stream=s)
    got = _run_gpu(pool, x, 256)
    for s, kw in enumerate(kws):
        want = O.run_streams(spec, O.default_controls(**kw), x[s:s + 1], 256)[0]
        if kw.get("enabled") == 0.0 or kw.get("net_bypass") == 1.0:
            assert np.array_equal(got[s], want), kw          # no NN in circuit
        else:
            errlog.bound(np.abs(got[s] - want).max(), 4e-6, "gpu_parity:175")


# ------------------------------------------------------------------ full chain

def _chain_case(tmp_path, name, model_kw, ctl_kw, S=4, n=2048, block=256, warm=True, tol=2e-6):
    path, spec = _model_file(tmp_path, name, **model_kw)
    m = ax.Model(path)
    x = modelgen.signal(S, n, seed=77)
    cg, co = _ctl_pair(**ctl_kw)
    pool = ax.Pool(S, block)
    pool.set_model(m, ax.START_WARMUP if warm else ax.START_RESET)
    pool.set_controls(cg)
    got = _run_gpu(pool, x, block)
    want = O.run_streams(spec, co, x, block, warmup=warm)
    err = np.abs(got - want).max()
    errlog.bound(err, tol, "gpu_parity:191")
    return pool, spec, got, want


def test_cfg2_lstm32_default_controls(tmp_path):
    _chain_case(tmp_path, "cfg2", dict(kind="lstm", hidden=32, input_size=1, seed=32), {}, S=8, n=4096)


def test_lstm32_skip_and_gains(tmp_path):
    _chain_case(tmp_path, "skip", dict(kind="lstm", hidden=32, input_size=1, seed=33, in_skip=1, in_gain=-3.0, out_gain=4.5),
                dict(master_db=3.0), tol=2e-6)


def test_cfg3_gru64_conditioned_eq_post(tmp_path):
    """BASELINE cfg #3: GRU-64, 2 params ramping, 5-band EQ post, DC blocker, default LPF."""
    path, spec = _model_file(tmp_path, "cfg3", kind="gru", hidden=64, input_size=3, seed=64)
    m = ax.Model(path)
    S, n, block = 4, 3072, 256
    x = modelgen.signal(S, n, seed=64)
    eq = dict(bass_boost_db=4.0, bass_freq=305.0, mid_boost_db=-3.0, mid_freq=750.0, mid_q=1.2,
              treble_boost_db=2.0, treble_freq=2000.0, depth_boost_db=3.0, presence_boost_db=3.0)
    pool = ax.Pool(S, block)
    pool.set_model(m)
    plugs = []
    for s in range(S):
        p = O.OraclePlugin()
        p.set_model(O.OracleModel(spec))
        plugs.append(p)
    got = np.empty_like(x)
    want = np.empty_like(x)
    for bi, b in enumerate(range(0, n, block)):
        t = bi / (n // block - 1)
        kw = dict(eq, param1=float(t), param2=float(1.0 - 0.7 * t))        # PARAM1 0->1, PARAM2 1->0.3
        pool.set_controls(ax.default_controls(**kw))
        got[:, b:b + block] = pool.process(np.ascontiguousarray(x[:, b:b + block]))
        for s in range(S):
            want[s, b:b + block] = plugs[s].run(O.default_controls(**kw), x[s, b:b + block])
    err = np.abs(got - want).max()
    errlog.bound(err, 1.5e-6, "gpu_parity:229")


def test_cfg1_bundled_lstm12_one_stream_full_chain(bundled_models):
    path = [p for p in bundled_models if "california_clean" in p][0]         # the TTL default model
    spec = O.load_model(path)
    x = modelgen.signal(1, 4096, seed=1)
    pool = ax.Pool(1, 256)
    pool.set_model(ax.Model(path))
    got = _run_gpu(pool, x, 256)
    want = O.run_streams(spec, O.default_controls(), x, 256)
    errlog.bound(np.abs(got - want).max(), 4e-6, "gpu_parity:240")


def test_warmup_state_matches_oracle_and_reset_mode_is_zero(bundled_models):
    spec = O.load_model(bundled_models[2])
    m = ax.Model(bundled_models[2])
    pool = ax.Pool(2, 64)
    pool.set_model(m, ax.START_WARMUP)
    h, c = pool.read_state(1)
    oh, oc = O.OracleModel(spec, warmup=True).state()
    assert np.abs(h - oh).max() < 4e-6 and np.abs(c - oc).max() < 4e-6 and np.abs(oh).max() > 1e-3
    pool.set_model(m, ax.START_RESET)
    h, c = pool.read_state(0)
    assert np.all(h == 0) and np.all(c == 0)


@pytest.mark.parametrize("kind,hidden", [("lstm", 64), ("gru", 80), ("lstm", 80)])
def test_read_state_of_a_quad_pool(kind, hidden, tmp_path):
    """LSTM-64 / LSTM-80 / GRU-80 pools run on k_quad at every stream count; their state (h | c, the table kernels'
    layout) is readable like any other pool's and matches the oracle after warm-up + one block."""
    path, spec = _model_file(tmp_path, f"{kind}{hidden}", kind=kind, hidden=hidden, input_size=1, seed=hidden + 3)
    pool = ax.Pool(5, 128)
    pool.set_model(ax.Model(path), ax.START_WARMUP)
    assert pool.kernel_name == "k_chain+k_quad"
    h, c = pool.read_state(3, hidden=128)
    om = O.OracleModel(spec, warmup=True)
    oh, oc = om.state()
    assert h.size == hidden and np.abs(oh).max() > 1e-4
    errlog.bound(np.abs(h - oh).max(), 2e-6, "gpu_parity:quad_state_h")
    if kind == "lstm":
        errlog.bound(np.abs(c - oc).max(), 2e-6, "gpu_parity:quad_state_c")
    with pytest.raises(ax.AidaxError):
        pool.read_state(3, layer=1)


def test_activate_and_model_swap_semantics(tmp_path, bundled_models):
    """activate() clears the gain ramps to their targets and re-arms paramFirstRun
    (:337-351); a model swap inherits the param targets (:822-825, :1053-1061)."""
    pa, spec_a = _model_file(tmp_path, "a", kind="gru", hidden=16, input_size=2, seed=5)
    pb, spec_b = _model_file(tmp_path, "b", kind="lstm", hidden=20, input_size=3, seed=6)
    x = modelgen.signal(2, 1024, seed=9)
    pool = ax.Pool(2, 128)
    plugs = [O.OraclePlugin() for _ in range(2)]
    pool.set_model(ax.Model(pa))
    for p in plugs:
        p.set_model(O.OracleModel(spec_a))
    script = [(0, dict(param1=0.8, pregain_db=6.0)), (2, "activate"), (3, dict(param1=0.2, param2=0.9, master_db=-6.0)),
              (4, "swap"), (5, dict(param1=0.6, param2=0.1)), (6, "activate")]
    kw = {}
    for bi, b in enumerate(range(0, 1024, 128)):
        for at, ev in script:
            if at != bi:
                continue
            if ev == "activate":
                pool.activate()
                for p in plugs:
                    p.activate()
            elif ev == "swap":
                pool.set_model(ax.Model(pb))
                for p in plugs:
                    old = (p.model.ptr.contents.param1Coeff.target, p.model.ptr.contents.param2Coeff.target)
                    p.set_model(O.OracleModel(spec_b, old[0], old[1]))
            else:
                kw = ev
        pool.set_controls(ax.default_controls(**kw))
        got = pool.process(np.ascontiguousarray(x[:, b:b + 128]))
        for s in range(2):
            want = plugs[s].run(O.default_controls(**kw), x[s, b:b + 128])
            errlog.bound(np.abs(got[s] - want).max(), 1.5e-6, "gpu_parity:289")


@pytest.mark.parametrize("first,env", [
    (dict(kind="lstm", hidden=16, input_size=1, seed=3), {}),                             # table kernel, no PARAM input
    (dict(kind="conv", hidden=16, input_size=1, seed=4), {}),                             # k_conv_ms, chain passes inside
    (dict(kind="conv", hidden=16, input_size=1, seed=4), {"AIDAX_CONV_FUSED": "0"}),      # k_chain + k_conv_ms + k_chain
    (dict(kind="conv", hidden=16, input_size=1, seed=4), {"AIDAX_CONV_MS": "0"}),         # k_conv_mfma (fp32 MFMAs)
    (dict(kind="conv", hidden=16, input_size=1, seed=4), {"AIDAX_KERNEL": "valu"}),       # k_conv
    (dict(kind="lstm", hidden=32, input_size=1, seed=5, n_rnn=2), {}),                    # k_mfma_lp
])
def test_param_targets_follow_the_controls_under_a_model_without_param_inputs(first, env, tmp_path, monkeypatch):
    """run() sets the PARAM smoothers' targets and serves paramFirstRun for EVERY model (:634-640), also one whose
    forward() takes the audio only; a conditioned model swapped in later starts its ramps from what the playing
    model holds then (:822-825). PARAM1/2 move while the first model plays, then the swap: the second model's
    first blocks ramp from those values (a stale target shows as a 0.1 s ramp error of ~1e-2)."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    pa, spec_a = _model_file(tmp_path, "first", **first)
    pb, spec_b = _model_file(tmp_path, "second", kind="gru", hidden=16, input_size=3, seed=6)
    x = modelgen.signal(3, 1536, seed=10)
    pool = ax.Pool(3, 128)
    plugs = [O.OraclePlugin() for _ in range(3)]
    pool.set_model(ax.Model(pa))
    for p in plugs:
        p.set_model(O.OracleModel(spec_a))
    script = {1: dict(param1=0.8, param2=0.3), 3: "activate", 4: dict(param1=0.1, param2=0.9, net_bypass=1.0),
              5: dict(param1=0.45, param2=0.65), 6: "swap", 9: dict(param1=0.7, param2=0.2)}
    kw = {}
    for bi, b in enumerate(range(0, 1536, 128)):
        ev = script.get(bi)
        if ev == "activate":
            pool.activate()
            for p in plugs:
                p.activate()
        elif ev == "swap":
            pool.set_model(ax.Model(pb))
            for p in plugs:
                old = (p.model.ptr.contents.param1Coeff.target, p.model.ptr.contents.param2Coeff.target)
                p.set_model(O.OracleModel(spec_b, old[0], old[1]))
        elif ev is not None:
            kw = ev
        pool.set_controls(ax.default_controls(**kw))
        got = pool.process(np.ascontiguousarray(x[:, b:b + 128]))
        for s in range(3):
            want = plugs[s].run(O.default_controls(**kw), x[s, b:b + 128])
            errlog.bound(np.abs(got[s] - want).max(), 2e-6, "gpu_parity:param_targets")


def test_worker_thread_prepares_while_the_audio_thread_processes(tmp_path):
    """The two-thread contract of a model swap with the threads REALLY concurrent: a worker thread prepares model after
    model (pack, allocate, upload, warm up on the pool's worker stream) and frees what the swaps retire, while the
    audio thread processes block after block and commits whatever the worker has ready at a block boundary — table
    kernels, the stacked matrix-core kernel with its hand-over ring, the conv stack. PARAM controls rest, so what a
    new model inherits does not depend on when its preparation ran; every block of every stream against the oracle."""
    import queue
    import threading
    kinds = [dict(kind="lstm", hidden=16, input_size=1, seed=51), dict(kind="gru", hidden=24, input_size=2, seed=52),
             dict(kind="lstm", hidden=32, input_size=1, seed=53, n_rnn=2), dict(kind="conv", hidden=16, input_size=1, seed=54)]
    files = [_model_file(tmp_path, f"m{i}", **kw) for i, kw in enumerate(kinds)]
    models = [ax.Model(p) for p, _ in files]
    S, n, blocks = 6, 128, 640               # (at least 160 blocks; more while the worker has not got eight swaps in — how
    x = modelgen.signal(S, n * blocks, seed=71)     # many it manages per block depends on how loaded the box is)
    ckw = dict(param1=0.35, pregain_db=2.0, bass_boost_db=3.0)
    cg, co = _ctl_pair(**ckw)
    pool = ax.Pool(S, n)
    pool.set_model(models[0])
    pool.set_controls(cg)
    plugs = [O.OraclePlugin() for _ in range(S)]
    for p in plugs:
        p.set_model(O.OracleModel(files[0][1]))
    ready, retired = queue.Queue(maxsize=1), queue.Queue()
    stop = threading.Event()
    failure = []

    def worker():
        try:
            k = 0
            while not stop.is_set():
                while not retired.empty():
                    pool.staged_free(retired.get())                 # waits for the passes that still read the old buffers
                mi = (1, 2, 3, 0, 2, 1, 3)[k % 7]
                sg = pool.prepare_model(models[mi])
                k += 1
                while not stop.is_set():
                    try:
                        ready.put((mi, sg), timeout=0.01)
                        break
                    except queue.Full:
                        pass
                else:
                    pool.staged_free(sg)
            while not retired.empty():
                pool.staged_free(retired.get())
        except Exception as e:                                      # pragma: no cover
            failure.append(e)

    t = threading.Thread(target=worker)
    swaps, names = 0, set()
    try:
        for b in range(blocks):
            if b == 1:
                # The worker starts once the first block has run: a prepared model inherits the PARAM targets the PLAYING model
                # holds at the time of its preparation (rt-neural-generic.cpp:1053-1061), and those are the controls' only after the
                # first run() has read the ports. (Started ahead of block 0, a host whose first prepare beats its first block —
                # two cores for both threads are enough — hands the new model targets of 0: 3e-3 off the oracle, decaying.)
                t.start()
            try:
                mi, sg = ready.get_nowait()
            except queue.Empty:
                mi = None
            if mi is not None:
                pool.commit_model(sg)                               # audio side: no allocation, no wait
                retired.put(sg)
                swaps += 1
                for p in plugs:
                    old = p.model.ptr.contents
                    p.set_model(O.OracleModel(files[mi][1], old.param1Coeff.target, old.param2Coeff.target))
            blk = np.ascontiguousarray(x[:, b * n:(b + 1) * n])
            got = pool.process(blk)
            names.add(pool.kernel_name)
            for s_ in range(S):
                want = plugs[s_].run(co, blk[s_])
                errlog.bound(np.abs(got[s_] - want).max(), 2e-6, "gpu_parity:concurrent_prepare")
            if b >= 159 and swaps >= 8 and len(names) >= 3:
                break
    finally:
        stop.set()
        if t.is_alive():
            t.join()
        while not ready.empty():
            pool.staged_free(ready.get()[1])
    assert not failure, failure
    assert swaps >= 8 and len(names) >= 3, (swaps, names)


def test_pools_of_one_process_on_several_threads(tmp_path):
    """Four pools (four kernel families, different stream counts) of one process, each driven by a thread of its own at
    full speed: nothing in the library is shared between pools but the device, so every pool must match its oracle
    as if it were alone (error strings are per thread, function attributes are idempotent)."""
    import threading
    cases = [("t_pipe", dict(kind="lstm", hidden=16, input_size=2, seed=61), 9, 128),
             ("t_split", dict(kind="gru", hidden=24, input_size=1, seed=62), 200, 64),
             ("t_lp", dict(kind="lstm", hidden=32, input_size=1, seed=63, n_rnn=2), 20, 256),
             ("t_conv", dict(kind="conv", hidden=16, input_size=1, seed=64), 6, 256)]
    made = [(_model_file(tmp_path, name, **kw), S, n) for name, kw, S, n in cases]
    failures, names = [], []
    blocks = 40

    def one(idx):
        try:
            (path, spec), S, n = made[idx]
            pool = ax.Pool(S, n)
            pool.set_model(ax.Model(path))
            cg, co = _ctl_pair(param1=0.3, pregain_db=1.0 + idx, bass_boost_db=2.0)
            pool.set_controls(cg)
            x = modelgen.signal(S, n * blocks, seed=80 + idx)
            got = _run_gpu(pool, x, n)
            names.append(pool.kernel_name)
            watch = [0, S // 2, S - 1]
            want = O.run_streams(spec, co, x[watch], n)
            err = float(np.abs(got[watch] - want).max())
            if err > 2e-6:
                failures.append((idx, err))
            pool.close()
        except Exception as e:                                      # pragma: no cover
            failures.append((idx, repr(e)))

    threads = [threading.Thread(target=one, args=(i,)) for i in range(len(cases))]
    for t in threads: t.start()
    for t in threads: t.join()
    assert not failures, failures
    assert len(set(names)) == 4, names


def test_long_run_drift_48000_samples(tmp_path):
    """One second of full-scale audio through LSTM-32: the fast sigmoid/tanh must hold
    1e-5 over >= 48000 recurrent steps (SURVEY §7 'Transcendentals at 1e-5')."""
    _chain_case(tmp_path, "drift", dict(kind="lstm", hidden=32, input_size=1, seed=32), {}, S=2, n=48128, block=256)



_EQ_POST = dict(bass_boost_db=4.0, mid_boost_db=-3.0, mid_q=1.2, treble_boost_db=2.0, depth_boost_db=3.0,
                presence_boost_db=3.0, param1=0.5, param2=0.3)


def _long_run(tmp_path, name, model_kw, S, distinct, kernel, tag, tol, n=48128, block=256, ramp=False, ckw=None):
    """>= one second of audio through a many-streams launch form: `distinct` different streams spread over a pool of S
    (neighbours in a workgroup carry different signals), every block against per-stream oracle plugins, controls moving
    from block to block when `ramp` (PARAM1 0 -> 1, PARAM2 1 -> 0.3 over the run). The reference's bar is 1e-5 on whatever
    the host plays (TEST_MODEL_THR, rt-neural-generic.h:182); the bound asserted is `tol`, the measured error is logged."""
    path, spec = _model_file(tmp_path, name, **model_kw)
    base = modelgen.signal(distinct, n, seed=404)
    idx = (np.arange(S) * 7) % distinct
    first = [int(np.argmax(idx == k)) for k in range(distinct)]        # one pool row per distinct stream
    pool = ax.Pool(S, block)
    pool.set_model(ax.Model(path))
    plugs = []
    for _ in range(distinct):
        p = O.OraclePlugin()
        p.set_model(O.OracleModel(spec))
        plugs.append(p)
    ckw = dict(ckw or {})
    worst, nblk = 0.0, n // block
    for bi in range(nblk):
        b = bi * block
        kw = dict(ckw)
        if ramp:
            t = bi / (nblk - 1)
            kw.update(param1=float(t), param2=float(1.0 - 0.7 * t))
        if ramp or bi == 0:
            pool.set_controls(ax.default_controls(**kw))
        got = pool.process(np.ascontiguousarray(base[idx, b:b + block]))
        if bi == 0:
            assert pool.kernel_name.startswith(kernel), pool.kernel_name
        co = O.default_controls(**kw)
        for k in range(distinct):
            want = plugs[k].run(co, base[k, b:b + block])
            worst = max(worst, float(np.abs(got[first[k]] - want).max()))
        if bi % 47 == 0:                                               # copies of a stream stay bitwise identical all the way
            for k in range(distinct):
                grp = got[idx == k]
                assert np.all(grp == grp[0]), (name, bi, k)
    pool.close()
    assert worst < THR, (name, worst)                                  # the reference's own bar, whatever else
    errlog.bound(worst, tol, tag)


def test_long_run_drift_gru64_conditioned_on_the_gate_major_kernel(tmp_path):
    """cfg3's kernel (k_gru_gs: gate-major tiles, recurrent product as six bf16 term products, candidate tanh in the
    four-instruction exp form) over 48 128 samples with both PARAM inputs ramping and the EQ in circuit: neither the exp
    form's absolute error nor the dropped 2^-24 term products may accumulate in h."""
    _long_run(tmp_path, "drift_gru64", dict(kind="gru", hidden=64, input_size=3, seed=64), S=4096, distinct=16,
              kernel="k_gru_gs", tag="gpu_parity:drift_gru64_gs", tol=4e-6, ramp=True, ckw=_EQ_POST)


def test_long_run_drift_gru64_on_the_fp32_gate_major_kernel(tmp_path, monkeypatch):
    """... and the same run on k_gru_gm (fp32 MFMAs, AIDAX_GRU_GM=f32), the kernel the split one is measured against."""
    monkeypatch.setenv("AIDAX_GRU_GM", "f32")
    _long_run(tmp_path, "drift_gru64f", dict(kind="gru", hidden=64, input_size=3, seed=64), S=4096, distinct=16,
              kernel="k_gru_gm", tag="gpu_parity:drift_gru64_gm", tol=4e-6, ramp=True, ckw=_EQ_POST)


def test_long_run_drift_lstm96x2_on_the_layer_pipelined_kernel(tmp_path):
    """cfg5's kernel (k_mfma_ls: two layers of 96 on separate workgroups, contractions as six bf16 term products) over 48 128
    samples at cfg5's pool size."""
    _long_run(tmp_path, "drift_lstm96x2", dict(kind="lstm", hidden=96, input_size=1, seed=96, n_rnn=2), S=2048, distinct=8,
              kernel="k_mfma_ls", tag="gpu_parity:drift_lstm96x2_ls", tol=4e-6)


def test_long_run_drift_lstm96x2_on_the_fp32_layer_pipelined_kernel(tmp_path, monkeypatch):
    """... and on k_mfma_lp (fp32 MFMAs, AIDAX_LP_SPLIT=0), the kernel the split one is measured against."""
    monkeypatch.setenv("AIDAX_LP_SPLIT", "0")
    _long_run(tmp_path, "drift_lstm96x2f", dict(kind="lstm", hidden=96, input_size=1, seed=96, n_rnn=2), S=2048, distinct=8,
              kernel="k_mfma_lp", tag="gpu_parity:drift_lstm96x2_lp", tol=4e-6)


def test_long_run_drift_lstm64_on_the_unit_major_split_kernel(tmp_path):
    """LSTM-64 at 4096 streams — where the pool picks k_lstm_gs by itself — over 48 128 samples with PARAM1 ramping."""
    _long_run(tmp_path, "drift_lstm64", dict(kind="lstm", hidden=64, input_size=2, seed=64), S=4096, distinct=8,
              kernel="k_lstm_gs", tag="gpu_parity:drift_lstm64_gs", tol=4e-6, ramp=True)


def test_long_run_drift_lstm64_on_the_lone_layer_split_kernel(tmp_path, monkeypatch):
    """... and on k_mfma_ls1 (AIDAX_LSTM_GS=0: a lone layer on k_mfma_ls's body), the kernel LSTM-80 / GRU-80 pools get."""
    monkeypatch.setenv("AIDAX_LSTM_GS", "0")
    _long_run(tmp_path, "drift_lstm64b", dict(kind="lstm", hidden=64, input_size=2, seed=64), S=4096, distinct=8,
              kernel="k_mfma_ls1", tag="gpu_parity:drift_lstm64_ls1", tol=4e-6, ramp=True)


def test_long_run_drift_small_gru_on_the_pipeline_kernel(tmp_path):
    """The three-wave pipeline's GRU cell (the exp-form candidate went into every GRU kernel) over 48 128 samples,
    PARAM1 ramping."""
    _long_run(tmp_path, "drift_gru16", dict(kind="gru", hidden=16, input_size=2, seed=16), S=1024, distinct=16,
              kernel="k_gru_pipe", tag="gpu_parity:drift_gru16_pipe", tol=4e-6, ramp=True)


# ------------------------------------------------------- properties at full size


@pytest.mark.parametrize("name,kw,S,ckw,kernel", [
    ("cfg2", dict(kind="lstm", hidden=32, input_size=1, seed=32), 1024, {}, "k_lstm_pipe4<32>"),
    ("cfg3", dict(kind="gru", hidden=64, input_size=3, seed=64), 4096, _EQ_POST, "k_gru_gs"),                     # one launch: gate-major tiles, the chain on the helper waves
    ("cfg4", dict(kind="conv", hidden=16, input_size=1, seed=1608), 1024, {}, "k_conv_st"),
    ("cfg5", dict(kind="lstm", hidden=96, input_size=1, seed=96, n_rnn=2), 2048, {}, "k_mfma_ls"),
    ("lstm80-1k", dict(kind="lstm", hidden=80, input_size=2, seed=80), 1024, dict(param1=0.7), "k_chain+k_quad"),
    ("lstm80-2k", dict(kind="lstm", hidden=80, input_size=2, seed=80), 2048, dict(param1=0.7), "k_mfma_ls1"),      # a lone layer on k_mfma_ls's body
    ("gru80-4k", dict(kind="gru", hidden=80, input_size=2, seed=81), 4096, dict(param1=0.7), "k_gru_gs"),           # five main waves, two helpers
    ("lstm40-4k", dict(kind="lstm", hidden=40, input_size=2, seed=40), 4096, dict(param1=0.7), "k_lstm_gs"),       # unit-major tiles, chain on helper waves
    ("lstm64-2k", dict(kind="lstm", hidden=64, input_size=3, seed=65), 2048, dict(param1=0.7, param2=0.1), "k_lstm_gs"),
    ("gru32-4k", dict(kind="gru", hidden=32, input_size=2, seed=33), 4096, dict(param1=0.7), "k_mfma_lp"),         # the fp32 one-launch form keeps what it wins
    ("gru16-4k", dict(kind="gru", hidden=16, input_size=3, seed=16), 4096, dict(param1=0.2, param2=0.9), "k_chain+k_quad"),
])
def test_full_size_properties(name, kw, S, ckw, kernel, tmp_path):
    """The BASELINE.json GPU configs at their per-GPU stream counts x 256 frames, in the launch form the
    pool picks at that size: identical streams give bitwise identical outputs wherever they sit in the
    launch (workgroup, wave, lane group), a permutation of the streams permutes the outputs (no
    cross-stream coupling), state carries across blocks, and the 16 distinct streams match the oracle."""
    path, spec = _model_file(tmp_path, name, **kw)
    m = ax.Model(path)
    block, nblk = 256, 3
    base = modelgen.signal(16, block * nblk, seed=2)
    idx = (np.arange(S) * 7) % 16                             # neighbours in a workgroup carry different signals
    x = base[idx]
    cg, co = _ctl_pair(**ckw)
    pool = ax.Pool(S, block)
    pool.set_model(m)
    pool.set_controls(cg)
    assert pool.kernel_name == kernel
    got = _run_gpu(pool, x, block)
    for k in range(16):                                       # identical inputs -> bitwise identical outputs
        grp = got[idx == k]
        assert np.all(grp == grp[0]), (name, k)
    perm = np.random.RandomState(0).permutation(S)
    pool.close()                                              # (one pool per device holds k_mfma_lp: the second must get the same kernel)
    pool2 = ax.Pool(S, block)
    pool2.set_model(m)
    pool2.set_controls(cg)
    got2 = _run_gpu(pool2, x[perm], block)
    assert np.array_equal(got2, got[perm])                    # no cross-stream coupling
    want = O.run_streams(spec, co, base, block)
    first = np.array([np.argmax(idx == k) for k in range(16)])
    err = np.abs(got[first] - want).max()
    errlog.bound(err, 1.5e-6, "gpu_parity:342")
    assert np.isfinite(got).all()


def test_device_resident_entry_point_matches_host_entry_point(tmp_path):
    import torch
    path, spec = _model_file(tmp_path, "dev", kind="lstm", hidden=32, input_size=1, seed=32)
    m = ax.Model(path)
    x = modelgen.signal(64, 512, seed=4)
    a = ax.Pool(64, 256)
    a.set_model(m)
    want = _run_gpu(a, x, 256)
    b = ax.Pool(64, 256)
    b.set_model(m)
    dx = torch.from_numpy(x).cuda()
    outs = []
    ts = torch.cuda.Stream()
    torch.cuda.set_stream(ts)
    stream = ts.cuda_stream
    for blk in range(2):
        din = dx[:, blk * 256:(blk + 1) * 256].contiguous()
        dout = torch.empty_like(din)
        b.process_device(din.data_ptr(), dout.data_ptr(), 256, stream)
        outs.append(dout)
    torch.cuda.synchronize()
    got = torch.cat(outs, dim=1).cpu().numpy()
    assert np.array_equal(got, want)


# ------------------------------------------------- extensions (parity unpinned by the reference)

@pytest.mark.parametrize("form", ["mfma", "valu", "split"])
@pytest.mark.parametrize("kind,kw", [
    ("lstm96x2", dict(kind="lstm", hidden=96, input_size=1, seed=96, n_rnn=2)),        # BASELINE cfg #5 model
    ("gru48x3", dict(kind="gru", hidden=48, input_size=2, seed=483, n_rnn=3)),
    ("conv16x8", dict(kind="conv", hidden=16, input_size=1, seed=1608)),                # BASELINE cfg #4 model
    ("conv8x4k5", dict(kind="conv", hidden=8, input_size=1, seed=85, conv_layers=4, conv_k=5)),
])
def test_extension_models_full_chain(kind, kw, form, tmp_path, monkeypatch):
    """Stacked recurrent layers and conv1d stacks through the full run() chain, 11 streams (not a
    multiple of the 8- or 16-stream workgroups), blocks shorter than the conv history, warm-up state.
    Both families run on their matrix-core kernel by default and on the VALU kernel with AIDAX_KERNEL=valu."""
    conv = kw["kind"] == "conv"
    if form == "valu":
        monkeypatch.setenv("AIDAX_KERNEL", "valu")
    if form == "split":                                       # conv stacks: packed k_chain launches around the conv kernel
        if not conv:
            pytest.skip("the stacked recurrent models have one matrix-core form")
        monkeypatch.setenv("AIDAX_CONV_FUSED", "0")
    path, spec = _model_file(tmp_path, kind, **kw)
    m = ax.Model(path)
    S, n, block = 11, 1536, 64
    x = modelgen.signal(S, n, seed=123)
    ckw = dict(bass_boost_db=3.0, treble_boost_db=-2.0, pregain_db=2.0, param1=0.4)
    cg, co = _ctl_pair(**ckw)
    pool = ax.Pool(S, 256)
    pool.set_model(m)
    mfma_name = ("k_chain+k_conv_mfma" if form == "split" else "k_conv_mfma") if conv else "k_mfma_lp"
    assert _canon(pool.kernel_name) == (("k_conv" if conv else "k_stack") if form == "valu" else mfma_name)
    pool.set_controls(cg)
    got = _run_gpu(pool, x, block)
    want = O.run_streams(spec, co, x, block)
    err = np.abs(got - want).max()
    errlog.bound(err, 1.5e-6, "gpu_parity:400")
    # block-size invariance on the device (history / state carried across launches)
    pool2 = ax.Pool(S, 256)
    pool2.set_model(m)
    pool2.set_controls(cg)
    got2 = _run_gpu(pool2, x, 256)
    errlog.bound(np.abs(got2 - got).max(), 1e-7, "gpu_parity:406")


@pytest.mark.parametrize("seed", range(8))
def test_random_conv_architectures(seed, tmp_path, monkeypatch):
    """Conv stacks drawn at random — 1..10 layers, 1..16 channels (all layers alike, as the kernels require), 1..8 taps,
    dilations that are NOT powers of two as well (history lengths that are no multiple of four take the scalar history
    path, the others the float4 one with shift or divide indexing), tanh / relu / sigmoid / linear layers, skip and
    gains — through the one-launch form, the split form and the VALU kernel against the oracle, ragged blocks."""
    rs = np.random.RandomState(900 + seed)
    C_, nl, k = int(rs.randint(1, 17)), int(rs.randint(1, 11)), int(rs.randint(1, 9))
    layers, cur = [], 1
    for l in range(nl):
        dil = int(rs.choice([1, 2, 3, 4, 5, 6, 8, 12, 16, 24, 32]))
        while (k - 1) * dil > 256:                       # the kernels keep at most 256 frames of history per layer... stay inside
            dil //= 2
        layers.append(modelgen.conv_layer(rs, cur, C_, k, max(dil, 1), str(rs.choice(["tanh", "tanh", "relu", "sigmoid", ""]))))
        cur = C_
    layers.append(modelgen.dense_layer(rs, C_))
    j = {"in_shape": [None, None, 1], "layers": layers, "metadata": {"name": f"random_conv_{seed}", "samplerate": "48000"},
         "in_skip": int(rs.randint(2)), "in_gain": float(rs.uniform(-3, 3)), "out_gain": float(rs.uniform(-3, 3))}
    path = modelgen.write_model(j, str(tmp_path / f"rc{seed}.json"))
    spec = O.parse_model(j)
    S = 5
    sizes = [256, 100, 1, 255, 0, 64, 256]
    x = modelgen.signal(S, sum(sizes), seed=300 + seed)
    cg, co = _ctl_pair(pregain_db=1.5, bass_boost_db=-2.0)
    want = O.run_streams(spec, co, x, 256)
    seen = set()
    for env, name in (({}, "k_conv_mfma"), ({"AIDAX_CONV_MS": "0"}, "k_conv_mfma"), ({"AIDAX_CONV_FUSED": "0"}, "k_chain+k_conv_mfma"), ({"AIDAX_KERNEL": "valu"}, "k_conv")):
        for k_, v in (("AIDAX_CONV_FUSED", None), ("AIDAX_KERNEL", None), ("AIDAX_CONV_MS", None)):
            monkeypatch.delenv(k_, raising=False)
        for k_, v in env.items():
            monkeypatch.setenv(k_, v)
        pool = ax.Pool(S, 256)
        pool.set_model(ax.Model(path))
        # (the stacks k_conv_ms admits — sixteen channels, two to four taps, histories its plane holds — run there unless AIDAX_CONV_MS=0)
        assert _canon(pool.kernel_name) == name, (pool.kernel_name, name, C_, nl, k)
        assert not ("k_conv_ms" in pool.kernel_name and env.get("AIDAX_CONV_MS") == "0")
        if pool.kernel_name in seen:
            pool.close()
            continue
        seen.add(pool.kernel_name)
        pool.set_controls(cg)
        got = np.empty_like(x)
        pos = 0
        for n in sizes:
            got[:, pos:pos + n] = pool.process(np.ascontiguousarray(x[:, pos:pos + n]))
            pos += n
        scale = max(1.0, float(np.abs(want).max()))
        errlog.bound(np.abs(got - want).max() / scale, 3e-6, "gpu_parity:random_conv")
        pool.close()


_MS_STACKS = [
    # (layer 0: taps, dilation), then (taps, dilation, activation) per sixteen-channel layer — what k_conv_ms admits (conv_ms_shape_ok), corners first
    ("cfg4-like", (3, 1), [(3, 2, "tanh"), (3, 4, "tanh"), (3, 8, "tanh"), (3, 16, "tanh"), (3, 32, "tanh"), (3, 64, "tanh"), (3, 128, "tanh")]),   # last layer: 256 frames back, beyond the plane
    ("cfg4 shape, mixed activations", (3, 1), [(3, 2, "relu"), (3, 4, "tanh"), (3, 8, "sigmoid"), (3, 16, ""), (3, 32, "tanh"), (3, 64, "relu"), (3, 128, "sigmoid")]),   # k_conv_st<false>: the activation switch left in
    ("two taps, one deep", (2, 3), [(2, 200, "relu"), (2, 1, "tanh")]),                                   # 200 frames back: tiles 0 .. 4 read the history in HBM
    ("four taps, two deep taps in one k-step", (4, 5), [(4, 85, "tanh"), (4, 1, "sigmoid"), (4, 7, "")]),      # shifts 255 / 170 share k-step 0: per-lane sources
    ("four taps, 64 apart", (1, 1), [(4, 64, "tanh"), (4, 42, "relu")]),                                 # shift 192: tiles 0 .. 3 deep; layer 0 with ONE tap
    ("odd dilations", (3, 8), [(3, 3, "tanh"), (3, 9, "tanh"), (3, 27, ""), (3, 81, "tanh"), (2, 127, "sigmoid")]),   # shifts that are no multiples of 16: unaligned reads
    ("history = the plane's", (2, 16), [(3, 64, "tanh"), (2, 128, "tanh"), (4, 42, "tanh")]),            # 128 frames back: the last in-plane frame
    # the other geometries k_conv_st is compiled for (aidax_layout.h StGeoB .. E): blocks of 64 / 128 / 256 frames stream, the rest runs k_conv_ms on the same state
    ("two cycles 1..16, two taps", (2, 1), [(2, d, "tanh") for d in (2, 4, 8, 16, 1, 2, 4, 8, 16)]),
    ("six layers, three taps", (3, 1), [(3, d, "tanh") for d in (2, 4, 8, 16, 32)]),
    ("two cycles 1..8, three taps, mixed activations", (3, 1), [(3, d, a) for d, a in zip((2, 4, 8, 1, 2, 4, 8), ("tanh", "relu", "tanh", "sigmoid", "", "tanh", "tanh"))]),
    ("cfg4's dilations, two taps", (2, 1), [(2, d, "tanh") for d in (2, 4, 8, 16, 32, 64, 128)]),         # one far tap (128 frames back) through the staging area
]
_ST_STACKS = ("cfg4-like", "cfg4 shape, mixed activations", "two cycles 1..16, two taps", "six layers, three taps",
              "two cycles 1..8, three taps, mixed activations", "cfg4's dilations, two taps")
_MS_SIZES = [256, 100, 1, 255, 0, 64, 256, 17, 128, 130, 3, 256, 64, 128, 64, 256]


def _ms_stack_model(name, l0, rest, tmp_path):
    import zlib
    rs = np.random.RandomState(zlib.crc32(name.encode()))
    layers = [modelgen.conv_layer(rs, 1, 16, l0[0], l0[1], "tanh")]
    for k, dil, act in rest:
        layers.append(modelgen.conv_layer(rs, 16, 16, k, dil, act))
    layers.append(modelgen.dense_layer(rs, 16))
    j = {"in_shape": [None, None, 1], "layers": layers, "metadata": {"name": name, "samplerate": "48000"},
         "in_skip": 1, "in_gain": -1.0, "out_gain": 2.0}
    return modelgen.write_model(j, str(tmp_path / "ms.json")), O.parse_model(j)


@pytest.mark.parametrize("name,l0,rest", _MS_STACKS, ids=[s[0] for s in _MS_STACKS])
def test_conv_stacks_as_the_pool_runs_them(name, l0, rest, tmp_path):
    """The same corner stacks with no switch set — the kernels a host gets (and the ship leg's copy of this test the shipped library's):
    k_conv_st for the blocks of 64 / 128 / 256 frames of the stacks with a compiled geometry, k_conv_ms for every other block and stack,
    one state under both (every strip of a layer's history a ring over time: ragged blocks in between leave the rings at any phase)."""
    path, spec = _ms_stack_model(name, l0, rest, tmp_path)
    S = 6
    x = modelgen.signal(S, sum(_MS_SIZES), seed=41)
    cg, co = _ctl_pair(pregain_db=1.0, treble_boost_db=2.0)
    want = O.run_streams(spec, co, x, 256)
    scale = max(1.0, float(np.abs(want).max()))
    m = ax.Model(path)
    assert m.conv_form == (4 if name in _ST_STACKS else 3)
    pool = ax.Pool(S, 256)
    pool.set_model(m)
    assert pool.kernel_name == ("k_conv_st" if name in _ST_STACKS else "k_conv_ms")
    pool.set_controls(cg)
    got = np.empty_like(x)
    pos = 0
    for n in _MS_SIZES:
        got[:, pos:pos + n] = pool.process(np.ascontiguousarray(x[:, pos:pos + n]))
        pos += n
    pool.close()
    assert np.isfinite(got).all()
    errlog.bound(np.abs(got - want).max() / scale, 3e-6, "gpu_parity:conv_stacks_default")


@pytest.mark.parametrize("name,l0,rest", _MS_STACKS, ids=[s[0] for s in _MS_STACKS])
def test_conv_stacks_on_the_split_kernel_corners(name, l0, rest, tmp_path, monkeypatch):
    """k_conv_ms at the corners of what it admits — two to four taps (one or two bf16 k-steps, the first half empty for odd counts), histories
    up to and beyond the 128 frames its plane holds (fragments straight from the history in HBM, lanes of one fragment from different
    sources), dilations that are no multiples of sixteen, every activation — against the oracle and against k_conv_mfma (fp32 MFMAs) on ragged
    blocks (a layer's history is a ring over time: a short block on a deep layer writes its own frames and nothing else); 0- and 1-frame blocks; the
    split-launch form too; and, for the stacks with a compiled k_conv_st geometry, the streaming form against the layer-major one bit for bit."""
    path, spec = _ms_stack_model(name, l0, rest, tmp_path)
    S = 6
    sizes = _MS_SIZES
    x = modelgen.signal(S, sum(sizes), seed=41)
    cg, co = _ctl_pair(pregain_db=1.0, treble_boost_db=2.0)
    want = O.run_streams(spec, co, x, 256)
    scale = max(1.0, float(np.abs(want).max()))
    outs = {}
    # (the stacks k_conv_st serves: their blocks of 64 / 128 / 256 frames run there — tile-major, the same bits — unless AIDAX_CONV_ST=0)
    streamed = name in _ST_STACKS
    for env, kname in (({}, "k_conv_ms"), ({"AIDAX_CONV_FUSED": "0"}, "k_chain+k_conv_ms"), ({"AIDAX_CONV_MS": "0"}, "k_conv_mfma"), ({"AIDAX_CONV_ST": "0"}, "k_conv_ms/all")):
        for k_ in ("AIDAX_CONV_FUSED", "AIDAX_CONV_MS", "AIDAX_CONV_ST"):
            monkeypatch.delenv(k_, raising=False)
        for k_, v in env.items():
            monkeypatch.setenv(k_, v)
        pool = ax.Pool(S, 256)
        pool.set_model(ax.Model(path))
        assert pool.kernel_name == ("k_conv_st" if streamed and kname == "k_conv_ms" else kname.split("/")[0]), (name, pool.kernel_name)
        pool.set_controls(cg)
        got = np.empty_like(x)
        pos = 0
        for n in sizes:
            got[:, pos:pos + n] = pool.process(np.ascontiguousarray(x[:, pos:pos + n]))
            pos += n
        pool.close()
        assert np.isfinite(got).all()
        errlog.bound(np.abs(got - want).max() / scale, 3e-6, "gpu_parity:conv_ms_corners")
        outs[kname] = got
    assert np.array_equal(outs["k_conv_ms"], outs["k_chain+k_conv_ms"])      # one launch or three: the same bits
    assert np.array_equal(outs["k_conv_ms"], outs["k_conv_ms/all"])          # full blocks as a stream of tiles or layer by layer: the same bits
    errlog.bound(np.abs(outs["k_conv_ms"] - outs["k_conv_mfma"]).max() / scale, 2e-6, "gpu_parity:conv_ms_vs_mfma")


_LONG_PERIODS = {"odd dilations": 20574, "history = the plane's": 8064, "four taps, 64 apart": 4032}
_RING_RUNS = {}


def _ring_period_case(name, tmp_path):
    """One of the stacks whose ring period is long, on ragged blocks until the stream's time (kept modulo the least common multiple of the
    layers' history lengths: conv_ms_period, ConvDesc::ms_pos_mod) has wrapped twice, both times INSIDE a block: (path, spec, sizes, x,
    controls, the oracle's run)."""
    from math import gcd
    _, l0, rest = next(s for s in _MS_STACKS if s[0] == name)
    period = 1
    for k, dil, _ in rest:
        h = (k - 1) * dil
        period = period // gcd(period, h) * h
    assert period == _LONG_PERIODS[name] and period < (1 << 24)
    sizes = []
    while sum(sizes) <= 2 * period + 300:
        sizes += _MS_SIZES
    starts = set(np.cumsum([0] + sizes).tolist())
    assert sum(sizes) > 2 * period and period not in starts and 2 * period not in starts
    cg, co = _ctl_pair(pregain_db=1.0, treble_boost_db=2.0)
    if name not in _RING_RUNS:                                  # (the input and the oracle's run: computed once, shared by the two tests, read-only)
        path, spec = _ms_stack_model(name, l0, rest, tmp_path)
        x = modelgen.signal(6, sum(sizes), seed=43)
        want = O.run_streams(spec, co, x, 256)
        for a in (x, want):
            a.setflags(write=False)
        _RING_RUNS[name] = dict(json=open(path).read(), x=x, want=want)
    return _RING_RUNS[name], sizes, cg


def _ring_period_run(r, sizes, cg, kname):
    pool = ax.Pool(6, 256)
    pool.set_model(ax.Model(text=r["json"]))
    assert pool.kernel_name == kname, (pool.kernel_name, kname)
    pool.set_controls(cg)
    got = np.empty_like(r["x"])
    pos = 0
    for n in sizes:
        got[:, pos:pos + n] = pool.process(np.ascontiguousarray(r["x"][:, pos:pos + n]))
        pos += n
    pool.close()
    assert np.isfinite(got).all()
    return got


@pytest.mark.parametrize("name", sorted(_LONG_PERIODS))
def test_conv_stacks_run_past_their_ring_period(name, tmp_path):
    """The runs above are 2241 frames long and the time word of these three stacks wraps after 20574, 8064 and 4032: here it wraps twice, in
    the middle of a block, with every ring at whatever phase the ragged blocks left it — as the pool runs them (no switch: the ship leg too)."""
    r, sizes, cg = _ring_period_case(name, tmp_path)
    got = _ring_period_run(r, sizes, cg, "k_conv_ms")
    scale = max(1.0, float(np.abs(r["want"]).max()))
    errlog.bound(np.abs(got - r["want"]).max() / scale, 3e-6, "gpu_parity:conv_ring_period")
    # ... and no worse behind the second wrap than before the first
    period = _LONG_PERIODS[name]
    errlog.bound(np.abs(got - r["want"])[:, 2 * period:].max() / scale, 3e-6, "gpu_parity:conv_ring_period_after_two_wraps")


@pytest.mark.parametrize("name", sorted(_LONG_PERIODS))
def test_conv_stacks_past_their_ring_period_on_the_other_forms(name, tmp_path, monkeypatch):
    """... bit for bit the split-launch form's run (the same rings, the same time word), and within the layouts' usual distance of
    k_conv_mfma, whose histories have no period."""
    r, sizes, cg = _ring_period_case(name, tmp_path)
    base = _ring_period_run(r, sizes, cg, "k_conv_ms")
    scale = max(1.0, float(np.abs(r["want"]).max()))
    monkeypatch.setenv("AIDAX_CONV_FUSED", "0")
    split = _ring_period_run(r, sizes, cg, "k_chain+k_conv_ms")
    monkeypatch.delenv("AIDAX_CONV_FUSED")
    monkeypatch.setenv("AIDAX_CONV_MS", "0")
    mfma = _ring_period_run(r, sizes, cg, "k_conv_mfma")
    assert np.array_equal(base, split), np.argwhere(base != split)[0]
    errlog.bound(np.abs(mfma - r["want"]).max() / scale, 3e-6, "gpu_parity:conv_ring_period")
    errlog.bound(np.abs(base - mfma).max() / scale, 2e-6, "gpu_parity:conv_ring_period_vs_mfma")


@pytest.mark.parametrize("seed", range(8))
def test_random_recurrent_stacks(seed, tmp_path, monkeypatch):
    """Stacked / wide recurrent models drawn at random — LSTM or GRU, 2..4 layers or one layer wider than the table,
    widths that are multiples of four but not of sixteen too (they run zero-padded on the matrix cores), 1..3 inputs,
    skip and gains — on the matrix-core kernel the pool picks and on the VALU kernel against the oracle, with PARAM
    moves and ragged blocks."""
    rs = np.random.RandomState(700 + seed)
    kind = str(rs.choice(["lstm", "gru"]))
    n_rnn = int(rs.choice([1, 2, 2, 3, 4]))
    hidden = int(rs.choice([84, 96, 100, 112, 128])) if n_rnn == 1 else int(rs.choice([8, 12, 20, 24, 36, 44, 48, 64, 72, 96]))
    I = int(rs.randint(1, 4))
    j = modelgen.make_model(kind, hidden, I, seed=70 + seed, n_rnn=n_rnn, in_skip=int(rs.randint(2)),
                            in_gain=float(rs.uniform(-2, 2)), out_gain=float(rs.uniform(-2, 2)))
    path = modelgen.write_model(j, str(tmp_path / f"rs{seed}.json"))
    spec = O.parse_model(j)
    S = int(rs.choice([3, 17, 40]))
    sizes = [256, 37, 0, 1, 200, 256]
    x = modelgen.signal(S, sum(sizes), seed=500 + seed)
    names = []
    for env in ({}, {"AIDAX_KERNEL": "valu"}):
        monkeypatch.delenv("AIDAX_KERNEL", raising=False)
        for k_, v in env.items():
            monkeypatch.setenv(k_, v)
        pool = ax.Pool(S, 256)
        pool.set_model(ax.Model(path))
        names.append(pool.kernel_name)
        plugs = [O.OraclePlugin() for _ in range(S)]
        for p_ in plugs:
            p_.set_model(O.OracleModel(spec))
        worst, pos = 0.0, 0
        for bi, n in enumerate(sizes):
            kw = dict(param1=0.2 + 0.1 * bi, param2=0.9 - 0.15 * bi, pregain_db=1.0)
            pool.set_controls(ax.default_controls(**kw))
            got = pool.process(np.ascontiguousarray(x[:, pos:pos + n]))
            for s_ in range(S):
                want = plugs[s_].run(O.default_controls(**kw), x[s_, pos:pos + n])
                if n:
                    worst = max(worst, float(np.abs(got[s_] - want).max()) / max(1.0, float(np.abs(want).max())))
            pos += n
        errlog.bound(worst, 3e-6, "gpu_parity:random_stack")
        pool.close()
    assert names[0] != names[1], names


def test_conv_stack_on_a_pool_with_long_blocks(tmp_path):
    """The matrix-core conv kernel carries 256 frames per launch; a pool created for longer host blocks sends a block
    through in time slices, each the whole run() of its slice (rows keep the block's pitch). Ragged long blocks against
    the oracle, and bit-identical to a pool that is handed the same audio in 256-frame blocks."""
    path, spec = _model_file(tmp_path, "c16long", kind="conv", hidden=16, input_size=1, seed=79, in_skip=1, out_gain=1.5)
    S = 5
    sizes = [2048, 1000, 513, 256, 300, 1, 0, 257]
    x = modelgen.signal(S, sum(sizes), seed=23)
    cg, co = _ctl_pair(bass_boost_db=3.0, pregain_db=2.0, eq_position=1.0)
    big = ax.Pool(S, 2048)
    big.set_model(ax.Model(path))
    assert big.kernel_name == "k_conv_st"              # (full slices as a stream of tiles, ragged ones through k_conv_ms: one state)
    big.set_controls(cg)
    got = np.empty_like(x)
    pos = 0
    for n in sizes:
        got[:, pos:pos + n] = big.process(np.ascontiguousarray(x[:, pos:pos + n]))
        pos += n
    want = O.run_streams(spec, co, x, 256)
    errlog.bound(np.abs(got - want).max(), 1.5e-6, "gpu_parity:conv_long_blocks")
    small = ax.Pool(S, 256)
    small.set_model(ax.Model(path))
    small.set_controls(cg)
    # the same slices: block boundaries of the long pool's launches (every `sizes` entry cut at multiples of 256)
    ref = np.empty_like(x)
    pos = 0
    for n in sizes:
        for d in range(0, max(n, 1), 256):
            c = min(256, n - d)
            ref[:, pos + d:pos + d + c] = small.process(np.ascontiguousarray(x[:, pos + d:pos + d + c]))
        pos += n
    assert np.array_equal(got, ref)


@pytest.mark.parametrize("ms", ["1", "0"])
def test_conv_fused_launch_is_bit_identical_to_split_launches(ms, tmp_path, monkeypatch):
    """The conv stack's one-launch form (chain passes inside k_conv_mfma) against packed k_chain launches around the
    same kernel: same operations per sample in the same order, so every output sample and the carried state agree
    to the bit — ragged blocks incl. 0 and 1 frames, per-stream disable / model bypass / EQ position / bandpass."""
    path, _ = _model_file(tmp_path, "c16x8f", kind="conv", hidden=16, input_size=1, seed=78, in_skip=1, in_gain=-1.5, out_gain=2.0)
    S = 37
    sizes = [256, 1, 0, 37, 200, 16, 255, 64, 129, 3, 128, 256]
    x = modelgen.signal(S, sum(sizes), seed=22)
    kws = [dict(), dict(enabled=0.0), dict(net_bypass=1.0), dict(eq_position=1.0, bass_boost_db=5.0, mid_type=1.0),
           dict(dc_blocker=0.0, in_lpf_pc=0.0, eq_bypass=1.0), dict(pregain_db=6.0, master_db=-6.0, treble_boost_db=4.0)]
    outs = []
    # (third run: the fused form without its issue priority by progress — AIDAX_TUNE bit 2048 — a scheduling hint, same bits)
    # (fourth run: full blocks through k_conv_ms too — AIDAX_CONV_ST=0 — instead of the streaming form k_conv_st: the same bits, the same state)
    for fused, tune, st in (("1", "0", "1"), ("0", "0", "1"), ("1", "2048", "1"), ("1", "0", "0")):
        monkeypatch.setenv("AIDAX_CONV_FUSED", fused)
        monkeypatch.setenv("AIDAX_TUNE", tune)
        monkeypatch.setenv("AIDAX_CONV_MS", ms)
        monkeypatch.setenv("AIDAX_CONV_ST", st)
        pool = ax.Pool(S, 256)
        pool.set_model(ax.Model(path))
        base = "k_conv_ms" if ms == "1" else "k_conv_mfma"
        assert pool.kernel_name == (("k_conv_st" if ms == "1" and st == "1" else base) if fused == "1" else "k_chain+" + base)
        got = np.empty_like(x)
        pos = 0
        for bi, n in enumerate(sizes):
            for s in range(S):
                c = dict(kws[s % len(kws)])
                if bi >= 4:
                    c.update(master_db=-3.0, pregain_db=1.0)
                pool.set_controls(ax.default_controls(**c), stream=s)
            got[:, pos:pos + n] = pool.process(np.ascontiguousarray(x[:, pos:pos + n]))
            pos += n
        outs.append(got)
        pool.close()
    assert np.array_equal(outs[0], outs[1])
    assert np.array_equal(outs[0], outs[2])
    assert np.array_equal(outs[0], outs[3])


@pytest.mark.parametrize("name,kw", [
    ("g128", dict(kind="gru", hidden=128, input_size=3, seed=128)),                      # one wide layer, both params
    ("l64x2", dict(kind="lstm", hidden=64, input_size=2, seed=642, n_rnn=2, in_skip=1, in_gain=-2.0, out_gain=3.0)),
    ("l16x4", dict(kind="lstm", hidden=16, input_size=1, seed=164, n_rnn=4)),             # one tile per wave, deepest skew
    ("c16x8", dict(kind="conv", hidden=16, input_size=1, seed=77, in_skip=1, out_gain=2.0)),   # receptive field 511 frames
    ("c8x4k5", dict(kind="conv", hidden=8, input_size=1, seed=85, conv_layers=4, conv_k=5)),    # 40 k rows: padded k-steps, 8 of 16 columns
])
def test_matrix_core_form_ragged_blocks_and_per_stream_controls(name, kw, tmp_path):
    """k_mfma with 37 streams (three 16-stream workgroups, the last one ragged), block sizes around the
    kernel's 256-frame staging chunk incl. 0 and 1, per-stream disable / bypass / EQ position, PARAM
    ramps that change between blocks - every fifth stream against the plugin mirror of the oracle."""
    path, spec = _model_file(tmp_path, name, **kw)
    S = 37
    conv = kw["kind"] == "conv"
    sizes = [256, 1, 0, 37, 200, 16, 255, 129, 3] if conv else [256, 1, 0, 37, 700, 16, 255, 513, 3]
    x = modelgen.signal(S, sum(sizes), seed=21)
    pool = ax.Pool(S, 256 if conv else 1024)
    pool.set_model(ax.Model(path))
    assert _canon(pool.kernel_name) == ("k_conv_mfma" if conv else "k_chain+k_mfma_lp" if kw.get("n_rnn", 1) > 1 else "k_chain+k_mfma")
    kws = [dict(param1=0.3, param2=0.8), dict(enabled=0.0), dict(net_bypass=1.0), dict(eq_position=1.0, bass_boost_db=5.0, mid_type=1.0),
           dict(dc_blocker=0.0, in_lpf_pc=0.0, eq_bypass=1.0, param1=1.0), dict(pregain_db=6.0, master_db=-6.0, treble_boost_db=4.0, param2=0.1)]
    flip = dict(param1=0.9, param2=0.2, master_db=-3.0)                     # applied to every stream from the 5th block on
    got = np.empty_like(x)
    pos = 0
    for bi, n in enumerate(sizes):
        for s in range(S):
            c = dict(kws[s % len(kws)])
            if bi >= 4:
                c.update(flip)
            pool.set_controls(ax.default_controls(**c), stream=s)
        got[:, pos:pos + n] = pool.process(np.ascontiguousarray(x[:, pos:pos + n]))
        pos += n
    for s in list(range(0, S, 5)) + [S - 1]:
        plug = O.OraclePlugin()
        plug.set_model(O.OracleModel(spec))
        want = np.empty(x.shape[1], np.float32)
        pos = 0
        for bi, n in enumerate(sizes):
            c = dict(kws[s % len(kws)])
            if bi >= 4:
                c.update(flip)
            want[pos:pos + n] = plug.run(O.default_controls(**c), x[s, pos:pos + n])
            pos += n
        c0 = kws[s % len(kws)]
        if c0.get("enabled", 1.0) == 0.0:
            assert np.array_equal(got[s], x[s])                              # hard bypass copies the input (:612-619)
        elif c0.get("net_bypass", 0.0) == 1.0:
            assert np.array_equal(got[s], want), s                           # no NN in circuit: bit-exact
        else:
            errlog.bound(np.abs(got[s] - want).max(), 2e-6, "gpu_parity:458")


def test_matrix_core_form_model_swap_and_activate(tmp_path, bundled_models):
    """A pool that moves between a register-resident model, a k_mfma model and no model keeps the
    reference's swap semantics (fresh state + warm-up, PARAM smoothers re-armed by activate)."""
    path_w, spec_w = _model_file(tmp_path, "w", kind="lstm", hidden=96, input_size=2, seed=7, n_rnn=2)
    path_t, spec_t = _model_file(tmp_path, "t", kind="gru", hidden=16, input_size=2, seed=9)
    S, n = 20, 192
    x = modelgen.signal(S, 4 * n, seed=5)
    cg, co = _ctl_pair(param1=0.6)
    pool = ax.Pool(S, 256)
    pool.set_controls(cg)
    plug = [O.OraclePlugin() for _ in range(2)]
    got, want = [], [[], []]
    seq = [(path_t, spec_t), (path_w, spec_w), (path_w, spec_w), (path_t, spec_t)]
    for bi, (pth, spec) in enumerate(seq):
        if bi != 2:
            pool.set_model(ax.Model(pth))
            for p in plug:                                                   # a swap inherits the param targets (:822-825)
                old = (p.model.ptr.contents.param1Coeff.target, p.model.ptr.contents.param2Coeff.target) if p.model else (0.0, 0.0)
                p.set_model(O.OracleModel(spec, old[0], old[1]))
        else:
            pool.activate()
            for p in plug:
                p.activate()
        got.append(pool.process(np.ascontiguousarray(x[:, bi * n:(bi + 1) * n])))
        for i, s in enumerate((0, S - 1)):
            want[i].append(plug[i].run(co, x[s, bi * n:(bi + 1) * n]))
    got = np.concatenate(got, axis=1)
    for i, s in enumerate((0, S - 1)):
        errlog.bound(np.abs(got[s] - np.concatenate(want[i])).max(), 1e-6, "gpu_parity:489")


def test_stacked_model_state_readback(tmp_path):
    path, spec = _model_file(tmp_path, "l96", kind="lstm", hidden=96, input_size=1, seed=96, n_rnn=2)
    pool = ax.Pool(3, 128)
    pool.set_model(ax.Model(path), ax.START_WARMUP)
    om = O.OracleModel(spec, warmup=True)
    for layer in (0, 1):
        h, c = pool.read_state(2, layer)
        oh, oc = om.state(layer)
        assert h.size == 96 and np.abs(h - oh).max() < 4e-6 and np.abs(c - oc).max() < 4e-6


# ------------------------------------------------------------ the launch forms of the chain

@pytest.mark.parametrize("form", ["wave", "pipe", "split", "mfma", "mfma_split", "quad", "q4"])
def test_every_kernel_form_passes_the_same_chain_cases(form, tmp_path, monkeypatch, bundled_models):
    """AIDAX_KERNEL pins one form: one wave per stream, the 3-wave pipeline, the split launches (packed
    chain kernels around the lean recurrent kernel), the matrix-core kernel (16 streams per workgroup) with
    the DSP chain on its helper waves (one launch) or between the packed chain launches. Same inputs, same oracle,
    same bars: ragged block sizes incl. the pre-run, per-stream controls with bypass/disable, conditioned GRU
    with ramping params, model swap and activate."""
    monkeypatch.setenv("AIDAX_KERNEL", form.split("_")[0])
    if form == "mfma_split":
        monkeypatch.setenv("AIDAX_LP_FUSED", "0")
    # (1) ragged blocks, 70 streams (not a multiple of the 8-stream chain waves), LSTM-32 with skip + gains
    path, spec = _model_file(tmp_path, "f1", kind="lstm", hidden=32, input_size=1, seed=5, in_skip=1, in_gain=-2.0, out_gain=3.0)
    S = 70
    sizes = [256, 1, 0, 37, 16, 255, 64, 3]
    x = modelgen.signal(S, sum(sizes), seed=8)
    pool = ax.Pool(S, 256)
    pool.set_model(ax.Model(path))
    kws = [dict(), dict(enabled=0.0), dict(net_bypass=1.0), dict(eq_position=1.0, bass_boost_db=5.0, mid_type=1.0),
           dict(dc_blocker=0.0, in_lpf_pc=0.0, eq_bypass=1.0), dict(pregain_db=6.0, master_db=-6.0, treble_boost_db=4.0)]
    for s in range(S):
        pool.set_controls(ax.default_controls(**kws[s % len(kws)]), stream=s)
    assert _canon(pool.kernel_name).startswith({"wave": "k_lstm<", "pipe": "k_lstm_pipe<", "split": "k_chain+k_nn<", "mfma": "k_mfma_lp", "mfma_split": "k_chain+k_mfma", "quad": "k_chain+k_quad", "q4": "k_lstm_q4<"}[form])
    got = np.empty_like(x)
    pos = 0
    for n in sizes:
        got[:, pos:pos + n] = pool.process(np.ascontiguousarray(x[:, pos:pos + n]))
        pos += n
    for s in range(0, S, 5):
        plug = O.OraclePlugin()
        plug.set_model(O.OracleModel(spec))
        want = np.empty(x.shape[1], np.float32)
        pos = 0
        for n in sizes:
            want[pos:pos + n] = plug.run(O.default_controls(**kws[s % len(kws)]), x[s, pos:pos + n])
            pos += n
        kw = kws[s % len(kws)]
        if kw.get("enabled") == 0.0 or kw.get("net_bypass") == 1.0:
            assert np.array_equal(got[s], want), (form, s)
        else:
            errlog.bound(np.abs(got[s] - want).max(), 1e-6, "gpu_parity:542")
    # (2) conditioned GRU, params ramping block by block, activate in the middle, then a model swap
    pa, spec_a = _model_file(tmp_path, "f2", kind="gru", hidden=24, input_size=3, seed=11)
    pb, spec_b = _model_file(tmp_path, "f3", kind="lstm", hidden=12, input_size=2, seed=12)
    S2 = 9
    x2 = modelgen.signal(S2, 1280, seed=13)
    pool = ax.Pool(S2, 128)
    pool.set_model(ax.Model(pa))
    plugs = [O.OraclePlugin() for _ in range(S2)]
    for p in plugs:
        p.set_model(O.OracleModel(spec_a))
    for bi, b in enumerate(range(0, 1280, 128)):
        kw = dict(param1=bi / 9.0, param2=1.0 - 0.07 * bi, mid_boost_db=3.0)
        if bi == 4:
            pool.activate()
            for p in plugs:
                p.activate()
        if bi == 6:
            pool.set_model(ax.Model(pb))
            for p in plugs:
                old = p.model.ptr.contents
                p.set_model(O.OracleModel(spec_b, old.param1Coeff.target, old.param2Coeff.target))
        pool.set_controls(ax.default_controls(**kw))
        g = pool.process(np.ascontiguousarray(x2[:, b:b + 128]))
        for s in range(S2):
            w = plugs[s].run(O.default_controls(**kw), x2[s, b:b + 128])
            errlog.bound(np.abs(g[s] - w).max(), 1e-6, "gpu_parity:568")
    # (3) no model at all (chain only, loading cleared): bit-exact in every form
    x3 = modelgen.signal(66, 300, seed=3)
    pool = ax.Pool(66, 300)
    pool.set_loading(False)
    cg, co = _ctl_pair(bass_boost_db=4.0, presence_boost_db=-3.0, pregain_db=1.5)
    pool.set_controls(cg)
    g3 = pool.process(x3)
    for s in (0, 7, 65):
        p = O.OraclePlugin()
        p.set_loading(False)
        assert np.array_equal(g3[s], p.run(co, x3[s])), (form, s)


@pytest.mark.parametrize("name,kw", [
    ("l32x2skip", dict(kind="lstm", hidden=32, input_size=1, seed=3220, n_rnn=2, in_skip=1, in_gain=-2.0, out_gain=3.0)),
    ("g48x3", dict(kind="gru", hidden=48, input_size=3, seed=4830, n_rnn=3)),
    ("l96x2", dict(kind="lstm", hidden=96, input_size=2, seed=9620, n_rnn=2)),
    ("g80", dict(kind="gru", hidden=80, input_size=3, seed=8030)),                        # one layer, no room for helper waves: the same form
])
@pytest.mark.parametrize("late", [False, True])
@pytest.mark.parametrize("arith", ["bf16x3", "fp32"])
def test_stacked_one_launch_form_is_bit_identical_to_the_three_launch_form(name, kw, late, arith, tmp_path, monkeypatch):
    """Stacked models on pools whose blocks fit one staging chunk run their whole run() in the k_mfma_lp launch: the packed
    pre pass on two waves of the first layer's workgroup (and, uncommitted, of the last layer's, which needs the model input
    for in_skip and for net-off streams), the post pass behind the last layer's last tick. Same chain code, same kernel body
    as between two k_chain launches (AIDAX_LP_FUSED=0): every output sample and every state word bit for bit, over ragged
    blocks incl. 0 and 1, 40 streams (the last group ragged), per-stream disable / bypass / EQ position / moving ramps,
    activate() in the middle — and against the oracle. `late`: with the last layer's workgroup held back by 100 us at its
    start (AIDAX_TUNE 8192) — the layers' workgroups share stream state, and the first version of this form was right only
    while they started together."""
    path, spec = _model_file(tmp_path, name, **kw)
    if late:
        monkeypatch.setenv("AIDAX_TUNE", "8192")
    if arith == "fp32":
        monkeypatch.setenv("AIDAX_LP_SPLIT", "0")             # k_mfma_lp (fp32 MFMAs) instead of k_mfma_ls
    if kw.get("n_rnn", 1) == 1:
        monkeypatch.setenv("AIDAX_KERNEL", "mfma")            # (40 streams of a table model would take k_quad)
        monkeypatch.setenv("AIDAX_GRU_GM", "0")               # (... and GRU-80 on the matrix cores k_gru_gs: this is about k_mfma_lp's chain form)
    S = 40
    sizes = [256, 1, 0, 37, 16, 255, 64, 3, 256]
    x = modelgen.signal(S, sum(sizes), seed=41)
    kws = [dict(param1=0.3, param2=0.8), dict(enabled=0.0), dict(net_bypass=1.0), dict(eq_position=1.0, bass_boost_db=5.0, mid_type=1.0),
           dict(dc_blocker=0.0, in_lpf_pc=0.0, eq_bypass=1.0, param1=1.0), dict(pregain_db=6.0, master_db=-6.0, treble_boost_db=4.0, param2=0.1)]
    outs, states, dsp = {}, {}, {}
    for form in ("one", "three"):
        monkeypatch.delenv("AIDAX_LP_FUSED", raising=False)
        if form == "three":
            monkeypatch.setenv("AIDAX_LP_FUSED", "0")
        pool = ax.Pool(S, 256)
        pool.set_model(ax.Model(path))
        lp = "k_mfma_lp" if arith == "fp32" or kw.get("n_rnn", 1) == 1 else "k_mfma_ls"
        assert pool.kernel_name == (lp if form == "one" else "k_chain+" + lp)
        for s_ in range(S):
            pool.set_controls(ax.default_controls(**kws[s_ % len(kws)]), stream=s_)
        got, pos = np.empty_like(x), 0
        for bi, n in enumerate(sizes):
            if bi == 5:
                pool.activate()
            got[:, pos:pos + n] = pool.process(np.ascontiguousarray(x[:, pos:pos + n]))
            pos += n
        outs[form] = got
        states[form] = [pool.read_state(stream=s_, layer=kw.get("n_rnn", 1) - 1, hidden=128) for s_ in (0, 3, S - 1)]
        dsp[form] = [pool.export_stream_dsp(s_) for s_ in (0, 3, 5, S - 1)]
        pool.close()
    assert np.array_equal(outs["one"], outs["three"])
    for (h1, c1), (h3, c3) in zip(states["one"], states["three"]):
        assert np.array_equal(h1, h3) and np.array_equal(c1, c3)
    for a_, b_ in zip(dsp["one"], dsp["three"]):
        assert bytes(a_) == bytes(b_)
    for s_ in range(0, S, 5):
        plug = O.OraclePlugin()
        plug.set_model(O.OracleModel(spec))
        want, pos = np.empty(x.shape[1], np.float32), 0
        for bi, n in enumerate(sizes):
            if bi == 5:
                plug.activate()
            want[pos:pos + n] = plug.run(O.default_controls(**kws[s_ % len(kws)]), x[s_, pos:pos + n])
            pos += n
        kw_ = kws[s_ % len(kws)]
        if kw_.get("enabled") == 0.0 or kw_.get("net_bypass") == 1.0:
            assert np.array_equal(outs["one"][s_], want), s_
        else:
            errlog.bound(np.abs(outs["one"][s_] - want).max(), 2e-6, "gpu_parity:lp_one_launch")


@pytest.mark.parametrize("kind,hidden,isz", [("lstm", 64, 2), ("lstm", 32, 1), ("gru", 16, 3), ("lstm", 12, 2)])
def test_one_layer_one_launch_form_is_bit_identical_to_the_three_launch_form(kind, hidden, isz, tmp_path, monkeypatch):
    """k_mfma_lp with its four helper waves (pre pass ahead of the frame loop, model inputs, the Dense's tail, post pass
    behind the loop: one launch) against the same kernel between two packed k_chain launches (AIDAX_LP_FUSED=0): the
    same chain arithmetic in resumable macro-steps, the same body — every output sample and every state word bit for
    bit, over ragged blocks incl. 0, 1 and blocks of several 256-frame staging chunks, 70 streams, per-stream controls,
    activate() in the middle; and against the oracle."""
    monkeypatch.setenv("AIDAX_KERNEL", "mfma")
    path, spec = _model_file(tmp_path, f"ol{kind}{hidden}_{isz}", kind=kind, hidden=hidden, input_size=isz, seed=800 + hidden + isz, in_skip=isz == 1)
    S = 70
    sizes = [256, 1, 0, 37, 700, 16, 255, 513, 3, 1024]
    x = modelgen.signal(S, sum(sizes), seed=43)
    kws = [dict(param1=0.3, param2=0.8), dict(enabled=0.0), dict(net_bypass=1.0), dict(eq_position=1.0, bass_boost_db=5.0, mid_type=1.0),
           dict(dc_blocker=0.0, in_lpf_pc=0.0, eq_bypass=1.0, param1=1.0), dict(pregain_db=6.0, master_db=-6.0, treble_boost_db=4.0, param2=0.1)]
    outs, states, dsp = {}, {}, {}
    for form in ("one", "three"):
        monkeypatch.delenv("AIDAX_LP_FUSED", raising=False)
        if form == "three":
            monkeypatch.setenv("AIDAX_LP_FUSED", "0")
        pool = ax.Pool(S, 1024)
        pool.set_model(ax.Model(path))
        assert pool.kernel_name == ("k_mfma_lp" if form == "one" else "k_chain+k_mfma_lp")
        for s_ in range(S):
            pool.set_controls(ax.default_controls(**kws[s_ % len(kws)]), stream=s_)
        got, pos = np.empty_like(x), 0
        for bi, n in enumerate(sizes):
            if bi == 5:
                pool.activate()
            got[:, pos:pos + n] = pool.process(np.ascontiguousarray(x[:, pos:pos + n]))
            pos += n
        outs[form] = got
        states[form] = [pool.read_state(stream=s_, layer=0, hidden=128) for s_ in (0, 3, S - 1)]
        dsp[form] = [pool.export_stream_dsp(s_) for s_ in (0, 3, 5, S - 1)]
        pool.close()
    assert np.array_equal(outs["one"], outs["three"])
    for (h1, c1), (h3, c3) in zip(states["one"], states["three"]):
        assert np.array_equal(h1, h3) and np.array_equal(c1, c3)
    for a_, b_ in zip(dsp["one"], dsp["three"]):
        assert bytes(a_) == bytes(b_)
    for s_ in range(0, S, 5):
        plug = O.OraclePlugin()
        plug.set_model(O.OracleModel(spec))
        want, pos = np.empty(x.shape[1], np.float32), 0
        for bi, n in enumerate(sizes):
            if bi == 5:
                plug.activate()
            want[pos:pos + n] = plug.run(O.default_controls(**kws[s_ % len(kws)]), x[s_, pos:pos + n])
            pos += n
        kw_ = kws[s_ % len(kws)]
        if kw_.get("enabled") == 0.0 or kw_.get("net_bypass") == 1.0:
            assert np.array_equal(outs["one"][s_], want), s_
        else:
            errlog.bound(np.abs(outs["one"][s_] - want).max(), 2e-6, "gpu_parity:lp1_one_launch")


@pytest.mark.parametrize("hidden,isz", [(64, 3), (64, 1), (40, 2)])
def test_gate_major_gru_kernel_ragged_blocks_controls_and_state_bits(hidden, isz, tmp_path, monkeypatch):
    """k_gru_gm (one-layer GRU, three recurrent tiles + an input-only accumulator per 16 units, the DSP chain on its
    helper waves: one launch per block) against the per-stream oracle plugins over ragged block sizes incl. 0 and 1 and
    blocks longer than the 256-frame staging chunk, 70 streams (the last group ragged), per-stream bypass / disable / EQ
    position / ramping params — and against the four-rows-per-unit kernels (k_mfma_lp's one-launch form, k_mfma behind
    packed chain launches) on the same weights: bit-identical recurrent state."""
    monkeypatch.setenv("AIDAX_KERNEL", "mfma")
    path, spec = _model_file(tmp_path, f"gm{hidden}_{isz}", kind="gru", hidden=hidden, input_size=isz, seed=700 + hidden + isz, in_skip=isz == 1)
    S = 70
    sizes = [256, 1, 0, 37, 700, 16, 255, 513, 3]
    x = modelgen.signal(S, sum(sizes), seed=31)
    kws = [dict(param1=0.3, param2=0.8), dict(enabled=0.0), dict(net_bypass=1.0), dict(eq_position=1.0, bass_boost_db=5.0, mid_type=1.0),
           dict(dc_blocker=0.0, in_lpf_pc=0.0, eq_bypass=1.0, param1=1.0), dict(pregain_db=6.0, master_db=-6.0, treble_boost_db=4.0, param2=0.1)]
    flip = dict(param1=0.9, param2=0.2, master_db=-3.0)                     # applied to every stream from the 5th block on
    outs, states = {}, {}
    forms = (("gs", {}), ("gs9", {"AIDAX_GS_PRODUCTS": "9"}), ("gm", {"AIDAX_GRU_GM": "f32"}), ("lp", {"AIDAX_GRU_GM": "0"}),
             ("mfma", {"AIDAX_GRU_GM": "0", "AIDAX_MFMA_LP": "0"}))
    for form, env in forms:
        for k in ("AIDAX_GRU_GM", "AIDAX_MFMA_LP", "AIDAX_GS_PRODUCTS"):
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        pool = ax.Pool(S, 1024)
        pool.set_model(ax.Model(path))
        assert pool.kernel_name == {"gs": "k_gru_gs", "gs9": "k_gru_gs", "gm": "k_gru_gm", "lp": "k_mfma_lp", "mfma": "k_chain+k_mfma"}[form]
        for s_ in range(S):
            pool.set_controls(ax.default_controls(**kws[s_ % len(kws)]), stream=s_)
        got, pos = np.empty_like(x), 0
        for bi, n in enumerate(sizes):
            if bi == 4:
                for s_ in range(S):
                    pool.set_controls(ax.default_controls(**dict(kws[s_ % len(kws)], **flip)), stream=s_)
            got[:, pos:pos + n] = pool.process(np.ascontiguousarray(x[:, pos:pos + n]))
            pos += n
        outs[form] = got
        states[form] = [pool.read_state(stream=s_, layer=0, hidden=128)[0].copy() for s_ in (0, 5, S - 1)]
        pool.close()
    for s_ in range(0, S, 5):
        plug = O.OraclePlugin()
        plug.set_model(O.OracleModel(spec))
        want, pos = np.empty(x.shape[1], np.float32), 0
        for bi, n in enumerate(sizes):
            kw = dict(kws[s_ % len(kws)], **(flip if bi >= 4 else {}))
            want[pos:pos + n] = plug.run(O.default_controls(**kw), x[s_, pos:pos + n])
            pos += n
        kw = kws[s_ % len(kws)]
        if kw.get("enabled") == 0.0 or kw.get("net_bypass") == 1.0:
            for f in ("gs", "gs9", "gm"):
                assert np.array_equal(outs[f][s_], want), (f, s_)
        else:
            errlog.bound(np.abs(outs["gm"][s_] - want).max(), 2e-6, "gpu_parity:gru_gm")
            # the bf16 x 3 kernel: the same bar — six term products are the fp32 product to rounding, nine to the last bit
            errlog.bound(np.abs(outs["gs"][s_] - want).max(), 2e-6, "gpu_parity:gru_gs6")
            errlog.bound(np.abs(outs["gs9"][s_] - want).max(), 2e-6, "gpu_parity:gru_gs9")
    # (the split kernel sums its products in another order: its state agrees with the fp32 kernels' to rounding, not to the bit)
    for f in ("gs", "gs9"):
        for a, b in zip(states[f], states["gm"]):
            errlog.bound(np.abs(a - b).max(), 2e-6, "gpu_parity:gru_gs_state_vs_gm")
    for a, b in zip(states["gm"], states["lp"]):
        assert np.array_equal(a, b)
    for a, b in zip(states["gm"], states["mfma"]):
        assert np.array_equal(a, b)
    errlog.bound(np.abs(outs["gm"] - outs["lp"]).max(), 5e-7, "gpu_parity:gru_gm_vs_lp_outputs")



@pytest.mark.parametrize("kind,hidden,n_rnn,isz", [
    ("lstm", 80, 2, 2),      # four waves x 512 registers (fragments in AGPRs), two of five tiles per wave started below
    ("gru", 80, 2, 3),
    ("gru", 96, 2, 1),       # eight waves, cfg5's geometry with GRU cells
    ("lstm", 64, 3, 1),      # three layers: a middle workgroup both consumes and produces, no tiles started below
    ("lstm", 16, 2, 2),      # one tile per wave, one k-step half empty
    ("gru", 40, 2, 1),       # 40 units run zero-padded to 48: the second k-step's upper half stays zero
])
def test_split_stack_geometries_match_the_oracle(kind, hidden, n_rnn, isz, tmp_path):
    """k_mfma_ls in every geometry ls_geo hands out (aidax_mfmals.h): ragged blocks incl. 0 and 1, 40 streams (the last group
    ragged), PARAM moves, against per-stream oracle plugins; the one-launch form on a 256-frame pool and the three-launch form
    on a 1024-frame pool."""
    path, spec = _model_file(tmp_path, f"ls_{kind}{hidden}x{n_rnn}", kind=kind, hidden=hidden, input_size=isz, seed=900 + hidden + n_rnn, n_rnn=n_rnn,
                             in_skip=isz == 1)
    S = 40
    for max_frames, sizes, name in ((256, [256, 1, 0, 37, 255, 64], "k_mfma_ls"), (1024, [700, 16, 3, 513], "k_chain+k_mfma_ls")):
        x = modelgen.signal(S, sum(sizes), seed=33)
        pool = ax.Pool(S, max_frames)
        pool.set_model(ax.Model(path))
        assert pool.kernel_name == name, pool.kernel_name
        plugs = {}
        for s_ in (0, 7, 17, S - 1):
            p = O.OraclePlugin()
            p.set_model(O.OracleModel(spec))
            plugs[s_] = p
        pos = 0
        for bi, n in enumerate(sizes):
            kw = dict(param1=0.2 + 0.15 * bi, param2=0.9 - 0.1 * bi, pregain_db=1.0)
            pool.set_controls(ax.default_controls(**kw))
            got = pool.process(np.ascontiguousarray(x[:, pos:pos + n]))
            for s_, p in plugs.items():
                want = p.run(O.default_controls(**kw), x[s_, pos:pos + n])
                if n:
                    errlog.bound(np.abs(got[s_] - want).max(), 2e-6, "gpu_parity:ls_geometries")
            pos += n
        pool.close()

@pytest.mark.parametrize("kind,hidden,isz", [
    ("lstm", 64, 1),       # eight waves, two tiles per wave
    ("lstm", 80, 2),       # four waves x 512 registers, five tiles per wave
    ("gru", 80, 3),
    ("lstm", 40, 1),       # 40 units run zero-padded to 48: four waves, three tiles
    ("lstm", 32, 3),       # one tile per wave: no second phase for the cell update to hide in
    ("gru", 16, 2),
    ("lstm", 96, 1),       # wider than the reference's table
])
def test_lone_layer_on_the_split_kernel_matches_the_oracle(kind, hidden, isz, tmp_path, monkeypatch):
    """k_mfma_ls1 (aidax_mfmals.h): ONE layer on k_mfma_ls's body — first and last role at once, no ring. Forced (AIDAX_KERNEL=mfma,
    AIDAX_LS1=1) so that every geometry runs whatever the pool's table says: ragged blocks incl. 0 and 1, 40 streams (the last
    group ragged), PARAM moves, in_skip, against per-stream oracle plugins; the one-launch form on a 256-frame pool and the
    three-launch form on a 1024-frame pool."""
    monkeypatch.setenv("AIDAX_KERNEL", "mfma")
    monkeypatch.setenv("AIDAX_LS1", "1")
    monkeypatch.setenv("AIDAX_GRU_GM", "0")
    path, spec = _model_file(tmp_path, f"ls1_{kind}{hidden}", kind=kind, hidden=hidden, input_size=isz, seed=700 + hidden + isz, in_skip=isz == 1)
    S = 40
    for max_frames, sizes, name in ((256, [256, 1, 0, 37, 255, 64], "k_mfma_ls1"), (1024, [700, 16, 3, 513], "k_chain+k_mfma_ls1")):
        x = modelgen.signal(S, sum(sizes), seed=34)
        pool = ax.Pool(S, max_frames)
        pool.set_model(ax.Model(path))
        assert pool.kernel_name == name, pool.kernel_name
        plugs = {}
        for s_ in (0, 7, 17, S - 1):
            p = O.OraclePlugin()
            p.set_model(O.OracleModel(spec))
            plugs[s_] = p
        pos = 0
        for bi, n in enumerate(sizes):
            kw = dict(param1=0.2 + 0.15 * bi, param2=0.9 - 0.1 * bi, pregain_db=1.0)
            pool.set_controls(ax.default_controls(**kw))
            got = pool.process(np.ascontiguousarray(x[:, pos:pos + n]))
            for s_, p in plugs.items():
                want = p.run(O.default_controls(**kw), x[s_, pos:pos + n])
                if n:
                    errlog.bound(np.abs(got[s_] - want).max(), 2e-6, "gpu_parity:ls1_geometries")
            pos += n
        pool.close()


@pytest.mark.parametrize("isz,nprod", [(3, 6), (1, 9)])
def test_gru80_on_the_split_gate_major_kernel_with_two_helper_waves(isz, nprod, tmp_path, monkeypatch):
    """k_gru_gs<5, 2>: GRU-80 — five main waves (one SIMD carries two) and two helper waves with eight streams each. Forced
    (AIDAX_KERNEL=mfma): ragged blocks incl. 0 and 1 and blocks longer than a staging chunk, 70 streams, per-stream bypass /
    disable / EQ, PARAM moves, against per-stream oracle plugins; the state against k_mfma_lp's (fp32 MFMAs) to rounding."""
    monkeypatch.setenv("AIDAX_KERNEL", "mfma")
    path, spec = _model_file(tmp_path, f"gs80_{isz}", kind="gru", hidden=80, input_size=isz, seed=880 + isz, in_skip=isz == 1)
    S = 70
    sizes = [256, 1, 0, 37, 700, 16, 255, 513, 3]
    x = modelgen.signal(S, sum(sizes), seed=37)
    kws = [dict(param1=0.3, param2=0.8), dict(enabled=0.0), dict(net_bypass=1.0), dict(eq_position=1.0, bass_boost_db=5.0, mid_type=1.0),
           dict(dc_blocker=0.0, in_lpf_pc=0.0, eq_bypass=1.0, param1=1.0), dict(pregain_db=6.0, master_db=-6.0, treble_boost_db=4.0, param2=0.1)]
    outs, states = {}, {}
    for form, env in (("gs", {"AIDAX_GS_PRODUCTS": str(nprod)}), ("lp", {"AIDAX_GRU_GM": "0", "AIDAX_LS1": "0"})):
        for k in ("AIDAX_GRU_GM", "AIDAX_GS_PRODUCTS", "AIDAX_LS1"):
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        pool = ax.Pool(S, 1024)
        pool.set_model(ax.Model(path))
        assert pool.kernel_name == {"gs": "k_gru_gs", "lp": "k_chain+k_mfma_lp"}[form], pool.kernel_name
        for s_ in range(S):
            pool.set_controls(ax.default_controls(**kws[s_ % len(kws)]), stream=s_)
        got, pos = np.empty_like(x), 0
        for n in sizes:
            got[:, pos:pos + n] = pool.process(np.ascontiguousarray(x[:, pos:pos + n]))
            pos += n
        outs[form] = got
        states[form] = [pool.read_state(stream=s_, layer=0, hidden=128)[0].copy() for s_ in (0, 5, S - 1)]
        pool.close()
    for s_ in range(0, S, 5):
        plug = O.OraclePlugin()
        plug.set_model(O.OracleModel(spec))
        kw = kws[s_ % len(kws)]
        want = np.concatenate([plug.run(O.default_controls(**kw), x[s_, p0:p0 + n]) for p0, n in zip(np.cumsum([0] + sizes[:-1]), sizes)])
        if kw.get("enabled") == 0.0 or kw.get("net_bypass") == 1.0:
            assert np.array_equal(outs["gs"][s_], want), s_
        else:
            errlog.bound(np.abs(outs["gs"][s_] - want).max(), 2e-6, f"gpu_parity:gru80_gs{nprod}")
    for a, b in zip(states["gs"], states["lp"]):
        errlog.bound(np.abs(a - b).max(), 2e-6, "gpu_parity:gru80_gs_state_vs_lp")


@pytest.mark.parametrize("hidden,isz,nprod", [(64, 1, 6), (64, 3, 9), (40, 2, 6), (80, 2, 6)])
def test_one_layer_lstm_on_the_unit_major_split_kernel_matches_the_oracle(hidden, isz, nprod, tmp_path, monkeypatch):
    """k_lstm_gs (aidax_tick.hip): k_gru_gs's structure for one-layer LSTMs of 40 (run as 48) / 64 units — unit-major tiles, one
    main wave per 16 units, the DSP chain on helper waves, the whole run() in the launch. Forced (AIDAX_KERNEL=mfma, AIDAX_LSTM_GS=1):
    ragged blocks incl. 0 and 1 and blocks longer than a staging chunk, 40 streams (the last group ragged), PARAM moves, in_skip,
    EQ in circuit, against per-stream oracle plugins; copies of a stream stay bitwise identical."""
    monkeypatch.setenv("AIDAX_KERNEL", "mfma")
    monkeypatch.setenv("AIDAX_LSTM_GS", "1")
    if nprod == 9:
        monkeypatch.setenv("AIDAX_GS_PRODUCTS", "9")
    path, spec = _model_file(tmp_path, f"lgs_{hidden}", kind="lstm", hidden=hidden, input_size=isz, seed=300 + hidden + isz, in_skip=isz == 1)
    S = 40
    for max_frames, sizes in ((256, [256, 1, 0, 37, 255, 64]), (1024, [700, 16, 3, 513])):
        base = modelgen.signal(8, sum(sizes), seed=36)
        idx = (np.arange(S) * 3) % 8
        pool = ax.Pool(S, max_frames)
        pool.set_model(ax.Model(path))
        assert pool.kernel_name == "k_lstm_gs", pool.kernel_name
        plugs = []
        for _ in range(8):
            p = O.OraclePlugin()
            p.set_model(O.OracleModel(spec))
            plugs.append(p)
        pos = 0
        for bi, n in enumerate(sizes):
            kw = dict(_EQ_POST, param1=0.2 + 0.15 * bi, param2=0.9 - 0.1 * bi, pregain_db=1.0)
            pool.set_controls(ax.default_controls(**kw))
            got = pool.process(np.ascontiguousarray(base[idx, pos:pos + n]))
            for k, p in enumerate(plugs):
                want = p.run(O.default_controls(**kw), base[k, pos:pos + n])
                rows = got[idx == k]
                assert np.all(rows == rows[0])
                if n:
                    errlog.bound(np.abs(rows[0] - want).max(), 2e-6, f"gpu_parity:lstm_gs{nprod}")
            pos += n
        h, c = pool.read_state(stream=S - 1, layer=0, hidden=128)
        assert h.size == hidden and np.abs(c).max() > 1e-4
        pool.close()


@pytest.mark.parametrize("kind,hidden,n_rnn,max_frames", [("lstm", 96, 2, 256), ("gru", 48, 3, 1024)])
def test_split_stack_in_several_ranges_is_bit_identical_to_one_launch(kind, hidden, n_rnn, max_frames, tmp_path, monkeypatch):
    """A stacked pool larger than one resident grid of k_mfma_ls goes out as one launch per range of streams (aidax_pool.cpp,
    lp_round_streams). Ranges forced small here (AIDAX_LP_ROUND_GROUPS=8: 300 streams = 19 groups = ranges of 8, 8 and a ragged 3):
    outputs and state bit-identical to the one-launch pass, and within the NN bar of the oracle — one-launch form (256-frame pool)
    and three-launch form (1024-frame pool), ragged blocks incl. 0 and 1."""
    path, spec = _model_file(tmp_path, f"lsr_{kind}{hidden}x{n_rnn}", kind=kind, hidden=hidden, input_size=1, seed=77 + hidden, n_rnn=n_rnn)
    S = 300
    sizes = [max_frames, 1, 0, 37, 255] if max_frames == 256 else [700, 16, 3, 513]
    x = modelgen.signal(S, sum(sizes), seed=35)
    cg, co = _ctl_pair(param1=0.4, param2=0.7, pregain_db=-1.0)
    outs, states = {}, {}
    for form in ("one", "ranges"):
        monkeypatch.delenv("AIDAX_LP_ROUND_GROUPS", raising=False)
        if form == "ranges":
            monkeypatch.setenv("AIDAX_LP_ROUND_GROUPS", "8")
        pool = ax.Pool(S, max_frames)
        pool.set_model(ax.Model(path))
        assert pool.kernel_name == ("k_mfma_ls" if max_frames == 256 else "k_chain+k_mfma_ls"), pool.kernel_name
        pool.set_controls(cg)
        got, pos = [], 0
        for n in sizes:
            got.append(pool.process(np.ascontiguousarray(x[:, pos:pos + n])))
            pos += n
        outs[form] = np.concatenate(got, axis=1)
        states[form] = [pool.read_state(stream=s_, layer=n_rnn - 1, hidden=128) for s_ in (0, 127, 128, 255, 256, S - 1)]
        pool.close()
    assert np.array_equal(outs["one"].view(np.uint32), outs["ranges"].view(np.uint32))
    for a_, b_ in zip(states["one"], states["ranges"]):
        for u, v in zip(a_, b_):
            assert np.array_equal(np.asarray(u).view(np.uint32), np.asarray(v).view(np.uint32))
    for s_ in (0, 127, 128, 256, S - 1):                      # first / last stream of a range, the ragged tail
        pl = O.OraclePlugin()
        pl.set_model(O.OracleModel(spec))
        want = pl.run(co, x[s_])
        errlog.bound(np.abs(outs["ranges"][s_] - want).max(), 2e-6, "gpu_parity:ls_ranges")


@pytest.mark.parametrize("name,kw", [
    ("lstm96x2", dict(kind="lstm", hidden=96, input_size=1, seed=96, n_rnn=2)),          # BASELINE cfg #5 model
    ("gru48x3", dict(kind="gru", hidden=48, input_size=3, seed=483, n_rnn=3)),            # three layers: a middle workgroup both consumes and produces
    ("l16x4", dict(kind="lstm", hidden=16, input_size=2, seed=164, n_rnn=4, in_skip=1)),
])
@pytest.mark.parametrize("placement", ["ids 8 apart (one XCD)", "adjacent ids (two XCDs)"])
def test_layer_pipelined_kernel_keeps_the_state_of_the_one_workgroup_kernel_bit_for_bit(name, kw, placement, tmp_path, monkeypatch):
    """k_mfma_lp (one workgroup per layer, layers chained through a global ring, weights in registers) against
    k_mfma (one workgroup walks all layers, AIDAX_MFMA_LP=0) on the same fragments: identical state bits, over ragged
    block sizes incl. blocks longer than the ring and the 256-frame staging chunk, 150 streams (10 stream groups,
    the last one ragged) so that several groups and layers are in flight at once, and against the oracle."""
    path, spec = _model_file(tmp_path, name, **kw)
    S = 150
    sizes = [256, 1, 5, 700, 16, 3, 255, 40]
    x = modelgen.signal(S, sum(sizes), seed=27)
    cg, co = _ctl_pair(param1=0.3, param2=0.8, pregain_db=1.0)
    outs = {}
    if placement.startswith("adjacent"):
        monkeypatch.setenv("AIDAX_TUNE", "2")       # the hand-over must not depend on where the two workgroups run
    for lp in ("1", "0", "s"):                      # k_mfma_lp (fp32 MFMAs), k_mfma, k_mfma_ls (bf16 term products of split operands)
        monkeypatch.setenv("AIDAX_MFMA_LP", "0" if lp == "0" else "1")
        monkeypatch.setenv("AIDAX_LP_SPLIT", "1" if lp == "s" else "0")
        pool = ax.Pool(S, 1024)
        pool.set_model(ax.Model(path))
        assert pool.kernel_name == {"1": "k_chain+k_mfma_lp", "0": "k_chain+k_mfma", "s": "k_chain+k_mfma_ls"}[lp]
        pool.set_controls(cg)
        got, pos = [], 0
        for n in sizes:
            got.append(pool.process(np.ascontiguousarray(x[:, pos:pos + n])))
            pos += n
        outs[lp] = np.concatenate(got, axis=1)
        h, c = pool.read_state(stream=S - 1, layer=kw["n_rnn"] - 1, hidden=128)
        outs[lp + "h"] = h
        pool.close()
    # same fragments, same accumulation order, same activations: the recurrent state is bit-identical; the outputs
    # differ only by the order in which Dense(H,1) is summed (per-wave partial sums on the matrix cores there, an
    # fma chain + lane tree here)
    assert np.array_equal(outs["1h"], outs["0h"])
    errlog.bound(np.abs(outs["1"] - outs["0"]).max(), 5e-7, "gpu_parity:lp_vs_mfma_outputs")
    # the split kernel sums other terms in another order: state and outputs agree with the fp32 kernels' to rounding
    errlog.bound(np.abs(outs["sh"] - outs["1h"]).max(), 2e-6, "gpu_parity:ls_vs_lp_state")
    errlog.bound(np.abs(outs["s"] - outs["1"]).max(), 2e-6, "gpu_parity:ls_vs_lp_outputs")
    for s_ in (0, 17, S - 1):
        want = O.run_streams(spec, co, x[s_:s_ + 1], 4096)       # block partition does not matter to the oracle
        errlog.bound(np.abs(outs["1"][s_] - want[0]).max(), 2e-6, "gpu_parity:lp_vs_oracle")
        errlog.bound(np.abs(outs["s"][s_] - want[0]).max(), 2e-6, "gpu_parity:ls_vs_oracle")


# ------------------------------------------------- k_lstm_pipe4: four streams per workgroup, one helper wave (round 6)

def _pipe4_run(path, S, sizes, x, schedule):
    """one pool through the block sequence; schedule[block index] = list of (stream or None, controls kwargs) applied before that block"""
    pool = ax.Pool(S, 256)
    pool.set_model(ax.Model(path))
    names = [pool.kernel_name]
    got = np.empty_like(x)
    pos = 0
    for bi, n in enumerate(sizes):
        for s_, kw in schedule.get(bi, []):
            if s_ == "activate":
                pool.activate()
            elif s_ is None:
                pool.set_controls(ax.default_controls(**kw))
            else:
                pool.set_controls(ax.default_controls(**kw), stream=s_)
        names.append(pool.kernel_name)
        got[:, pos:pos + n] = pool.process(np.ascontiguousarray(x[:, pos:pos + n]))
        pos += n
    pool.close()
    return got, names


def test_four_streams_per_workgroup_pipeline_matches_the_oracle(tmp_path):
    """k_lstm_pipe4<32> (BASELINE cfg2's cell: a CU's four streams in one workgroup, four free-running recurrent waves and ONE helper wave that
    carries all four streams' chain passes side by side, paced by progress words in LDS: profiles/r06_cfg2_pipe4.txt) with no switch set —
    whole-tile blocks run there — streams that are disabled or have their model bypassed ride along, the last workgroup has two streams —
    and every ragged block runs k_lstm_pipe<32> on the same state. Per-stream
    controls: EQ in front of and behind the model on some streams (six-stage cascades next to one-stage ones in the same wave), gain ramps
    that move, activate(); against the oracle's plugin mirror per stream."""
    path, spec = _model_file(tmp_path, "l32p4", kind="lstm", hidden=32, input_size=1, seed=32, in_skip=1, in_gain=-2.0, out_gain=1.5)
    S = 10
    sizes = [256, 64, 16, 128, 100, 256, 0, 1, 48, 256, 256, 32]
    x = modelgen.signal(S, sum(sizes), seed=77)
    per = [dict(), dict(eq_position=1.0, bass_boost_db=5.0, mid_boost_db=-2.0), dict(treble_boost_db=3.0, depth_boost_db=2.0),
           dict(eq_position=1.0, mid_type=1.0, mid_boost_db=4.0), dict(dc_blocker=0.0, in_lpf_pc=0.0), dict(eq_bypass=1.0, pregain_db=3.0),
           dict(pregain_db=-6.0, master_db=-3.0), dict(eq_position=1.0, presence_boost_db=4.0, in_lpf_pc=30.0), dict(net_bypass=1.0), dict(master_db=2.0)]
    schedule = {0: [(s_, per[s_]) for s_ in range(S)],
                3: [(2, dict(per[2], pregain_db=6.0, master_db=-6.0))],                      # ramps move on one stream: the general macro-step
                5: [("activate", None)],
                8: [(5, dict(per[5], enabled=0.0)), ("activate", None)],                     # a stream disabled (a raw copy; activate() still latches its gains)
                9: [(5, per[5])],
                10: [(1, dict(per[1], net_bypass=1.0)), (8, per[0])]}                         # one model goes out of circuit, another comes back in
    got, names = _pipe4_run(path, S, sizes, x, schedule)
    assert set(names) == {"k_lstm_pipe4<32>"}, names
    plugs = [O.OraclePlugin() for _ in range(S)]
    for p_ in plugs:
        p_.set_model(O.OracleModel(spec))
    cur = [dict() for _ in range(S)]
    worst, pos = 0.0, 0
    for bi, n in enumerate(sizes):
        for s_, kw in schedule.get(bi, []):
            if s_ == "activate":
                for p_ in plugs:
                    p_.activate()
            else:
                cur[s_] = kw
        for s_ in range(S):
            want = plugs[s_].run(O.default_controls(**cur[s_]), x[s_, pos:pos + n])
            if n:
                worst = max(worst, float(np.abs(got[s_, pos:pos + n] - want).max()))
        pos += n
    errlog.bound(worst, 2e-6, "gpu_parity:pipe4")


def test_four_streams_per_workgroup_pipeline_is_bit_identical_to_the_three_wave_pipeline(tmp_path, monkeypatch):
    """... and against k_lstm_pipe<32> serving every pass (AIDAX_PIPE4=0, test build): same operations per sample in the same order, the same bits."""
    path, _ = _model_file(tmp_path, "l32p4b", kind="lstm", hidden=32, input_size=1, seed=33, in_skip=0, in_gain=1.0, out_gain=-1.0)
    S = 13
    sizes = [256, 64, 16, 128, 100, 256, 48, 256]
    x = modelgen.signal(S, sum(sizes), seed=78)
    per = [dict(), dict(eq_position=1.0, bass_boost_db=5.0), dict(treble_boost_db=3.0), dict(eq_position=1.0, mid_type=1.0, mid_boost_db=4.0)]
    schedule = {0: [(s_, per[s_ % 4]) for s_ in range(S)], 2: [(3, dict(per[3], pregain_db=4.0))], 4: [("activate", None)],
                5: [(2, dict(per[2], enabled=0.0)), (7, dict(per[3], net_bypass=1.0))], 6: [("activate", None)], 7: [(2, per[2])]}
    a, na = _pipe4_run(path, S, sizes, x, schedule)
    monkeypatch.setenv("AIDAX_PIPE4", "0")
    b, nb = _pipe4_run(path, S, sizes, x, schedule)
    assert na[1] == "k_lstm_pipe4<32>" and set(nb) == {"k_lstm_pipe<32>"}, (na, nb)
    assert np.array_equal(a, b)


_P4_PLAIN = [("lstm", 8), ("lstm", 12), ("lstm", 16), ("lstm", 20), ("gru", 8), ("gru", 12), ("gru", 16), ("gru", 24)]
_P4_CONDITIONED = [("lstm", 12, 2), ("lstm", 16, 3), ("gru", 8, 3), ("gru", 12, 2), ("lstm", 32, 2), ("lstm", 32, 3),
                   ("lstm", 20, 3), ("lstm", 24, 2), ("gru", 20, 2), ("gru", 24, 3), ("gru", 32, 3)]


def _p4_case(tmp_path, kind, hidden, inputs, streams=7):
    """a pool's worth of streams, a block sequence of whole tiles (k_*_pipe4) with ragged blocks between (k_*_pipe on the same state), per-stream
    controls that move: (model path, spec, S, sizes, x, schedule)"""
    if inputs == 1:
        path, spec = _model_file(tmp_path, f"{kind}{hidden}p4", kind=kind, hidden=hidden, input_size=1, seed=100 + hidden, in_skip=hidden % 16 == 0, in_gain=1.5, out_gain=-2.0)
        S, sizes = 8, [256, 64, 100, 32, 256, 128]
        per = [dict(), dict(eq_position=1.0, bass_boost_db=5.0), dict(treble_boost_db=3.0, dc_blocker=0.0), dict(eq_position=1.0, mid_type=1.0, mid_boost_db=4.0)]
        schedule = {0: [(s_, per[s_ % 4]) for s_ in range(S)], 2: [(5, dict(per[1], pregain_db=4.0, master_db=-5.0))], 4: [("activate", None)]}
        return path, spec, S, sizes, modelgen.signal(S, sum(sizes), seed=79 + hidden), schedule
    path, spec = _model_file(tmp_path, f"{kind}{hidden}i{inputs}p4", kind=kind, hidden=hidden, input_size=inputs, seed=300 + hidden + inputs,
                             in_skip=1, in_gain=1.25, out_gain=-1.5)
    S, sizes = streams, [256, 64, 128, 32, 256, 16, 100, 128]
    per = [dict(param1=0.2 + 0.1 * s_, param2=0.9 - 0.1 * s_, **(dict(eq_position=1.0, bass_boost_db=4.0) if s_ % 3 == 1 else {})) for s_ in range(7)]
    schedule = {0: [(s_, per[s_]) for s_ in range(7)],
                1: [(2, dict(per[2], param1=0.95)), (4, dict(per[4], param2=0.05, net_bypass=1.0))],      # a ramp starts; a model out of circuit whose PARAMs move
                2: [(2, dict(per[2], param1=0.5, param2=0.5)), (6, dict(per[6], param1=0.0))],             # a new target while the ramp is under way
                4: [("activate", None), (4, dict(per[4], param1=0.7, param2=0.3))],                          # the model back in circuit
                5: [(0, dict(per[0], param1=1.0, param2=0.0, pregain_db=3.0))],
                6: [(3, dict(per[3], param1=0.1))]}                                                         # (block 6 is ragged: k_*_pipe takes the ramp over, block 7 hands it back)
    schedule = {b: [(s_, kw) for s_, kw in ev if s_ == "activate" or s_ < S] for b, ev in schedule.items()}
    return path, spec, S, sizes, modelgen.signal(S, sum(sizes), seed=91 + hidden), schedule


def _p4_oracle_worst(spec, S, sizes, x, schedule, got):
    plugs = [O.OraclePlugin() for _ in range(S)]
    for p_ in plugs:
        p_.set_model(O.OracleModel(spec))
    cur = [dict() for _ in range(S)]
    worst, pos = 0.0, 0
    for bi, n in enumerate(sizes):
        for s_, kw in schedule.get(bi, []):
            if s_ == "activate":
                for p_ in plugs:
                    p_.activate()
            else:
                cur[s_] = kw
        for s_ in range(S):
            want = plugs[s_].run(O.default_controls(**cur[s_]), x[s_, pos:pos + n])
            worst = max(worst, float(np.abs(got[s_, pos:pos + n] - want).max()))
        pos += n
    return worst


@pytest.mark.parametrize("kind,hidden", _P4_PLAIN)
def test_four_streams_per_workgroup_pipeline_small_cells(kind, hidden, tmp_path):
    """The other cells of the reference's table that run k_*_pipe4 (where it measured ahead of the three-wave pipeline at a full pool:
    profiles/r06_pipe4_cells.txt — the sizes the reference's own models have, LSTM-12 / 16): against the oracle's plugin mirror per stream
    with per-stream EQ placement and moving ramps. (No switch set: both builds run this, and their outputs are compared bit for bit.)"""
    path, spec, S, sizes, x, schedule = _p4_case(tmp_path, kind, hidden, 1)
    got, names = _pipe4_run(path, S, sizes, x, schedule)
    assert names[1] == f"k_{kind}_pipe4<{hidden}>", names
    errlog.bound(_p4_oracle_worst(spec, S, sizes, x, schedule, got), 2e-6, "gpu_parity:pipe4_small")


@pytest.mark.parametrize("kind,hidden,inputs", _P4_CONDITIONED)
def test_four_streams_per_workgroup_pipeline_conditioned_models(kind, hidden, inputs, tmp_path):
    """Conditioned models (PARAM1 / PARAM2 as model inputs, rt-neural-generic.cpp:175-189) in k_*_pipe4<H, conditioned>: the helper wave's
    PARAM lanes run the linear smoothers a value per frame into LDS rows beside the audio tile. Per-stream PARAM targets that move between
    blocks (ramps still under way when the next target arrives, and handed to k_*_pipe and back at a ragged block), a first run that snaps,
    activate(), a stream whose model is out of circuit while its PARAMs change; against the oracle's plugin mirror. Conditioned, every cell
    of the table up to 32 runs here (profiles/r06_pipe4_cells.txt) — also LSTM-20 / 24 and GRU-20 / 24 / 32, whose plain models keep k_*_pipe."""
    path, spec, S, sizes, x, schedule = _p4_case(tmp_path, kind, hidden, inputs)
    got, names = _pipe4_run(path, S, sizes, x, schedule)
    assert set(names[1:]) == {f"k_{kind}_pipe4<{hidden}>"}, names
    errlog.bound(_p4_oracle_worst(spec, S, sizes, x, schedule, got), 2e-6, "gpu_parity:pipe4_conditioned")


@pytest.mark.parametrize("streams", [1, 3])
@pytest.mark.parametrize("kind,hidden,inputs", [("lstm", 16, 2), ("gru", 8, 3), ("lstm", 32, 3)])
def test_four_streams_per_workgroup_pipeline_conditioned_small_pools(kind, hidden, inputs, streams, tmp_path):
    """a conditioned model runs k_*_pipe4 also below one full workgroup — the LV2 instance's pool of one stream (11 - 20 % ahead of the
    three-wave pipeline there: profiles/r06_pipe4_cells.txt); a plain model's small pool keeps k_*_pipe"""
    path, spec, S, sizes, x, schedule = _p4_case(tmp_path, kind, hidden, inputs, streams=streams)
    got, names = _pipe4_run(path, S, sizes, x, schedule)
    assert set(names[1:]) == {f"k_{kind}_pipe4<{hidden}>"}, names
    errlog.bound(_p4_oracle_worst(spec, S, sizes, x, schedule, got), 2e-6, "gpu_parity:pipe4_conditioned")
    path1, _, S1, sizes1, x1, schedule1 = _p4_case(tmp_path, kind, hidden, 1)
    pool = ax.Pool(streams, 256)
    pool.set_model(ax.Model(path1))
    assert pool.kernel_name == f"k_{kind}_pipe<{hidden}>"
    pool.close()


@pytest.mark.parametrize("kind,hidden,inputs", [(k, h, 1) for k, h in _P4_PLAIN] + _P4_CONDITIONED)
def test_four_streams_per_workgroup_pipeline_equals_the_three_wave_pipeline(kind, hidden, inputs, tmp_path, monkeypatch):
    """the same runs, bit for bit, with k_*_pipe serving every pass (AIDAX_PIPE4=0, test build)"""
    path, spec, S, sizes, x, schedule = _p4_case(tmp_path, kind, hidden, inputs)
    got, names = _pipe4_run(path, S, sizes, x, schedule)
    assert f"k_{kind}_pipe4<{hidden}>" in names, names
    monkeypatch.setenv("AIDAX_PIPE4", "0")
    ref, names0 = _pipe4_run(path, S, sizes, x, schedule)
    assert set(names0) == {f"k_{kind}_pipe<{hidden}>"}, names0
    assert np.array_equal(got, ref)
