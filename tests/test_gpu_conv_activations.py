"""The conv epilogues' activations at saturation, through the overflow of exp and around 0 (run with -m gpu on an MI355X): the probe
stacks of tests/convprobes.py — the model's output is ONE evaluation of tanh_exp_pre or fast_sigmoid on the observed channel — on every
conv kernel form, with `pool.kernel_name` asserted. tests/test_gpu_activations.py does this for the recurrent cells; the conv call sites
(cs_activate in aidax_convs.hip, the switches of aidax_convm.hip and of k_conv, k_conv_st's mixed instantiation) were only ever called with
|z| of order 1.

Per sample (tests/convprobes.py derives both, tests/test_conv_probes_reference.py establishes them on the CPU):
  * where float32's own function returns exactly 0, 1 or -1 — tanh from |z| = 17 on and at 0, the sigmoid from 17 up and from -110 down —
    the pool's output equals the oracle's bit for bit;
  * everywhere else it stays within the bound computed from the header's per-instruction ulp budget and the rounding of the
    pre-activation. Nothing here is a measured tolerance; the measured maxima, as fractions of the bound and in absolute terms, go to the
    session's parity error log through tests/errlog.py (tags probe:conv:<activation>:<form>:...; profiles/activation_probe_errors.json);
  * no NaN or infinity at any probe.
The forms that set no switch run on the shipped library too."""
import importlib
import json

import numpy as np
import pytest

from tests import convprobes as cp, errlog

pytestmark = pytest.mark.gpu
ax = importlib.import_module("aidadsp-lv2_amd")

CONTROLS = dict(in_lpf_pc=0.0, dc_blocker=0.0, eq_bypass=1.0)
RAGGED = [256, 100, 156, 256, 255, 1]                    # the two-layer probe: full blocks (k_conv_ms<FULL>) and ragged ones
STREAMED = [256, 128, 64, 64, 256, 256]                  # the StGeoC shape: every block length k_conv_st is compiled for
assert sum(RAGGED) == sum(STREAMED) == cp.FRAMES
# form: (shape, switches, kernel name, block plan)
FORMS = {
    "ms": ("two layers", {}, "k_conv_ms", RAGGED),
    "st": ("StGeoC", {}, "k_conv_st", STREAMED),
    "st-ragged": ("StGeoC", {}, "k_conv_st", RAGGED),                                   # (the ragged blocks of such a pool: k_conv_ms)
    "st0": ("StGeoC", {"AIDAX_CONV_ST": "0"}, "k_conv_ms", STREAMED),
    "split": ("two layers", {"AIDAX_CONV_FUSED": "0"}, "k_chain+k_conv_ms", RAGGED),
    "mfma": ("two layers", {"AIDAX_CONV_MS": "0"}, "k_conv_mfma", RAGGED),
    "mfma-split": ("two layers", {"AIDAX_CONV_MS": "0", "AIDAX_CONV_FUSED": "0"}, "k_chain+k_conv_mfma", RAGGED),
    "valu": ("two layers", {"AIDAX_KERNEL": "valu"}, "k_conv", RAGGED),
}
PLAIN = [f for f, v in FORMS.items() if not v[1]]
FORCED = [f for f, v in FORMS.items() if v[1]]


def _probe(form, act, observed):
    shape, _, name, plan = FORMS[form]
    r = cp.pool_reference(act, observed, shape)
    S = cp.STREAMS
    pool = ax.Pool(S, 256)
    pool.set_model(ax.Model(text=json.dumps(r["j"])))
    assert pool.kernel_name == name, (pool.kernel_name, name)
    pool.set_controls(ax.default_controls(**CONTROLS))
    got = np.zeros_like(r["x"])
    pos = 0
    for n in plan:
        got[:, pos:pos + n] = pool.process(np.ascontiguousarray(r["x"][:, pos:pos + n]))
        pos += n
    pool.close()
    tag = f"probe:conv:{act}:{form}"
    assert np.all(np.isfinite(got)), (tag, np.argwhere(~np.isfinite(got))[:3])
    exact = r["exact"]
    bad = np.argwhere(exact & (got != r["want"]))
    assert bad.size == 0, (tag, "not the exact bits", len(bad), [(float(r["z"][s, t]), float(got[s, t]), float(r["want"][s, t])) for s, t in bad[:4]])
    err = np.abs(got.astype(np.float64) - r["ref"])
    ratio = np.where(exact, 0.0, err / r["allowed"])
    worst = np.unravel_index(np.argmax(ratio), ratio.shape)
    print(f"{tag} ch{observed}: worst {ratio[worst]:.3f} of the bound at z = {r['z'][worst]:.6g} (error {err[worst]:.3g}); largest error {err[~exact].max():.3g}")
    errlog.bound(ratio.max(), 1.0, tag + ":over_bound")
    errlog.bound(err[~exact].max(), float(r["allowed"][~exact].max()), tag + ":abs")


@pytest.mark.parametrize("observed", cp.OBSERVED)
@pytest.mark.parametrize("act", ["tanh", "sigmoid"])
@pytest.mark.parametrize("form", PLAIN)
def test_conv_activation_probe_as_the_pool_runs_it(form, act, observed):
    _probe(form, act, observed)


@pytest.mark.parametrize("observed", cp.OBSERVED)
@pytest.mark.parametrize("act", ["tanh", "sigmoid"])
@pytest.mark.parametrize("form", FORCED)
def test_conv_activation_probe_on_a_forced_form(form, act, observed, monkeypatch):
    for k, v in FORMS[form][1].items():
        monkeypatch.setenv(k, v)
    _probe(form, act, observed)
