"""The model bank's host side (no GPU): aidax_model_bank_compatible over synthetic models, the argument checks of the four pool calls
that need no device, and the binding's constants against the header."""
import ctypes as C
import importlib
import json
import os
import re

import pytest

from tests import modelgen

ax = importlib.import_module("aidadsp-lv2_amd")
ERR_ARG, ERR_ARCH = -1, -4
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _model(**kw):
    return ax.Model(text=json.dumps(modelgen.make_model(**kw)), label="bank")


def _rc(a, b):
    return ax.lib().aidax_model_bank_compatible(a.h, b.h)


def test_equal_architecture_is_compatible_whatever_the_weights_gains_and_skip():
    for kind, hidden, isz in (("lstm", 32, 1), ("gru", 8, 1), ("lstm", 16, 3), ("gru", 40, 2)):
        pool = _model(kind=kind, hidden=hidden, input_size=isz, seed=1)
        for kw in (dict(seed=2), dict(seed=3, in_skip=1), dict(seed=4, in_gain=-3.0, out_gain=4.5), dict(seed=1)):
            m = _model(kind=kind, hidden=hidden, input_size=isz, **kw)
            assert _rc(pool, m) == 0 and _rc(m, pool) == 0, (kind, hidden, isz, kw)
            assert ax.bank_compatible(pool, m)
    # a numeric sample rate that both files carry is an equal one
    a, b = _model(kind="lstm", hidden=12, seed=1, samplerate=44100), _model(kind="lstm", hidden=12, seed=2, samplerate=44100)
    assert _rc(a, b) == 0


@pytest.mark.parametrize("field,other", [
    ("cell", dict(kind="gru", hidden=16, input_size=1)),
    ("hidden", dict(kind="lstm", hidden=20, input_size=1)),
    ("input_size", dict(kind="lstm", hidden=16, input_size=2)),
    ("samplerate", dict(kind="lstm", hidden=16, input_size=1, samplerate=44100)),
])
def test_a_mismatch_names_its_field(field, other):
    pool = _model(kind="lstm", hidden=16, input_size=1, seed=1)
    m = _model(seed=2, **other)
    for a, b in ((pool, m), (m, pool)):
        assert _rc(a, b) == ERR_ARCH
        msg = ax.last_error()
        assert re.search(rf"\b{field}\b", msg), msg
    assert not ax.bank_compatible(pool, m)


@pytest.mark.parametrize("kw", [dict(kind="lstm", hidden=16, n_rnn=2), dict(kind="conv", hidden=16), dict(kind="gru", hidden=128)])
def test_stacked_wide_and_conv_models_are_refused_on_either_side(kw):
    table = _model(kind="lstm", hidden=16, seed=1)
    ext = _model(seed=2, **kw)
    assert _rc(table, ext) == ERR_ARCH and "one-layer" in ax.last_error()
    assert _rc(ext, table) == ERR_ARCH and "one-layer" in ax.last_error()
    assert _rc(ext, ext) == ERR_ARCH


def test_null_and_out_of_range_arguments_need_no_device():
    L = ax.lib()
    m = _model(kind="lstm", hidden=16, seed=1)
    sg = C.c_void_p(0x1234)
    slot = C.c_int32(7)
    assert L.aidax_model_bank_compatible(None, m.h) == ERR_ARG and L.aidax_model_bank_compatible(m.h, None) == ERR_ARG
    assert L.aidax_pool_prepare_model_slot(None, 0, m.h, C.byref(sg)) == ERR_ARG and not sg.value      # *out is cleared
    assert L.aidax_pool_prepare_model_slot(None, ax.MODEL_SLOTS, m.h, C.byref(sg)) == ERR_ARG
    assert L.aidax_pool_prepare_model_slot(None, 0, m.h, None) == ERR_ARG
    assert L.aidax_pool_set_model_slot(None, 0, m.h) == ERR_ARG
    assert L.aidax_pool_set_model_slot(None, ax.MODEL_SLOTS, None) == ERR_ARG
    assert L.aidax_pool_assign_model(None, 0, 0, ax.START_WARMUP) == ERR_ARG
    assert L.aidax_pool_assign_model(None, ax.ALL_STREAMS, ax.MODEL_POOL, ax.START_RESET) == ERR_ARG
    assert L.aidax_pool_stream_model(None, 0, C.byref(slot)) == ERR_ARG
    assert ax.last_error()


def test_the_bindings_constants_are_the_headers():
    with open(os.path.join(ROOT, "include", "aidax.h")) as f:
        text = f.read()
    assert int(re.search(r"#define\s+AIDAX_MODEL_SLOTS\s+(\d+)", text).group(1)) == ax.MODEL_SLOTS == 64
    assert int(re.search(r"AIDAX_MODEL_POOL\s*=\s*(-?\d+)", text).group(1)) == ax.MODEL_POOL == -1
    for name in ("aidax_model_bank_compatible", "aidax_pool_prepare_model_slot", "aidax_pool_set_model_slot", "aidax_pool_assign_model",
                 "aidax_pool_stream_model"):
        assert name in ax.declared_symbols() and hasattr(ax.lib(), name)
