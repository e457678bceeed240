"""Per-stream cabinet IRs, the parts that need no device: the constants of include/aidax.h and the binding's mirror of them, the new entry
points' exports, and the argument checks made before any device is touched."""
import ctypes as C
import importlib
import re

from tests.conftest import ROOT

ax = importlib.import_module("aidadsp-lv2_amd")
ERR_ARG = -1
NEW = ("aidax_pool_prepare_ir_slot", "aidax_pool_set_ir_slot", "aidax_pool_assign_ir", "aidax_pool_stream_ir")


def _header():
    with open(f"{ROOT}/include/aidax.h") as f:
        return f.read()


def test_bank_constants_in_the_header_and_the_binding():
    h = _header()
    assert re.search(r"#define AIDAX_IR_SLOTS 64\b", h)
    assert re.search(r"enum \{ AIDAX_IR_POOL = -1, AIDAX_IR_NONE = -2 \};", h)
    assert (ax.IR_SLOTS, ax.IR_POOL, ax.IR_NONE) == (64, -1, -2)


def test_new_entry_points_are_declared_and_exported():
    names = ax.declared_symbols()
    L = ax.lib()
    for n in NEW:
        assert n in names, n
        assert hasattr(L, n), n
    # the thread contract names them on their sides
    threads = _header().split("/* Threads.")[1].split("*/")[0]
    assert "assign_ir" in threads.split("plus, concurrently")[0]
    assert "prepare_ir_slot" in threads.split("plus, concurrently")[1]


def test_argument_checks_without_a_pool():
    L = ax.lib()
    slot = C.c_int32(123)
    sg = C.c_void_p(1)
    assert L.aidax_pool_assign_ir(None, 0, 0) == ERR_ARG
    assert L.aidax_pool_assign_ir(None, ax.ALL_STREAMS, ax.IR_NONE) == ERR_ARG
    assert L.aidax_pool_stream_ir(None, 0, C.byref(slot)) == ERR_ARG and slot.value == 123
    assert L.aidax_pool_prepare_ir_slot(None, 0, None, 0, 48000.0, C.byref(sg)) == ERR_ARG
    assert L.aidax_pool_prepare_ir_slot(None, ax.IR_SLOTS, None, 0, 48000.0, C.byref(sg)) == ERR_ARG
    assert sg.value is None                                             # *out is cleared on a refusal
    assert "slot" in L.aidax_last_error().decode()
    assert L.aidax_pool_set_ir_slot(None, 0, None, 0, 48000.0) == ERR_ARG
