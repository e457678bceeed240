"""Stream meters, host side (no device): the record's layout as the binding sees it, and the calls' answers for a null pool."""
import ctypes as C
import importlib

import numpy as np

ax = importlib.import_module("aidadsp-lv2_amd")

ERR_ARG = -1
HEADER_ORDER = (("frames", 8), ("passes", 8), ("in_nonfinite", 8), ("out_nonfinite", 8), ("out_over", 8), ("in_energy", 8),
                ("out_energy", 8), ("in_peak", 4), ("out_peak", 4))


def test_the_record_is_64_bytes_in_header_order():
    assert C.sizeof(ax.StreamMeter) == 64
    at = 0
    for (name, size), (got, _) in zip(HEADER_ORDER, ax.StreamMeter._fields_):
        assert got == name
        f = getattr(ax.StreamMeter, name)
        assert (f.offset, f.size) == (at, size), name
        at += size
    assert at == 64 and len(ax.StreamMeter._fields_) == len(HEADER_ORDER)
    # ... and the structured array Pool.read_meters returns is that record, field for field
    assert ax.METER_DTYPE.itemsize == 64 and ax.METER_DTYPE.names == tuple(n for n, _ in HEADER_ORDER)
    assert [ax.METER_DTYPE.fields[n][1] for n, _ in HEADER_ORDER] == [getattr(ax.StreamMeter, n).offset for n, _ in HEADER_ORDER]


def test_the_calls_are_declared_and_exported():
    for name in ("aidax_pool_set_metering", "aidax_pool_metering", "aidax_pool_read_meters"):
        assert name in ax.declared_symbols() and hasattr(ax.lib(), name)


def test_a_null_pool_is_an_argument_error_without_a_device():
    L = ax.lib()
    assert L.aidax_pool_set_metering(None, 1) == ERR_ARG and b"null" in L.aidax_last_error()
    assert L.aidax_pool_set_metering(None, 0) == ERR_ARG
    rec = np.zeros(1, ax.METER_DTYPE)
    out = rec.ctypes.data_as(C.POINTER(ax.StreamMeter))
    assert L.aidax_pool_read_meters(None, 0, 1, out, 0) == ERR_ARG and b"null" in L.aidax_last_error()
    assert L.aidax_pool_read_meters(None, 0, 1, out, 1) == ERR_ARG
    assert rec.tobytes() == bytes(64)
    assert L.aidax_pool_metering(None) == 0
