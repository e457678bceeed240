"""aidadsp-lv2_amd — MI355X-native hot path of AIDA-X's rt-neural-generic plugin.

The product is the C-ABI shared library ``lib/libaidax_hip.so`` (declared in
``include/aidax.h``) and the LV2 shell ``lv2/rt-neural-generic.so`` that calls it.
This Python package is only a thin ctypes binding over that C ABI for tests and
``bench.py``; it adds no compute of its own and has no CPU fallback.

The directory name carries a hyphen, so import it with
``importlib.import_module("aidadsp-lv2_amd")``.
"""
from .binding import (  # noqa: F401
    AidaxError, Controls, StreamDsp, StreamMeter, METER_DTYPE, GateParams, GateRec, GateState, GATE_STATE_DTYPE, gate_design, TunerParams, TunerRec, TunerReading, TunerReadingStruct, tuner_params, tuner_design, tuner_note, mix_gain, BusLimitParams, BusLimitRec, BusMeter, BUS_METER_DTYPE, bus_limit_design, BusReverbParams, BusReverbRec, bus_reverb_design, DelayParams, DelayRec, DelayState, DelayStateStruct, delay_design, DELAY_MIN, DELAY_MAX, Hub, Model, ModelInfo, Pool, Resampler, RateAdapter, lib, lib_path, default_controls,
    biquad_design, db_to_coeff, lpf_fc, declared_symbols, load_ir_wav, load_ir_wav_for, resample_ir, resampler_row, rate_latency, device_count, pick_device, pick_hub, many_streams_form, bank_compatible, last_error,
    ALL_STREAMS, START_WARMUP, START_RESET, IR_SLOTS, IR_POOL, IR_NONE, MODEL_SLOTS, MODEL_POOL, SENDS, BUS_NONE, MAX_BUSES, ALL_BUSES, BUS_LOOKAHEAD_MAX, BUS_HOLD_MAX, BUS_REVERB_LINES, BUS_REVERB_MIN_DELAY, BUS_REVERB_MAX_DELAY,
)
from . import workloads  # noqa: F401,E402
