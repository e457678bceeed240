"""ctypes binding of include/aidax.h (no logic beyond argument marshalling)."""
from __future__ import annotations

import ctypes as C
import os
import re
import weakref
from typing import Optional

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(_HERE)
_HEADER = os.path.join(_ROOT, "include", "aidax.h")

ALL_STREAMS = -1
START_WARMUP, START_RESET = 0, 1
IR_SLOTS = 64                     # AIDAX_IR_SLOTS: bank slots per pool, besides the pool IR
IR_POOL, IR_NONE = -1, -2         # a stream's IR: the pool IR (default), none, or a bank slot 0 .. IR_SLOTS - 1
MODEL_SLOTS = 64                  # AIDAX_MODEL_SLOTS: model-bank slots per pool, besides the pool model
MODEL_POOL = -1                   # a stream's model: the pool model (default) or a bank slot 0 .. MODEL_SLOTS - 1
SENDS = 4                         # AIDAX_SENDS: sends per stream into the pool's mix buses
BUS_NONE = -1                     # AIDAX_BUS_NONE: a send that goes nowhere (the default)
MAX_BUSES = 4096                  # AIDAX_MAX_BUSES
ALL_BUSES = -1                    # AIDAX_ALL_BUSES: every bus's limiter
BUS_LOOKAHEAD_MAX, BUS_HOLD_MAX = 512, 4096      # AIDAX_BUS_LOOKAHEAD_MAX, AIDAX_BUS_HOLD_MAX: frames
BUS_REVERB_LINES, BUS_REVERB_MIN_DELAY, BUS_REVERB_MAX_DELAY = 8, 64, 32768      # AIDAX_BUS_REVERB_*: lines per bus, frames
_fp = C.POINTER(C.c_float)


class AidaxError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"aidax error {code}: {msg}")
        self.code = code


class ModelInfo(C.Structure):
    _fields_ = [("cell", C.c_int32), ("hidden", C.c_int32), ("input_size", C.c_int32),
                ("n_rnn_layers", C.c_int32), ("input_skip", C.c_int32),
                ("input_gain", C.c_float), ("output_gain", C.c_float), ("samplerate", C.c_float),
                ("n_golden", C.c_int32), ("in_reference_set", C.c_int32), ("n_weights", C.c_uint64)]


CONTROL_FIELDS = ("in_lpf_pc", "pregain_db", "net_bypass", "param1", "param2", "eq_bypass",
                  "eq_position", "bass_boost_db", "bass_freq", "mid_boost_db", "mid_freq", "mid_q",
                  "mid_type", "treble_boost_db", "treble_freq", "depth_boost_db",
                  "presence_boost_db", "dc_blocker", "master_db", "enabled")


class StreamDsp(C.Structure):
    _fields_ = [("z", (C.c_double * 2) * 7), ("pre_mem", C.c_float), ("master_mem", C.c_float), ("pre_target", C.c_float),
                ("master_target", C.c_float), ("param_target", C.c_float * 2)]


class Controls(C.Structure):
    _fields_ = [(n, C.c_float) for n in CONTROL_FIELDS]


class StreamMeter(C.Structure):
    """aidax_stream_meter: one stream's record (64 bytes)"""
    _fields_ = [("frames", C.c_uint64), ("passes", C.c_uint64), ("in_nonfinite", C.c_uint64), ("out_nonfinite", C.c_uint64),
                ("out_over", C.c_uint64), ("in_energy", C.c_double), ("out_energy", C.c_double), ("in_peak", C.c_float),
                ("out_peak", C.c_float)]


METER_DTYPE = np.dtype([("frames", "<u8"), ("passes", "<u8"), ("in_nonfinite", "<u8"), ("out_nonfinite", "<u8"), ("out_over", "<u8"),
                        ("in_energy", "<f8"), ("out_energy", "<f8"), ("in_peak", "<f4"), ("out_peak", "<f4")])


class GateParams(C.Structure):
    """aidax_gate_params: a noise gate as a user sets it (levels in dB, times in ms)"""
    _fields_ = [("open_db", C.c_float), ("close_db", C.c_float), ("floor_db", C.c_float), ("attack_ms", C.c_float),
                ("hold_ms", C.c_float), ("release_ms", C.c_float)]


class GateRec(C.Structure):
    """aidax_gate_rec: the record k_gate reads (32 bytes), what aidax_gate_design makes of GateParams at a sample rate"""
    _fields_ = [("t_open", C.c_float), ("t_close", C.c_float), ("floor", C.c_float), ("span", C.c_float),
                ("hold", C.c_uint32), ("up", C.c_uint32), ("down", C.c_uint32), ("on", C.c_uint32)]


class GateState(C.Structure):
    """aidax_gate_state: a stream's gate state (hold frames left, attenuation position 0 .. 2^24)"""
    _fields_ = [("hold_left", C.c_uint32), ("atten", C.c_uint32)]


GATE_STATE_DTYPE = np.dtype([("hold_left", "<u4"), ("atten", "<u4")])


class TunerParams(C.Structure):
    """aidax_tuner_params: the stream tuners as a user sets them (window and hop in frames, the range in Hz)"""
    _fields_ = [("window", C.c_uint32), ("hop", C.c_uint32), ("f_min", C.c_float), ("f_max", C.c_float), ("threshold", C.c_float),
                ("clarity_min", C.c_float), ("level_min_db", C.c_float)]


class TunerRec(C.Structure):
    """aidax_tuner_rec: the designed record (40 bytes), what aidax_tuner_design makes of TunerParams at a sample rate"""
    _fields_ = [("window", C.c_uint32), ("hop", C.c_uint32), ("tmin", C.c_uint32), ("tmax", C.c_uint32), ("threshold", C.c_float),
                ("clarity_min", C.c_float), ("level_min", C.c_float), ("reserved", C.c_float), ("samplerate", C.c_double)]


class TunerReadingStruct(C.Structure):
    """aidax_tuner_reading: one stream's reading (32 bytes)"""
    _fields_ = [("frame", C.c_uint64), ("analyses", C.c_uint32), ("lag", C.c_uint32), ("hz", C.c_float), ("period", C.c_float),
                ("clarity", C.c_float), ("level", C.c_float)]


TunerReading = np.dtype([("frame", "<u8"), ("analyses", "<u4"), ("lag", "<u4"), ("hz", "<f4"), ("period", "<f4"), ("clarity", "<f4"),
                         ("level", "<f4")])


class BusLimitParams(C.Structure):
    """aidax_bus_limit_params: a bus limiter as a user sets it (the ceiling in dB, times in ms)"""
    _fields_ = [("ceiling_db", C.c_float), ("lookahead_ms", C.c_float), ("hold_ms", C.c_float)]


class BusLimitRec(C.Structure):
    """aidax_bus_limit_rec: the record k_bus_limit reads (16 bytes), what aidax_bus_limit_design makes of BusLimitParams at a sample rate"""
    _fields_ = [("ceiling", C.c_float), ("lookahead", C.c_uint32), ("hold", C.c_uint32), ("on", C.c_uint32)]


class BusMeter(C.Structure):
    """aidax_bus_meter: one bus's record (48 bytes)"""
    _fields_ = [("frames", C.c_uint64), ("passes", C.c_uint64), ("in_nonfinite", C.c_uint64), ("limited", C.c_uint64),
                ("in_peak", C.c_float), ("out_peak", C.c_float), ("min_gain", C.c_float), ("reserved", C.c_float)]


class BusReverbParams(C.Structure):
    """aidax_bus_reverb_params: a bus reverb as a user sets it (decay time in s, room size, damping, levels, one of four delay tables)"""
    _fields_ = [("rt60_s", C.c_float), ("size", C.c_float), ("damping", C.c_float), ("wet", C.c_float), ("dry", C.c_float), ("variant", C.c_uint32)]


class BusReverbRec(C.Structure):
    """aidax_bus_reverb_rec: the record k_bus_reverb reads (96 bytes), what aidax_bus_reverb_design makes of BusReverbParams at a sample rate"""
    _fields_ = [("m", C.c_uint32 * 8), ("gq", C.c_float * 8), ("a", C.c_float), ("wet", C.c_float), ("dry", C.c_float),
                ("on", C.c_uint32), ("epoch", C.c_uint32), ("reserved", C.c_uint32 * 3)]


BUS_METER_DTYPE = np.dtype([("frames", "<u8"), ("passes", "<u8"), ("in_nonfinite", "<u8"), ("limited", "<u8"),
                            ("in_peak", "<f4"), ("out_peak", "<f4"), ("min_gain", "<f4"), ("reserved", "<f4")])


class DelayParams(C.Structure):
    """aidax_delay_params: a stream delay as a user sets it (times in ms, the modulation rate in Hz)"""
    _fields_ = [("time_ms", C.c_float), ("feedback", C.c_float), ("damping", C.c_float), ("wet", C.c_float), ("dry", C.c_float),
                ("mod_rate_hz", C.c_float), ("mod_depth_ms", C.c_float), ("fade_ms", C.c_float)]


class DelayRec(C.Structure):
    """aidax_delay_rec: the record k_delay reads (48 bytes), what aidax_delay_design makes of DelayParams at a sample rate"""
    _fields_ = [("m", C.c_uint32), ("depth_q16", C.c_uint32), ("lfo_step", C.c_uint32), ("fade", C.c_uint32), ("fb", C.c_float),
                ("damp", C.c_float), ("wet", C.c_float), ("dry", C.c_float), ("on", C.c_uint32), ("reserved", C.c_uint32 * 3)]


class DelayStateStruct(C.Structure):
    """aidax_delay_state: one stream's delay state (32 bytes)"""
    _fields_ = [("pos", C.c_uint64), ("m_cur", C.c_uint32), ("m_old", C.c_uint32), ("fade_len", C.c_uint32), ("fade_left", C.c_uint32),
                ("phase", C.c_uint32), ("replaced", C.c_uint32)]


DelayState = np.dtype([("pos", "<u8"), ("m_cur", "<u4"), ("m_old", "<u4"), ("fade_len", "<u4"), ("fade_left", "<u4"), ("phase", "<u4"),
                       ("replaced", "<u4")])
DELAY_MIN, DELAY_MAX = 64, 1 << 18               # AIDAX_DELAY_MIN, AIDAX_DELAY_MAX: frames


def lib_path() -> str:
    # AIDAX_LIB: another build of the library (A/B measurements of two builds in one gpurun call)
    return os.environ.get("AIDAX_LIB") or os.path.join(_HERE, "lib", "libaidax_hip.so")


_lib: Optional[C.CDLL] = None


def lib() -> C.CDLL:
    """Load the HIP library. Fails loudly when it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    # Python processes that also use torch (bench.py, some tests) must end up with ONE HIP/HSA
    # runtime: torch ships its own copy, and a second runtime initialised later finds no GPU.
    # Importing torch first makes the loader resolve libamdhip64.so.7 to the copy torch loaded.
    # (AIDAX_NO_TORCH=1: processes that never touch torch, e.g. tests/rt_audit.py, skip that.)
    if not os.environ.get("AIDAX_NO_TORCH"):
        try:
            import torch  # noqa: F401
        except Exception:
            pass
    path = lib_path()
    if not os.path.exists(path):
        raise FileNotFoundError(f"{path} missing: run `make` (or __graft_entry__.build()); there is no CPU fallback")
    L = C.CDLL(path)
    vp, i32, u32 = C.c_void_p, C.c_int32, C.c_uint32
    L.aidax_last_error.restype = C.c_char_p
    L.aidax_version.restype = C.c_char_p
    L.aidax_model_load.argtypes = [C.c_char_p, C.POINTER(vp)]
    L.aidax_model_load_memory.argtypes = [C.c_char_p, C.c_size_t, C.c_char_p, C.POINTER(vp)]
    L.aidax_model_info.argtypes = [vp, C.POINTER(ModelInfo)]
    L.aidax_model_path.argtypes = [vp]
    L.aidax_model_path.restype = C.c_char_p
    L.aidax_model_golden.argtypes = [vp, _fp, _fp, u32]
    L.aidax_model_free.argtypes = [vp]
    L.aidax_model_free.restype = None
    L.aidax_controls_default.argtypes = [C.POINTER(Controls)]
    L.aidax_controls_default.restype = None
    L.aidax_biquad_design.argtypes = [C.c_int, C.c_double, C.c_double, C.c_double, C.POINTER(C.c_double)]
    L.aidax_db_to_coeff.argtypes = [C.c_float]
    L.aidax_db_to_coeff.restype = C.c_float
    L.aidax_lpf_fc.argtypes = [C.c_float]
    L.aidax_lpf_fc.restype = C.c_float
    L.aidax_device_count.argtypes = [C.POINTER(C.c_int)]
    L.aidax_pick_device.argtypes = [C.c_char_p, C.c_int, C.POINTER(u32), C.POINTER(C.c_int)]
    L.aidax_pick_hub.argtypes = [C.POINTER(C.c_int), C.POINTER(u32), C.c_int, C.c_int, C.c_char_p, C.c_int, C.POINTER(u32),
                                 C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.aidax_many_streams_form.argtypes = [C.c_int, C.c_int, u32, C.c_int]
    L.aidax_many_streams_form.restype = C.c_int
    L.aidax_many_streams_form_at.argtypes = [C.c_int, C.c_int, u32, C.c_int, u32]
    L.aidax_many_streams_form_at.restype = C.c_int
    L.aidax_model_conv_form.argtypes = [C.c_void_p]
    L.aidax_model_conv_form.restype = C.c_int
    L.aidax_pool_create.argtypes = [u32, u32, C.c_double, C.c_int, C.POINTER(vp)]
    L.aidax_pool_destroy.argtypes = [vp]
    L.aidax_pool_destroy.restype = None
    L.aidax_pool_streams.argtypes = [vp]
    L.aidax_pool_streams.restype = u32
    L.aidax_pool_set_model.argtypes = [vp, vp, C.c_int]
    L.aidax_pool_prepare_model.argtypes = [vp, vp, C.c_int, C.POINTER(vp)]
    L.aidax_pool_commit_model.argtypes = [vp, vp]
    L.aidax_staged_free.argtypes = [vp]
    if hasattr(L, "aidax_pool_assign_model"):      # (AIDAX_LIB may name a build from before the model bank: A/B runs against it)
        L.aidax_model_bank_compatible.argtypes = [vp, vp]
        L.aidax_pool_prepare_model_slot.argtypes = [vp, u32, vp, C.POINTER(vp)]
        L.aidax_pool_set_model_slot.argtypes = [vp, u32, vp]
        L.aidax_pool_assign_model.argtypes = [vp, i32, i32, C.c_int]
        L.aidax_pool_stream_model.argtypes = [vp, u32, C.POINTER(i32)]
    L.aidax_staged_free.restype = None
    L.aidax_pool_set_loading.argtypes = [vp, i32, C.c_int]
    L.aidax_pool_set_controls.argtypes = [vp, i32, C.POINTER(Controls)]
    L.aidax_pool_activate.argtypes = [vp, i32]
    L.aidax_pool_process.argtypes = [vp, _fp, _fp, u32]
    L.aidax_pool_submit.argtypes = [vp, _fp, u32]
    L.aidax_pool_collect.argtypes = [vp, _fp, u32]
    L.aidax_pool_submit_to.argtypes = [vp, _fp, _fp, u32]
    L.aidax_pool_register_host.argtypes = [vp, C.c_void_p, C.c_size_t]
    L.aidax_pool_unregister_host.argtypes = [vp, C.c_void_p]
    L.aidax_pool_process_device.argtypes = [vp, vp, vp, u32, vp]
    L.aidax_pool_sync.argtypes = [vp]
    L.aidax_model_self_test.argtypes = [vp, C.c_int, C.POINTER(i32), _fp, _fp]
    L.aidax_model_forward.argtypes = [vp, C.c_int, _fp, _fp, u32, C.c_int]
    L.aidax_pool_read_state.argtypes = [vp, u32, C.c_int, _fp, _fp, u32]
    L.aidax_pool_kernel_name.argtypes = [vp]
    L.aidax_pool_kernel_name.restype = C.c_char_p
    L.aidax_pool_reset_stream.argtypes = [vp, u32, C.c_int]
    L.aidax_hub_create.argtypes = [u32, u32, C.c_double, C.c_int, C.POINTER(vp)]
    L.aidax_hub_destroy.argtypes = [vp]
    L.aidax_hub_destroy.restype = None
    L.aidax_hub_set_model.argtypes = [vp, vp, C.c_int]
    L.aidax_hub_attach.argtypes = [vp, C.POINTER(i32)]
    L.aidax_hub_detach.argtypes = [vp, i32]
    L.aidax_hub_set_controls.argtypes = [vp, i32, C.POINTER(Controls)]
    L.aidax_hub_run.argtypes = [vp, i32, _fp, _fp, u32]
    L.aidax_hub_set_loading.argtypes = [vp, i32, C.c_int]
    L.aidax_hub_activate.argtypes = [vp, i32]
    L.aidax_hub_latency_frames.argtypes = [vp]
    L.aidax_hub_latency_frames.restype = u32
    L.aidax_hub_attached.argtypes = [vp]
    L.aidax_hub_attached.restype = u32
    L.aidax_hub_max_frames.argtypes = [vp]
    L.aidax_hub_max_frames.restype = u32
    L.aidax_hub_attach_successor.argtypes = [vp, vp, C.c_int32, C.POINTER(C.c_int32)]
    L.aidax_hub_adopt.argtypes = [vp, C.c_int32, vp, C.c_int32]
    L.aidax_pool_export_stream_dsp.argtypes = [vp, u32, C.POINTER(StreamDsp)]
    L.aidax_pool_import_stream_dsp.argtypes = [vp, u32, C.POINTER(StreamDsp)]
    L.aidax_hub_launches.argtypes = [vp]
    L.aidax_hub_launches.restype = C.c_uint64
    L.aidax_hub_deadline_launches.argtypes = [vp]
    L.aidax_hub_deadline_launches.restype = C.c_uint64
    L.aidax_hub_faults_unmapped.argtypes = [vp]
    L.aidax_hub_faults_unmapped.restype = C.c_uint64
    L.aidax_hub_set_deadline_us.argtypes = [vp, C.c_int64]
    L.aidax_hub_flush.argtypes = [vp]
    L.aidax_ir_load_wav.argtypes = [C.c_char_p, _fp, u32, C.POINTER(u32), C.POINTER(C.c_double)]
    L.aidax_pool_prepare_ir.argtypes = [vp, _fp, u32, C.c_double, C.POINTER(vp)]
    L.aidax_pool_commit_ir.argtypes = [vp, vp]
    L.aidax_pool_set_ir.argtypes = [vp, _fp, u32, C.c_double]
    L.aidax_pool_prepare_ir_slot.argtypes = [vp, u32, _fp, u32, C.c_double, C.POINTER(vp)]
    L.aidax_pool_set_ir_slot.argtypes = [vp, u32, _fp, u32, C.c_double]
    L.aidax_pool_assign_ir.argtypes = [vp, i32, i32]
    L.aidax_pool_stream_ir.argtypes = [vp, u32, C.POINTER(i32)]
    L.aidax_pool_set_ir_fade.argtypes = [vp, u32]
    L.aidax_pool_ir_fade.argtypes = [vp]
    L.aidax_pool_ir_fade.restype = u32
    L.aidax_ir_resample.argtypes = [_fp, u32, C.c_double, C.c_double, u32, _fp, u32, C.POINTER(u32)]
    L.aidax_pool_set_ir_capacity.argtypes = [vp, u32]
    L.aidax_pool_ir_capacity.argtypes = [vp]
    L.aidax_pool_ir_capacity.restype = u32
    L.aidax_resampler_create.argtypes = [u32, C.c_double, C.c_double, u32, u32, u32, C.c_int, C.POINTER(vp)]
    L.aidax_resampler_destroy.argtypes = [vp]
    L.aidax_resampler_destroy.restype = None
    L.aidax_resampler_row.argtypes = [C.c_double, C.c_double, u32, _fp, u32, C.POINTER(u32)]
    L.aidax_resampler_process_device.argtypes = [vp, vp, u32, vp, u32, vp]
    L.aidax_resampler_process.argtypes = [vp, _fp, u32, _fp, u32]
    L.aidax_resampler_ready.argtypes = [vp]
    L.aidax_resampler_ready.restype = u32
    L.aidax_resampler_reset_stream.argtypes = [vp, u32]
    L.aidax_pool_samplerate.argtypes = [vp]
    L.aidax_pool_samplerate.restype = C.c_double
    L.aidax_rate_create.argtypes = [vp, C.c_double, u32, C.POINTER(vp)]
    L.aidax_rate_destroy.argtypes = [vp]
    L.aidax_rate_destroy.restype = None
    L.aidax_rate_latency_frames.argtypes = [vp]
    L.aidax_rate_latency_frames.restype = u32
    L.aidax_rate_latency.argtypes = [C.c_double, C.c_double, C.POINTER(u32)]
    L.aidax_rate_process.argtypes = [vp, _fp, _fp, u32]
    L.aidax_rate_process_device.argtypes = [vp, vp, vp, u32, vp]
    L.aidax_rate_reset_stream.argtypes = [vp, u32]
    if hasattr(L, "aidax_pool_set_ir_mix"):        # (... or from before the IR blend)
        L.aidax_pool_assign_ir_b.argtypes = [vp, i32, i32]
        L.aidax_pool_set_ir_mix.argtypes = [vp, i32, C.c_float, u32]
        L.aidax_pool_stream_ir_mix.argtypes = [vp, u32, C.POINTER(i32), _fp, _fp, C.POINTER(u32)]
    if hasattr(L, "aidax_pool_read_meters"):       # (AIDAX_LIB may name a build from before the stream meters: A/B runs against it)
        L.aidax_pool_set_metering.argtypes = [vp, C.c_int]
        L.aidax_pool_metering.argtypes = [vp]
        L.aidax_pool_read_meters.argtypes = [vp, u32, u32, C.POINTER(StreamMeter), C.c_int]
    if hasattr(L, "aidax_pool_set_gate"):          # (... or from before the noise gate)
        L.aidax_gate_design.argtypes = [C.POINTER(GateParams), C.c_double, C.POINTER(GateRec)]
        L.aidax_pool_set_gate.argtypes = [vp, i32, C.POINTER(GateParams)]
        L.aidax_pool_stream_gate.argtypes = [vp, u32, C.POINTER(GateParams), C.POINTER(C.c_int)]
        L.aidax_pool_read_gate.argtypes = [vp, u32, u32, C.POINTER(GateState)]
    if hasattr(L, "aidax_pool_set_tuning"):        # (... or from before the stream tuners)
        L.aidax_tuner_params_default.argtypes = [C.POINTER(TunerParams)]
        L.aidax_tuner_params_default.restype = None
        L.aidax_tuner_design.argtypes = [C.c_double, C.POINTER(TunerParams), C.POINTER(TunerRec)]
        L.aidax_tuner_note.argtypes = [C.c_double, C.c_double, C.POINTER(i32), _fp]
        L.aidax_pool_set_tuning.argtypes = [vp, C.POINTER(TunerParams)]
        L.aidax_pool_tuning.argtypes = [vp, C.POINTER(TunerRec)]
        L.aidax_pool_set_tuner.argtypes = [vp, i32, C.c_int]
        L.aidax_pool_stream_tuner.argtypes = [vp, u32, C.POINTER(C.c_int), C.POINTER(C.c_uint64)]
        L.aidax_pool_read_tuners.argtypes = [vp, u32, u32, C.POINTER(TunerReadingStruct)]
        L.aidax_pool_read_tuner_curve.argtypes = [vp, u32, _fp, u32]
    if hasattr(L, "aidax_pool_set_buses"):         # (... or from before the mix buses)
        L.aidax_pool_set_buses.argtypes = [vp, u32]
        L.aidax_pool_buses.argtypes = [vp]
        L.aidax_pool_buses.restype = u32
        L.aidax_pool_set_send.argtypes = [vp, i32, u32, i32, C.c_float, u32]
        L.aidax_pool_stream_send.argtypes = [vp, u32, u32, C.POINTER(i32), _fp, _fp, C.POINTER(u32)]
        L.aidax_mix_gain.argtypes = [C.c_float, C.c_float, u32, u32, _fp]
        L.aidax_pool_read_buses.argtypes = [vp, u32, u32, _fp, C.c_size_t, C.POINTER(u32)]
        L.aidax_pool_buses_device.argtypes = [vp, C.POINTER(vp)]
        L.aidax_pool_process_buses.argtypes = [vp, _fp, _fp, u32]
    if hasattr(L, "aidax_pool_set_bus_limiting"):  # (... or from before the bus limiters)
        L.aidax_bus_limit_design.argtypes = [C.POINTER(BusLimitParams), C.c_double, C.POINTER(BusLimitRec)]
        L.aidax_pool_set_bus_limiting.argtypes = [vp, C.c_int, u32, u32]
        L.aidax_pool_bus_limiting.argtypes = [vp]
        L.aidax_pool_set_bus_limiter.argtypes = [vp, i32, C.POINTER(BusLimitParams)]
        L.aidax_pool_bus_limiter.argtypes = [vp, u32, C.POINTER(BusLimitParams), C.POINTER(C.c_int), C.POINTER(u32)]
        L.aidax_pool_read_bus_meters.argtypes = [vp, u32, u32, C.POINTER(BusMeter), C.c_int]
    if hasattr(L, "aidax_pool_set_bus_reverbs"):  # (... or from before the bus reverbs)
        L.aidax_bus_reverb_design.argtypes = [C.POINTER(BusReverbParams), C.c_double, C.POINTER(BusReverbRec)]
        L.aidax_pool_set_bus_reverbs.argtypes = [vp, C.c_int, u32]
        L.aidax_pool_bus_reverbs.argtypes = [vp]
        L.aidax_pool_set_bus_reverb.argtypes = [vp, i32, C.POINTER(BusReverbParams)]
        L.aidax_pool_set_bus_reverb_rec.argtypes = [vp, i32, C.POINTER(BusReverbRec)]
        L.aidax_pool_bus_reverb.argtypes = [vp, u32, C.POINTER(BusReverbParams), C.POINTER(BusReverbRec), C.POINTER(C.c_int), C.POINTER(C.c_uint64)]
        L.aidax_pool_reset_bus_reverb.argtypes = [vp, i32]
    if hasattr(L, "aidax_pool_set_delays"):       # (... or from before the stream delays)
        L.aidax_delay_design.argtypes = [C.POINTER(DelayParams), C.c_double, C.POINTER(DelayRec)]
        L.aidax_pool_set_delays.argtypes = [vp, C.c_int, u32]
        L.aidax_pool_delays.argtypes = [vp]
        L.aidax_pool_set_delay.argtypes = [vp, i32, C.POINTER(DelayParams)]
        L.aidax_pool_set_delay_rec.argtypes = [vp, i32, C.POINTER(DelayRec)]
        L.aidax_pool_stream_delay.argtypes = [vp, u32, C.POINTER(DelayParams), C.POINTER(DelayRec), C.POINTER(C.c_int)]
        L.aidax_pool_read_delays.argtypes = [vp, u32, u32, C.POINTER(DelayStateStruct)]
        L.aidax_pool_reset_delay.argtypes = [vp, i32]
    _lib = L
    return L


def declared_symbols() -> list:
    """Every AIDAX_API function name declared in include/aidax.h."""
    with open(_HEADER) as f:
        text = f.read()
    return sorted(set(re.findall(r"AIDAX_API[^;(]*?\b(aidax_[a-z_0-9]+)\s*\(", text)))


def _check(rc: int):
    if rc < 0:
        raise AidaxError(rc, lib().aidax_last_error().decode(errors="replace"))
    return rc


def _f32(a) -> np.ndarray:
    return np.ascontiguousarray(np.asarray(a, dtype=np.float32))


def default_controls(**kw) -> Controls:
    c = Controls()
    lib().aidax_controls_default(C.byref(c))
    for k, v in kw.items():
        if k not in CONTROL_FIELDS:
            raise KeyError(k)
        setattr(c, k, v)
    return c


def biquad_design(kind: int, fc: float, q: float, gain_db: float) -> np.ndarray:
    out = (C.c_double * 5)()
    _check(lib().aidax_biquad_design(kind, fc, q, gain_db, out))
    return np.array(list(out), np.float64)


def gate_design(params: GateParams, samplerate: float) -> GateRec:
    """aidax_gate_design: the record of `params` at `samplerate` (pure, host only)"""
    out = GateRec()
    _check(lib().aidax_gate_design(C.byref(params) if params is not None else None, samplerate, C.byref(out)))
    return out


def tuner_params(**kw) -> TunerParams:
    """aidax_tuner_params_default, with the named fields replaced"""
    p = TunerParams()
    lib().aidax_tuner_params_default(C.byref(p))
    for k, v in kw.items():
        if k not in dict(TunerParams._fields_):
            raise KeyError(k)
        setattr(p, k, v)
    return p


def tuner_design(samplerate: float, params: TunerParams) -> TunerRec:
    """aidax_tuner_design: the record of `params` at `samplerate` (pure, host only)"""
    out = TunerRec()
    _check(lib().aidax_tuner_design(samplerate, C.byref(params) if params is not None else None, C.byref(out)))
    return out


def tuner_note(hz: float, a4_hz: float = 440.0):
    """aidax_tuner_note: (the nearest equal-tempered MIDI note, the deviation in cents)"""
    note, cents = C.c_int32(0), C.c_float(0.0)
    _check(lib().aidax_tuner_note(hz, a4_hz, C.byref(note), C.byref(cents)))
    return note.value, cents.value


def bus_reverb_design(params: BusReverbParams, samplerate: float) -> BusReverbRec:
    """aidax_bus_reverb_design: the record of `params` at `samplerate` (pure, host only)"""
    out = BusReverbRec()
    _check(lib().aidax_bus_reverb_design(C.byref(params) if params is not None else None, samplerate, C.byref(out)))
    return out


def delay_design(params: DelayParams, samplerate: float) -> DelayRec:
    """aidax_delay_design: the record of `params` at `samplerate` (pure, host only)"""
    out = DelayRec()
    _check(lib().aidax_delay_design(C.byref(params) if params is not None else None, samplerate, C.byref(out)))
    return out


def bus_limit_design(params: BusLimitParams, samplerate: float) -> BusLimitRec:
    """aidax_bus_limit_design: the record of `params` at `samplerate` (pure, host only)"""
    out = BusLimitRec()
    _check(lib().aidax_bus_limit_design(C.byref(params) if params is not None else None, samplerate, C.byref(out)))
    return out


def mix_gain(g0: float, g1: float, ramp_frames: int, k: int) -> float:
    """aidax_mix_gain: the gain of frame k of a send's ramp g0 -> g1 over ramp_frames frames (pure, host only)"""
    out = C.c_float(0)
    _check(lib().aidax_mix_gain(g0, g1, ramp_frames, k, C.byref(out)))
    return out.value


def load_ir_wav(path: str):
    """aidax_ir_load_wav: (taps as float32, samplerate) of channel 0 of a WAV file."""
    n, sr = C.c_uint32(0), C.c_double(0.0)
    _check(lib().aidax_ir_load_wav(os.fsencode(path), None, 0, C.byref(n), C.byref(sr)))
    taps = np.empty(n.value, np.float32)
    _check(lib().aidax_ir_load_wav(os.fsencode(path), taps.ctypes.data_as(_fp), n.value, C.byref(n), C.byref(sr)))
    return taps, sr.value


def resample_ir(taps, rate_in: float, rate_out: float, lead: int = 0, cap: Optional[int] = None):
    """aidax_ir_resample: (taps at rate_out as float32, n_full). `lead` frames of the pre-ringing are kept (the caller's latency);
    cap cuts the result (no tail fade), None keeps all n_full frames."""
    t = _f32(taps).reshape(-1)
    n = C.c_uint32(0)
    _check(lib().aidax_ir_resample(t.ctypes.data_as(_fp), t.size, rate_in, rate_out, lead, None, 0, C.byref(n)))
    out = np.empty(n.value if cap is None else min(int(cap), n.value), np.float32)
    if out.size:
        _check(lib().aidax_ir_resample(t.ctypes.data_as(_fp), t.size, rate_in, rate_out, lead, out.ctypes.data_as(_fp), out.size, C.byref(n)))
    return out, n.value


def load_ir_wav_for(pool: "Pool", path: str, lead: int = 0) -> np.ndarray:
    """A WAV file's IR ready for `pool`: read (aidax_ir_load_wav), converted to the pool's host rate (aidax_ir_resample; a file at that
    rate is taken as it is, behind `lead` zeros) and cut to the pool's IR capacity."""
    taps, sr = load_ir_wav(path)
    return resample_ir(taps, sr, pool.samplerate, lead, pool.ir_capacity())[0]


def resampler_row(rate_in: float, rate_out: float, phase: int) -> np.ndarray:
    """aidax_resampler_row: the T weights of row `phase` of the streaming resampler's filter (host only)"""
    n = C.c_uint32(0)
    _check(lib().aidax_resampler_row(rate_in, rate_out, phase, None, 0, C.byref(n)))
    w = np.empty(n.value, np.float32)
    _check(lib().aidax_resampler_row(rate_in, rate_out, phase, w.ctypes.data_as(_fp), n.value, C.byref(n)))
    return w


def rate_latency(host_rate: float, pool_rate: float) -> int:
    """aidax_rate_latency: host frames of delay of a rate adapter between these rates (host only)"""
    n = C.c_uint32(0)
    _check(lib().aidax_rate_latency(host_rate, pool_rate, C.byref(n)))
    return n.value


def device_count() -> int:
    n = C.c_int(0)
    _check(lib().aidax_device_count(C.byref(n)))
    return n.value


def pick_device(spec: Optional[str], count: int, load=None) -> int:
    """The placement rule (pure): least-loaded device among those `spec` names ("auto", "0-3,6", None = device 0)."""
    arr = None
    if load is not None:
        arr = (C.c_uint32 * len(load))(*load)
    out = C.c_int(-1)
    _check(lib().aidax_pick_device(spec.encode() if spec is not None else None, count, arr, C.byref(out)))
    return out.value


def pick_hub(hub_devices, hub_free_seats, current_device: int, spec: Optional[str], count: int, load=None):
    """-> (index of the hub to join or -1 = open a new one, device)"""
    n = len(hub_devices)
    dev = (C.c_int * max(n, 1))(*hub_devices)
    free = (C.c_uint32 * max(n, 1))(*hub_free_seats)
    arr = (C.c_uint32 * count)(*load) if load is not None else None
    idx, out = C.c_int(-2), C.c_int(-1)
    _check(lib().aidax_pick_hub(dev, free, n, current_device, spec.encode() if spec is not None else None, count, arr,
                                C.byref(idx), C.byref(out)))
    return idx.value, out.value


def many_streams_form(cell: int, hidden: int, n_streams: int, compute_units: int = 256, max_frames: int = 256) -> int:
    """aidax_many_streams_form_at: 0 per-stream forms, 1 k_quad, 2 the 16-stream matrix-core kernels"""
    return int(lib().aidax_many_streams_form_at(cell, hidden, n_streams, compute_units, max_frames))


def bank_compatible(pool_model: "Model", m: "Model") -> bool:
    """aidax_model_bank_compatible (host only): may `m` sit in a bank slot of a pool whose pool model is `pool_model`? The reason of a
    refusal is in last_error()."""
    rc = lib().aidax_model_bank_compatible(pool_model.h, m.h)
    if rc == 0:
        return True
    if rc == -4:                  # AIDAX_ERR_ARCH: the answer "no"
        return False
    _check(rc)
    return False


def last_error() -> str:
    return lib().aidax_last_error().decode(errors="replace")


def db_to_coeff(db: float) -> float:
    return float(lib().aidax_db_to_coeff(C.c_float(db)))


def lpf_fc(pc: float) -> float:
    return float(lib().aidax_lpf_fc(C.c_float(pc)))


class Model:
    """aidax_model: the json-side half of the reference's DynamicModel."""

    def __init__(self, path: Optional[str] = None, text: Optional[str] = None, label: str = "<memory>"):
        h = C.c_void_p()
        if path is not None:
            _check(lib().aidax_model_load(path.encode(), C.byref(h)))
        else:
            b = text.encode()
            _check(lib().aidax_model_load_memory(b, len(b), label.encode(), C.byref(h)))
        self.h = h

    @property
    def info(self) -> ModelInfo:
        i = ModelInfo()
        _check(lib().aidax_model_info(self.h, C.byref(i)))
        return i

    @property
    def path(self) -> str:
        return lib().aidax_model_path(self.h).decode()

    @property
    def conv_form(self) -> int:
        """aidax_model_conv_form: 0 not a conv stack, 1 k_conv, 2 k_conv_mfma, 3 k_conv_ms, 4 k_conv_ms + k_conv_st for full blocks"""
        return int(lib().aidax_model_conv_form(self.h))

    def golden(self):
        n = self.info.n_golden
        a, b = np.zeros(n, np.float32), np.zeros(n, np.float32)
        lib().aidax_model_golden(self.h, a.ctypes.data_as(_fp), b.ctypes.data_as(_fp), n)
        return a, b

    def self_test(self, device: int = 0):
        n_err, max_err = C.c_int32(0), C.c_float(0)
        out = np.zeros(self.info.n_golden, np.float32)
        _check(lib().aidax_model_self_test(self.h, device, C.byref(n_err), C.byref(max_err), out.ctypes.data_as(_fp)))
        return int(n_err.value), float(max_err.value), out

    def forward(self, X, device: int = 0, unit_gains: bool = False) -> np.ndarray:
        X = _f32(X).reshape(-1, self.info.input_size)
        y = np.zeros(X.shape[0], np.float32)
        _check(lib().aidax_model_forward(self.h, device, X.ctypes.data_as(_fp), y.ctypes.data_as(_fp),
                                         X.shape[0], 1 if unit_gains else 0))
        return y

    def close(self):
        if self.h:
            lib().aidax_model_free(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# the pools and hubs that are open (test harnesses close what a failed test left behind: a pool that holds a device's right to
# the chained kernels would otherwise change the kernel every later pool of the process gets)
live_handles = weakref.WeakSet()


class Pool:
    """aidax_pool: N plugin instances' DSP state on one GPU."""

    def __init__(self, n_streams: int, max_frames: int = 256, samplerate: float = 48000.0, device: int = 0):
        h = C.c_void_p()
        _check(lib().aidax_pool_create(n_streams, max_frames, samplerate, device, C.byref(h)))
        self.h = h
        live_handles.add(self)
        self.n_streams = n_streams
        self.max_frames = max_frames
        self.samplerate = samplerate

    def set_model(self, m: Optional[Model], start_mode: int = START_WARMUP):
        _check(lib().aidax_pool_set_model(self.h, m.h if m is not None else None, start_mode))

    def prepare_model(self, m: Optional[Model], start_mode: int = START_WARMUP) -> C.c_void_p:
        """worker half of a model swap: returns the staged handle for commit_model / staged_free"""
        sg = C.c_void_p()
        _check(lib().aidax_pool_prepare_model(self.h, m.h if m is not None else None, start_mode, C.byref(sg)))
        return sg

    def commit_model(self, staged: C.c_void_p):
        """audio half: swaps the staged model in; `staged` then holds what was retired (free it with staged_free)"""
        _check(lib().aidax_pool_commit_model(self.h, staged))

    @staticmethod
    def staged_free(staged: C.c_void_p):
        lib().aidax_staged_free(staged)

    def prepare_model_slot(self, slot: int, m: Optional[Model]) -> C.c_void_p:
        """worker half of a model-bank slot's swap (m None: empty it): returns the staged handle for commit_model / staged_free"""
        sg = C.c_void_p()
        _check(lib().aidax_pool_prepare_model_slot(self.h, slot, m.h if m is not None else None, C.byref(sg)))
        return sg

    def set_model_slot(self, slot: int, m: Optional[Model]):
        """aidax_pool_set_model_slot: load model-bank slot `slot` with a weight variant of the pool model's architecture (m None: empty it)"""
        _check(lib().aidax_pool_set_model_slot(self.h, slot, m.h if m is not None else None))

    def assign_model(self, stream: int, slot: int, start_mode: int = START_WARMUP):
        """aidax_pool_assign_model: `stream` plays `slot` (MODEL_POOL or a bank slot) from the next pass on, as a fresh DynamicModel"""
        _check(lib().aidax_pool_assign_model(self.h, stream, slot, start_mode))

    def stream_model(self, stream: int) -> int:
        v = C.c_int32(0)
        _check(lib().aidax_pool_stream_model(self.h, stream, C.byref(v)))
        return v.value

    def set_ir(self, taps: Optional[np.ndarray], samplerate: Optional[float] = None):
        """aidax_pool_set_ir: attach a cabinet IR (taps None: remove it); samplerate defaults to the pool's"""
        t = None if taps is None else _f32(taps)
        _check(lib().aidax_pool_set_ir(self.h, None if t is None else t.ctypes.data_as(_fp), 0 if t is None else t.size,
                                       self.samplerate if samplerate is None else samplerate))

    def prepare_ir(self, taps: Optional[np.ndarray], samplerate: Optional[float] = None) -> C.c_void_p:
        """worker half of an IR swap: returns the staged handle for commit_ir / staged_free"""
        t = None if taps is None else _f32(taps)
        sg = C.c_void_p()
        _check(lib().aidax_pool_prepare_ir(self.h, None if t is None else t.ctypes.data_as(_fp), 0 if t is None else t.size,
                                           self.samplerate if samplerate is None else samplerate, C.byref(sg)))
        return sg

    def commit_ir(self, staged: C.c_void_p):
        """audio half: swaps the staged IR in; `staged` then holds the retired one (free it with staged_free)"""
        _check(lib().aidax_pool_commit_ir(self.h, staged))

    def set_ir_slot(self, slot: int, taps: Optional[np.ndarray], samplerate: Optional[float] = None):
        """aidax_pool_set_ir_slot: load bank slot `slot` (taps None: empty it); samplerate defaults to the pool's"""
        t = None if taps is None else _f32(taps)
        _check(lib().aidax_pool_set_ir_slot(self.h, slot, None if t is None else t.ctypes.data_as(_fp), 0 if t is None else t.size,
                                            self.samplerate if samplerate is None else samplerate))

    def prepare_ir_slot(self, slot: int, taps: Optional[np.ndarray], samplerate: Optional[float] = None) -> C.c_void_p:
        """worker half of a bank slot's swap: returns the staged handle for commit_ir / staged_free"""
        t = None if taps is None else _f32(taps)
        sg = C.c_void_p()
        _check(lib().aidax_pool_prepare_ir_slot(self.h, slot, None if t is None else t.ctypes.data_as(_fp), 0 if t is None else t.size,
                                                self.samplerate if samplerate is None else samplerate, C.byref(sg)))
        return sg

    def assign_ir(self, stream: int, slot: int):
        """aidax_pool_assign_ir: the IR `stream` (ALL_STREAMS: every stream) goes through from the next pass on (IR_POOL, IR_NONE or a
        bank slot)"""
        _check(lib().aidax_pool_assign_ir(self.h, stream, slot))

    def stream_ir(self, stream: int) -> int:
        v = C.c_int32(0)
        _check(lib().aidax_pool_stream_ir(self.h, stream, C.byref(v)))
        return v.value

    def assign_ir_b(self, stream: int, slot: int):
        """aidax_pool_assign_ir_b: the second IR of `stream` (ALL_STREAMS: every stream), the one its mix blends in (IR_POOL, IR_NONE, the
        default, or a bank slot)"""
        _check(lib().aidax_pool_assign_ir_b(self.h, stream, slot))

    def set_ir_mix(self, stream: int, mix: float, ramp_frames: int = 0):
        """aidax_pool_set_ir_mix: the weight of the second IR moves to `mix` (0 .. 1) over the stream's next `ramp_frames` frames (0: a jump
        at the block boundary)"""
        _check(lib().aidax_pool_set_ir_mix(self.h, stream, mix, ramp_frames))

    def stream_ir_mix(self, stream: int):
        """aidax_pool_stream_ir_mix: (slot_b, mix_now, mix_target, frames_left) behind the last pass issued"""
        b, now, target, left = C.c_int32(0), C.c_float(0), C.c_float(0), C.c_uint32(0)
        _check(lib().aidax_pool_stream_ir_mix(self.h, stream, C.byref(b), C.byref(now), C.byref(target), C.byref(left)))
        return b.value, now.value, target.value, left.value

    def set_ir_fade(self, frames: int):
        """aidax_pool_set_ir_fade: crossfade old and new IR over the first min(frames, n_frames) frames of the pass behind an IR change
        (0: off, the default)"""
        _check(lib().aidax_pool_set_ir_fade(self.h, frames))

    def ir_fade(self) -> int:
        return int(lib().aidax_pool_ir_fade(self.h))

    def set_ir_capacity(self, max_taps: int):
        """aidax_pool_set_ir_capacity: the longest IR the pool takes (8192 .. 65536 taps), before its first prepare_ir / set_ir of any kind"""
        _check(lib().aidax_pool_set_ir_capacity(self.h, max_taps))

    def ir_capacity(self) -> int:
        return int(lib().aidax_pool_ir_capacity(self.h))

    def set_metering(self, on: bool):
        """aidax_pool_set_metering: the per-stream meters on or off (the first enabling call allocates: a set-up side call)"""
        _check(lib().aidax_pool_set_metering(self.h, 1 if on else 0))

    @property
    def metering(self) -> bool:
        return bool(lib().aidax_pool_metering(self.h))

    def read_meters(self, first: int = 0, count: Optional[int] = None, clear: bool = False) -> np.ndarray:
        """aidax_pool_read_meters: the records of `count` streams from `first` (default: all from `first` on) as a structured array with
        aidax_stream_meter's field names, behind every pass issued so far; clear zeroes exactly those records behind the copy"""
        if count is None:
            count = self.n_streams - first
        out = np.zeros(max(count, 0), METER_DTYPE)
        _check(lib().aidax_pool_read_meters(self.h, first, count, out.ctypes.data_as(C.POINTER(StreamMeter)), 1 if clear else 0))
        return out

    def set_tuning(self, params: Optional[TunerParams]):
        """aidax_pool_set_tuning: the tuner stage with this design (the first enabling call allocates and fixes the design: a set-up
        side call), None: off"""
        _check(lib().aidax_pool_set_tuning(self.h, C.byref(params) if params is not None else None))

    def tuning(self):
        """aidax_pool_tuning: (the design as a TunerRec, whether the stage is on)"""
        out = TunerRec()
        on = lib().aidax_pool_tuning(self.h, C.byref(out))
        return out, bool(on)

    def set_tuner(self, on: bool, stream: int = ALL_STREAMS):
        """aidax_pool_set_tuner: the stream's (default: every stream's) tuner on or off; off -> on restarts it"""
        _check(lib().aidax_pool_set_tuner(self.h, stream, 1 if on else 0))

    def stream_tuner(self, stream: int):
        """aidax_pool_stream_tuner: (whether the stream's tuner is on, its frame count as the host mirrors it)"""
        on, pos = C.c_int(0), C.c_uint64(0)
        _check(lib().aidax_pool_stream_tuner(self.h, stream, C.byref(on), C.byref(pos)))
        return bool(on.value), pos.value

    def read_tuners(self, first: int = 0, count: Optional[int] = None) -> np.ndarray:
        """aidax_pool_read_tuners: the readings of `count` streams from `first` (default: all from `first` on) as a structured array with
        aidax_tuner_reading's field names, behind every pass issued so far"""
        if count is None:
            count = self.n_streams - first
        out = np.zeros(max(count, 0), TunerReading)
        _check(lib().aidax_pool_read_tuners(self.h, first, count, out.ctypes.data_as(C.POINTER(TunerReadingStruct))))
        return out

    def read_tuner_curve(self, stream: int, count: Optional[int] = None) -> np.ndarray:
        """aidax_pool_read_tuner_curve: the NSDF row of the stream's last analysis, lags 0 .. count - 1 (default: all tmax + 2)"""
        if count is None:
            count = self.tuning()[0].tmax + 2
        out = np.zeros(max(count, 0), np.float32)
        _check(lib().aidax_pool_read_tuner_curve(self.h, stream, out.ctypes.data_as(_fp), count))
        return out

    def set_gate(self, params: Optional[GateParams], stream: int = ALL_STREAMS):
        """aidax_pool_set_gate: the stream's (default: every stream's) noise gate ahead of the model, None: off (the first enabling call
        allocates: a set-up side call)"""
        _check(lib().aidax_pool_set_gate(self.h, stream, C.byref(params) if params is not None else None))

    def stream_gate(self, stream: int):
        """aidax_pool_stream_gate: (the stream's GateParams as last set, whether its gate is on)"""
        out, on = GateParams(), C.c_int(0)
        _check(lib().aidax_pool_stream_gate(self.h, stream, C.byref(out), C.byref(on)))
        return out, bool(on.value)

    def read_gate(self, first: int = 0, count: Optional[int] = None) -> np.ndarray:
        """aidax_pool_read_gate: the gate states of `count` streams from `first` (default: all from `first` on) as a structured array with
        aidax_gate_state's field names, behind every pass issued so far"""
        if count is None:
            count = self.n_streams - first
        out = np.zeros(max(count, 0), GATE_STATE_DTYPE)
        _check(lib().aidax_pool_read_gate(self.h, first, count, out.ctypes.data_as(C.POINTER(GateState))))
        return out

    def set_delays(self, on: bool, max_delay_frames: int = 48000):
        """aidax_pool_set_delays: the stream delays behind the IR stage on or off (the first enabling call allocates and fixes the
        capacity: a set-up side call; off -> on restarts every line)"""
        _check(lib().aidax_pool_set_delays(self.h, 1 if on else 0, max_delay_frames))

    @property
    def delays(self) -> bool:
        return bool(lib().aidax_pool_delays(self.h))

    def set_delay(self, params: Optional[DelayParams], stream: int = ALL_STREAMS):
        """aidax_pool_set_delay: the stream's (default: every stream's) delay from the next pass on, None: off"""
        _check(lib().aidax_pool_set_delay(self.h, stream, C.byref(params) if params is not None else None))

    def set_delay_rec(self, rec: Optional[DelayRec], stream: int = ALL_STREAMS):
        """aidax_pool_set_delay_rec: the same with a record of the caller's own, None: off"""
        _check(lib().aidax_pool_set_delay_rec(self.h, stream, C.byref(rec) if rec is not None else None))

    def stream_delay(self, stream: int):
        """aidax_pool_stream_delay: (the stream's DelayParams as last set, its DelayRec, whether its delay is on)"""
        out, rec, on = DelayParams(), DelayRec(), C.c_int(0)
        _check(lib().aidax_pool_stream_delay(self.h, stream, C.byref(out), C.byref(rec), C.byref(on)))
        return out, rec, bool(on.value)

    def read_delays(self, first: int = 0, count: Optional[int] = None) -> np.ndarray:
        """aidax_pool_read_delays: the delay states of `count` streams from `first` (default: all from `first` on) as a structured array
        with aidax_delay_state's field names, behind every pass issued so far"""
        if count is None:
            count = self.n_streams - first
        out = np.zeros(max(count, 0), DelayState)
        _check(lib().aidax_pool_read_delays(self.h, first, count, out.ctypes.data_as(C.POINTER(DelayStateStruct))))
        return out

    def reset_delay(self, stream: int = ALL_STREAMS):
        """aidax_pool_reset_delay: the stream's (default: every stream's) line restarts at the next pass's first frame"""
        _check(lib().aidax_pool_reset_delay(self.h, stream))

    def set_buses(self, n_buses: int):
        """aidax_pool_set_buses: the pool's mix buses (the first call with a count allocates: a set-up side call; 0: off)"""
        _check(lib().aidax_pool_set_buses(self.h, n_buses))

    @property
    def buses(self) -> int:
        return int(lib().aidax_pool_buses(self.h))

    def set_send(self, stream: int, send: int, bus: int, gain: float = 1.0, ramp_frames: int = 0):
        """aidax_pool_set_send: send `send` (0 .. SENDS - 1) of `stream` (ALL_STREAMS: of every stream) goes to `bus` (BUS_NONE: nowhere)
        and its gain moves to `gain` over the stream's next `ramp_frames` frames (0: a jump at the block boundary)"""
        _check(lib().aidax_pool_set_send(self.h, stream, send, bus, gain, ramp_frames))

    def stream_send(self, stream: int, send: int):
        """aidax_pool_stream_send: (bus, gain_now, gain_target, frames_left) behind the last pass issued"""
        b, now, target, left = C.c_int32(0), C.c_float(0), C.c_float(0), C.c_uint32(0)
        _check(lib().aidax_pool_stream_send(self.h, stream, send, C.byref(b), C.byref(now), C.byref(target), C.byref(left)))
        return b.value, now.value, target.value, left.value

    def read_buses(self, first: int = 0, count: Optional[int] = None) -> np.ndarray:
        """aidax_pool_read_buses: rows `first` .. of the last mixed pass's bus block as [count][n_frames] (default: all from `first` on),
        behind every pass issued so far"""
        if count is None:
            count = self.buses - first
        out = np.zeros((max(count, 0), self.max_frames), np.float32)
        n = C.c_uint32(0)
        _check(lib().aidax_pool_read_buses(self.h, first, count, out.ctypes.data_as(_fp), out.size, C.byref(n)))
        return np.ascontiguousarray(out.reshape(-1)[:count * n.value].reshape(count, n.value))

    @property
    def buses_device(self) -> int:
        """aidax_pool_buses_device: the device address of the bus block ([buses][n_frames] of the last pass mixed)"""
        d = C.c_void_p()
        _check(lib().aidax_pool_buses_device(self.h, C.byref(d)))
        return d.value

    def process_buses(self, x: np.ndarray) -> np.ndarray:
        """aidax_pool_process_buses: one blocking pass that downloads the buses only, [buses][n_frames]"""
        x = _f32(x)
        assert x.ndim == 2 and x.shape[0] == self.n_streams
        out = np.empty((self.buses, x.shape[1]), np.float32)
        _check(lib().aidax_pool_process_buses(self.h, x.ctypes.data_as(_fp), out.ctypes.data_as(_fp), x.shape[1]))
        return out

    def set_bus_limiting(self, on: bool, max_lookahead_frames: int = BUS_LOOKAHEAD_MAX, max_hold_frames: int = BUS_HOLD_MAX):
        """aidax_pool_set_bus_limiting: the limiter and meter stage behind the buses on or off (the first enabling call allocates and
        fixes the capacities: a set-up side call)"""
        _check(lib().aidax_pool_set_bus_limiting(self.h, 1 if on else 0, max_lookahead_frames, max_hold_frames))

    @property
    def bus_limiting(self) -> bool:
        return bool(lib().aidax_pool_bus_limiting(self.h))

    def set_bus_limiter(self, params: Optional[BusLimitParams], bus: int = ALL_BUSES):
        """aidax_pool_set_bus_limiter: the bus's (default: every bus's) limiter from the next pass on, None: off"""
        _check(lib().aidax_pool_set_bus_limiter(self.h, bus, C.byref(params) if params is not None else None))

    def bus_limiter(self, bus: int):
        """aidax_pool_bus_limiter: (the bus's BusLimitParams as last set, whether its limiter is on, its latency in frames)"""
        out, on, latency = BusLimitParams(), C.c_int(0), C.c_uint32(0)
        _check(lib().aidax_pool_bus_limiter(self.h, bus, C.byref(out), C.byref(on), C.byref(latency)))
        return out, bool(on.value), latency.value

    def read_bus_meters(self, first: int = 0, count: Optional[int] = None, clear: bool = False) -> np.ndarray:
        """aidax_pool_read_bus_meters: the records of `count` buses from `first` (default: all from `first` on) as a structured array
        with aidax_bus_meter's field names, behind every pass issued so far; clear resets exactly those records behind the copy"""
        if count is None:
            count = self.buses - first
        out = np.zeros(max(count, 0), BUS_METER_DTYPE)
        _check(lib().aidax_pool_read_bus_meters(self.h, first, count, out.ctypes.data_as(C.POINTER(BusMeter)), 1 if clear else 0))
        return out

    def set_bus_reverbs(self, on: bool, max_delay_frames: int = 4096):
        """aidax_pool_set_bus_reverbs: the reverb stage between the buses and their limiters on or off (the first enabling call
        allocates and fixes the delay capacity: a set-up side call)"""
        _check(lib().aidax_pool_set_bus_reverbs(self.h, 1 if on else 0, max_delay_frames))

    @property
    def bus_reverbs(self) -> bool:
        return bool(lib().aidax_pool_bus_reverbs(self.h))

    def set_bus_reverb(self, params: Optional[BusReverbParams], bus: int = ALL_BUSES):
        """aidax_pool_set_bus_reverb: the bus's (default: every bus's) reverb from the next pass on, None: off"""
        _check(lib().aidax_pool_set_bus_reverb(self.h, bus, C.byref(params) if params is not None else None))

    def set_bus_reverb_rec(self, rec: Optional[BusReverbRec], bus: int = ALL_BUSES):
        """aidax_pool_set_bus_reverb_rec: the same with a record of the caller's own, None: off"""
        _check(lib().aidax_pool_set_bus_reverb_rec(self.h, bus, C.byref(rec) if rec is not None else None))

    def bus_reverb(self, bus: int):
        """aidax_pool_bus_reverb: (the bus's BusReverbParams as last set, its BusReverbRec, whether its reverb is on, frames since its epoch)"""
        out, rec, on, since = BusReverbParams(), BusReverbRec(), C.c_int(0), C.c_uint64(0)
        _check(lib().aidax_pool_bus_reverb(self.h, bus, C.byref(out), C.byref(rec), C.byref(on), C.byref(since)))
        return out, rec, bool(on.value), since.value

    def reset_bus_reverb(self, bus: int = ALL_BUSES):
        """aidax_pool_reset_bus_reverb: the bus's (default: every bus's) memories are cut at the next pass's first frame"""
        _check(lib().aidax_pool_reset_bus_reverb(self.h, bus))

    def set_controls(self, c: Controls, stream: int = ALL_STREAMS):
        _check(lib().aidax_pool_set_controls(self.h, stream, C.byref(c)))

    def set_loading(self, loading: bool, stream: int = ALL_STREAMS):
        _check(lib().aidax_pool_set_loading(self.h, stream, 1 if loading else 0))

    def activate(self, stream: int = ALL_STREAMS):
        _check(lib().aidax_pool_activate(self.h, stream))

    def process(self, x: np.ndarray) -> np.ndarray:
        x = _f32(x)
        assert x.ndim == 2 and x.shape[0] == self.n_streams
        out = np.empty_like(x)
        _check(lib().aidax_pool_process(self.h, x.ctypes.data_as(_fp), out.ctypes.data_as(_fp), x.shape[1]))
        return out

    def submit(self, x: np.ndarray):
        x = _f32(x)
        assert x.ndim == 2 and x.shape[0] == self.n_streams
        _check(lib().aidax_pool_submit(self.h, x.ctypes.data_as(_fp), x.shape[1]))

    def register_host(self, arr: np.ndarray):
        """Page-lock a caller buffer once: blocks inside it are uploaded / downloaded without staging copies."""
        _check(lib().aidax_pool_register_host(self.h, C.c_void_p(arr.ctypes.data), arr.nbytes))

    def unregister_host(self, arr: np.ndarray):
        _check(lib().aidax_pool_unregister_host(self.h, C.c_void_p(arr.ctypes.data)))

    def submit_to(self, x: np.ndarray, out: np.ndarray):
        assert x.dtype == np.float32 and out.dtype == np.float32 and x.flags.c_contiguous and out.flags.c_contiguous
        assert x.ndim == 2 and x.shape[0] == self.n_streams and out.size >= x.size
        _check(lib().aidax_pool_submit_to(self.h, x.ctypes.data_as(_fp), out.ctypes.data_as(_fp), x.shape[1]))

    def collect(self, n_frames: int, out: Optional[np.ndarray] = None) -> np.ndarray:
        if out is None:
            out = np.empty((self.n_streams, n_frames), np.float32)
        _check(lib().aidax_pool_collect(self.h, out.ctypes.data_as(_fp), n_frames))
        return out

    def process_device(self, d_in: int, d_out: int, n_frames: int, stream: int = 0):
        """d_in/d_out: raw device pointers ([n_streams][n_frames] fp32); stream: hipStream_t as int."""
        _check(lib().aidax_pool_process_device(self.h, C.c_void_p(d_in), C.c_void_p(d_out), n_frames,
                                               C.c_void_p(stream) if stream else None))

    def sync(self):
        _check(lib().aidax_pool_sync(self.h))

    def export_stream_dsp(self, stream: int) -> "StreamDsp":
        d = StreamDsp()
        _check(lib().aidax_pool_export_stream_dsp(self.h, stream, C.byref(d)))
        return d

    def import_stream_dsp(self, stream: int, d: "StreamDsp"):
        _check(lib().aidax_pool_import_stream_dsp(self.h, stream, C.byref(d)))

    def reset_stream(self, stream: int, start_mode: int = START_WARMUP):
        _check(lib().aidax_pool_reset_stream(self.h, stream, start_mode))

    def read_state(self, stream: int = 0, layer: int = 0, hidden: int = 128):
        h, c = np.zeros(hidden, np.float32), np.zeros(hidden, np.float32)
        H = _check(lib().aidax_pool_read_state(self.h, stream, layer, h.ctypes.data_as(_fp), c.ctypes.data_as(_fp), hidden))
        return h[:H], c[:H]

    @property
    def kernel_name(self) -> str:
        return lib().aidax_pool_kernel_name(self.h).decode()

    def close(self):
        if self.h:
            for a in list(getattr(self, "_adapters", ())):      # a rate adapter borrows the pool: it goes first
                a.close()
            lib().aidax_pool_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Hub:
    """aidax_hub: many plugin instances of one process, one pool pass per audio period (one period of latency)."""

    def __init__(self, max_instances: int, max_frames: int = 256, samplerate: float = 48000.0, device: int = 0):
        h = C.c_void_p()
        _check(lib().aidax_hub_create(max_instances, max_frames, samplerate, device, C.byref(h)))
        self.h = h
        live_handles.add(self)

    def set_model(self, m: Optional[Model], start_mode: int = START_WARMUP):
        _check(lib().aidax_hub_set_model(self.h, m.h if m is not None else None, start_mode))

    def attach(self) -> int:
        slot = C.c_int32(-1)
        _check(lib().aidax_hub_attach(self.h, C.byref(slot)))
        return slot.value

    def detach(self, slot: int):
        _check(lib().aidax_hub_detach(self.h, slot))

    def attach_successor(self, prev: "Hub", prev_slot: int) -> int:
        slot = C.c_int32(-1)
        _check(lib().aidax_hub_attach_successor(self.h, prev.h if prev is not None else None, prev_slot, C.byref(slot)))
        return slot.value

    def adopt(self, slot: int, prev: "Hub", prev_slot: int):
        _check(lib().aidax_hub_adopt(self.h, slot, prev.h, prev_slot))

    def set_controls(self, slot: int, c: Controls):
        _check(lib().aidax_hub_set_controls(self.h, slot, C.byref(c)))

    def run(self, slot: int, x: np.ndarray) -> np.ndarray:
        x = _f32(x)
        out = np.empty_like(x)
        _check(lib().aidax_hub_run(self.h, slot, x.ctypes.data_as(_fp), out.ctypes.data_as(_fp), x.size))
        return out

    def set_deadline_us(self, us: int):
        _check(lib().aidax_hub_set_deadline_us(self.h, us))

    def flush(self):
        _check(lib().aidax_hub_flush(self.h))

    @property
    def deadline_launches(self) -> int:
        return lib().aidax_hub_deadline_launches(self.h)

    @property
    def latency_frames(self) -> int:
        return lib().aidax_hub_latency_frames(self.h)

    @property
    def attached(self) -> int:
        return lib().aidax_hub_attached(self.h)

    @property
    def launches(self) -> int:
        return lib().aidax_hub_launches(self.h)

    def close(self):
        if self.h:
            lib().aidax_hub_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Resampler:
    """aidax_resampler: the streaming polyphase resampler for n_streams streams (rate_in -> rate_out, delays d_in / d_out in frames)."""

    def __init__(self, n_streams: int, rate_in: float, rate_out: float, d_in: int = 0, d_out: int = 0, max_in_frames: int = 256,
                 device: int = 0):
        h = C.c_void_p()
        _check(lib().aidax_resampler_create(n_streams, rate_in, rate_out, d_in, d_out, max_in_frames, device, C.byref(h)))
        self.h = h
        live_handles.add(self)
        self.n_streams = n_streams
        self.d_in, self.d_out = d_in, d_out

    @property
    def ready(self) -> int:
        return int(lib().aidax_resampler_ready(self.h))

    @property
    def latency_frames(self):
        """the delays the stage was created with: (d_in input frames, d_out output frames)"""
        return self.d_in, self.d_out

    def process(self, x: np.ndarray, n_out: Optional[int] = None) -> np.ndarray:
        """append x ([n_streams][n_in]) and return the next n_out outputs (None: every output that is ready then)"""
        x = _f32(x)
        assert x.ndim == 2 and x.shape[0] == self.n_streams
        if n_out is None:
            _check(lib().aidax_resampler_process(self.h, x.ctypes.data_as(_fp), x.shape[1], None, 0))
            x = x[:, :0]
            n_out = self.ready
        out = np.empty((self.n_streams, n_out), np.float32)
        _check(lib().aidax_resampler_process(self.h, x.ctypes.data_as(_fp), x.shape[1], out.ctypes.data_as(_fp), n_out))
        return out

    def process_device(self, d_in: int, n_in: int, d_out: int, n_out: int, stream: int = 0):
        """d_in / d_out: raw device pointers ([n_streams][n_in] resp. [n_streams][n_out] fp32); stream: hipStream_t as int."""
        _check(lib().aidax_resampler_process_device(self.h, C.c_void_p(d_in) if d_in else None, n_in, C.c_void_p(d_out) if d_out else None, n_out,
                                                    C.c_void_p(stream) if stream else None))

    def reset_stream(self, stream: int):
        _check(lib().aidax_resampler_reset_stream(self.h, stream))

    def close(self):
        if self.h:
            lib().aidax_resampler_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class RateAdapter:
    """aidax_rate: a pool created at its model's rate, driven in blocks at the host's rate. Close it before the pool."""

    def __init__(self, pool: Pool, host_rate: float, max_frames: int = 256):
        h = C.c_void_p()
        _check(lib().aidax_rate_create(pool.h, host_rate, max_frames, C.byref(h)))
        self.h = h
        self.pool = pool
        live_handles.add(self)
        if not hasattr(pool, "_adapters"):
            pool._adapters = weakref.WeakSet()
        pool._adapters.add(self)
        self.n_streams = pool.n_streams

    @property
    def latency_frames(self) -> int:
        return int(lib().aidax_rate_latency_frames(self.h))

    def process(self, x: np.ndarray) -> np.ndarray:
        x = _f32(x)
        assert x.ndim == 2 and x.shape[0] == self.n_streams
        out = np.empty_like(x)
        _check(lib().aidax_rate_process(self.h, x.ctypes.data_as(_fp), out.ctypes.data_as(_fp), x.shape[1]))
        return out

    def process_device(self, d_in: int, d_out: int, n_frames: int, stream: int = 0):
        _check(lib().aidax_rate_process_device(self.h, C.c_void_p(d_in) if d_in else None, C.c_void_p(d_out) if d_out else None, n_frames,
                                               C.c_void_p(stream) if stream else None))

    def reset_stream(self, stream: int):
        _check(lib().aidax_rate_reset_stream(self.h, stream))

    def close(self):
        if self.h:
            lib().aidax_rate_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
