"""CPU tests of the cabinet IR stage's host side: both builds of the library export its C ABI, and the WAV reader
(aidax_ir_load_wav) returns exact samples, length and rate for every format it reads, and an error code with a message,
never a crash or a read past the buffer, for every malformed file. The WAV files are synthesised here."""
import ctypes as C
import importlib
import struct

import numpy as np
import pytest

ax = importlib.import_module("aidadsp-lv2_amd")
IR_SYMBOLS = ("aidax_ir_load_wav", "aidax_pool_prepare_ir", "aidax_pool_commit_ir", "aidax_pool_set_ir")
ERR_ARG, ERR_IO = -1, -2
_SUBTYPE_TAIL = bytes([0x00, 0x00, 0x10, 0x00, 0x80, 0x00, 0x00, 0xAA, 0x00, 0x38, 0x9B, 0x71])


def test_both_libraries_export_the_ir_abi():
    from tests.conftest import HOOKS_LIB, SHIP_LIB
    for name in IR_SYMBOLS:
        assert name in ax.declared_symbols()
    for path in (SHIP_LIB, HOOKS_LIB):
        L = C.CDLL(path)
        assert [n for n in IR_SYMBOLS if not hasattr(L, n)] == [], path


def _chunk(cid: bytes, body: bytes) -> bytes:
    return cid + struct.pack("<I", len(body)) + body + (b"\0" if len(body) & 1 else b"")


def _fmt(tag, channels, rate, bits, extensible=False):
    align = channels * bits // 8
    body = struct.pack("<HHIIHH", 0xFFFE if extensible else tag, channels, rate, rate * align, align, bits)
    if extensible:
        body += struct.pack("<HHI", 22, bits, 0) + struct.pack("<I", tag) + _SUBTYPE_TAIL
    return _chunk(b"fmt ", body)


def _riff(*chunks: bytes) -> bytes:
    payload = b"WAVE" + b"".join(chunks)
    return b"RIFF" + struct.pack("<I", len(payload)) + payload


def _encode(x: np.ndarray, tag: int, bits: int) -> bytes:
    """x: [frames][channels] of the raw sample values (integers for PCM, float32 for IEEE float)"""
    if tag == 3:
        return np.ascontiguousarray(x, dtype="<f4").tobytes()
    if bits == 16:
        return np.ascontiguousarray(x, dtype="<i2").tobytes()
    if bits == 32:
        return np.ascontiguousarray(x, dtype="<i4").tobytes()
    u = np.ascontiguousarray(x, dtype="<i4").view(np.uint8).reshape(*x.shape, 4)[..., :3]       # 24-bit: the low three bytes
    return np.ascontiguousarray(u).tobytes()


def _raw(rng, frames, channels, tag, bits):
    if tag == 3:
        return rng.uniform(-1.5, 1.5, (frames, channels)).astype(np.float32)
    lo, hi = -(1 << (bits - 1)), (1 << (bits - 1)) - 1
    x = rng.integers(lo, hi, (frames, channels), endpoint=True, dtype=np.int64)
    x[0, 0], x[1 % frames, 0] = lo, hi                                    # both ends of the range
    return x


def _expected(raw, tag, bits):
    c0 = raw[:, 0]
    if tag == 3:
        return c0.astype(np.float32)
    return (c0.astype(np.float64) / float(1 << (bits - 1))).astype(np.float32)


def _load(path, cap=None):
    L = ax.lib()
    n, sr = C.c_uint32(0), C.c_double(0.0)
    if cap is None:
        buf = np.zeros(1, np.float32)
        rc = L.aidax_ir_load_wav(str(path).encode(), None, 0, C.byref(n), C.byref(sr))
    else:
        buf = np.full(cap + 4, -7.0, np.float32)                           # a guard behind cap: the reader writes no further
        rc = L.aidax_ir_load_wav(str(path).encode(), buf.ctypes.data_as(C.POINTER(C.c_float)), cap, C.byref(n), C.byref(sr))
    return rc, buf, n.value, sr.value


@pytest.mark.parametrize("tag,bits", [(1, 16), (1, 24), (1, 32), (3, 32)])
@pytest.mark.parametrize("channels", [1, 2])
@pytest.mark.parametrize("extensible", [False, True])
def test_wav_reader_returns_exact_samples(tmp_path, tag, bits, channels, extensible):
    rng = np.random.default_rng(bits * 10 + channels + 100 * extensible + tag)
    frames, rate = 517, 44100 + 3 * bits
    raw = _raw(rng, frames, channels, tag, bits)
    extra = [_chunk(b"LIST", b"INFOISFT\x05\0\0\0test\0"), _chunk(b"junk", b"\x01\x02\x03")]      # unknown chunks (one of odd size) around fmt
    data = _encode(raw, tag, bits)
    path = tmp_path / "ir.wav"
    path.write_bytes(_riff(extra[0], _fmt(tag, channels, rate, bits, extensible), extra[1], _chunk(b"data", data)))
    rc, _, n, sr = _load(path)                                             # cap == 0: length and rate only
    assert (rc, n, sr) == (0, frames, float(rate))
    taps, sr2 = ax.load_ir_wav(str(path))
    assert sr2 == float(rate) and taps.dtype == np.float32
    assert np.array_equal(taps.view(np.uint32), _expected(raw, tag, bits).view(np.uint32))
    rc, buf, n, _ = _load(path, cap=100)                                   # a short buffer: the first cap samples, the file's length
    assert (rc, n) == (0, frames)
    assert np.array_equal(buf[:100], _expected(raw, tag, bits)[:100]) and np.all(buf[100:] == -7.0)


def test_wav_reader_reads_a_cabinet_ir_shaped_like_the_references(tmp_path):
    """mono, 48 kHz, 24-bit PCM, 8192 frames: seeded exponentially decaying noise"""
    rng = np.random.default_rng(8192)
    t = np.arange(8192)
    h = rng.standard_normal(8192) * np.exp(-t / 900.0)
    raw = np.round(h / np.abs(h).max() * 0.9 * (1 << 23)).astype(np.int64).reshape(-1, 1)
    path = tmp_path / "cab.wav"
    path.write_bytes(_riff(_fmt(1, 1, 48000, 24), _chunk(b"data", _encode(raw, 1, 24))))
    taps, sr = ax.load_ir_wav(str(path))
    assert sr == 48000.0 and taps.size == 8192
    assert np.array_equal(taps, (raw[:, 0] / float(1 << 23)).astype(np.float32))
    assert np.abs(taps).max() <= 1.0


def _good(frames=64):
    raw = np.arange(frames, dtype=np.int64).reshape(-1, 1) * 100
    return _fmt(1, 1, 48000, 16), _chunk(b"data", _encode(raw, 1, 16))


def _cases():
    fmt, data = _good()
    full = _riff(fmt, data)
    long_data = b"data" + struct.pack("<I", 10_000) + b"\0" * 128                    # data size beyond the end of the file
    ext_bad = _chunk(b"fmt ", struct.pack("<HHIIHH", 0xFFFE, 1, 48000, 96000, 2, 16) + struct.pack("<HHI", 22, 16, 0)
                     + struct.pack("<I", 1) + bytes(12))                              # EXTENSIBLE with an unknown subformat GUID
    return {
        "empty": b"",
        "not_riff": b"RIFX" + full[4:],
        "not_wave": full[:8] + b"AVI " + full[12:],
        "header_only": full[:12],
        "truncated_chunk_header": full[:12 + 5],
        "truncated_fmt": full[:12 + 8 + 7],
        "fmt_too_short": _riff(_chunk(b"fmt ", b"\x01\x00\x01\x00"), data),
        "truncated_data": full[:-10],
        "data_past_end": _riff(fmt) + long_data,
        "no_fmt": _riff(data),
        "no_data": _riff(fmt),
        "zero_frames": _riff(fmt, _chunk(b"data", b"")),
        "partial_frame_only": _riff(_fmt(1, 2, 48000, 24), _chunk(b"data", b"\1\2\3\4\5")),
        "alaw_tag": _riff(_fmt(6, 1, 48000, 8), _chunk(b"data", b"\0" * 16)),
        "pcm_8bit": _riff(_fmt(1, 1, 48000, 8), _chunk(b"data", b"\0" * 16)),
        "float64": _riff(_fmt(3, 1, 48000, 64), _chunk(b"data", b"\0" * 64)),
        "zero_channels": _riff(_fmt(1, 0, 48000, 16), data),
        "bad_block_align": _riff(_chunk(b"fmt ", struct.pack("<HHIIHH", 1, 1, 48000, 96000, 3, 16)), data),
        "zero_rate": _riff(_fmt(1, 1, 0, 16), data),
        "extensible_short": _riff(_chunk(b"fmt ", struct.pack("<HHIIHH", 0xFFFE, 1, 48000, 96000, 2, 16) + b"\0\0"), data),
        "extensible_unknown_guid": _riff(ext_bad, data),
        "huge_chunk_size": _riff(fmt) + b"LIST" + struct.pack("<I", 0xFFFFFFFF) + b"xx",
    }


@pytest.mark.parametrize("name", sorted(_cases()))
def test_wav_reader_refuses_malformed_files_with_a_message(tmp_path, name):
    path = tmp_path / f"{name}.wav"
    path.write_bytes(_cases()[name])
    for cap in (None, 64):
        rc, buf, n, sr = _load(path, cap)
        assert rc == ERR_ARG, (name, rc)
        assert (n, sr) == (0, 0.0)
        msg = ax.lib().aidax_last_error().decode()
        assert msg.startswith(str(path)) and len(msg) > len(str(path)) + 2, msg
        if cap is not None:
            assert np.all(buf == -7.0)                                      # nothing written on failure
    with pytest.raises(ax.AidaxError):
        ax.load_ir_wav(str(path))


def test_wav_reader_reports_unreadable_files(tmp_path):
    rc, _, _, _ = _load(tmp_path / "missing.wav")
    assert rc == ERR_IO
    assert "cannot open" in ax.lib().aidax_last_error().decode()
    rc, _, _, _ = _load(tmp_path)                                           # a directory
    assert rc in (ERR_IO, ERR_ARG)


def test_wav_reader_null_arguments():
    L = ax.lib()
    n, sr = C.c_uint32(0), C.c_double(0.0)
    assert L.aidax_ir_load_wav(None, None, 0, C.byref(n), C.byref(sr)) == ERR_ARG
    assert L.aidax_ir_load_wav(b"x.wav", None, 4, C.byref(n), C.byref(sr)) == ERR_ARG      # cap > 0 needs a buffer
    assert L.aidax_ir_load_wav(b"x.wav", None, 0, None, C.byref(sr)) == ERR_ARG


def test_ir_calls_refuse_null_pools():
    L = ax.lib()
    sg = C.c_void_p()
    assert L.aidax_pool_prepare_ir(None, None, 0, 48000.0, C.byref(sg)) == ERR_ARG
    assert L.aidax_pool_commit_ir(None, None) == ERR_ARG
    assert L.aidax_pool_set_ir(None, None, 0, 48000.0) == ERR_ARG
