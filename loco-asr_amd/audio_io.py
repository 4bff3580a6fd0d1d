"""Reading audio files: 16 / 32-bit PCM and float WAV files and FLAC files (SLURP's format) are decoded here without libsndfile
(read_pcm_wav; the library's loco_flac_decode, CRC- and MD5-verified), anything else through soundfile when it is installed; the two
loaders hand files at another rate than 16 kHz to the device polyphase resampler (resample.py).  Used by extract.py and transcribe.py."""
from __future__ import annotations

import ctypes as C
import struct

import numpy as np

from . import _lib

_soundfile = None  # module, or False once its import has failed (a failed import is re-tried -- and re-paid -- on every call otherwise)


def read_pcm_wav(path: str):
    """(rate, float32 mono samples in [-1, 1)) of an uncompressed RIFF/WAVE file -- 16 / 32-bit PCM or 32-bit float, the formats
    SLURP's .wav files and this repo's synthetic corpora use -- or None for anything else (the caller falls back to scipy).
    One read, one frombuffer, one scaling pass: the loader threads share the interpreter lock with the thread that feeds the GPU,
    so the Python spent per file matters more than the bytes."""
    got = _read_pcm_wav_interleaved(path)
    if got is None:
        return None
    rate, channels, x = got
    if channels > 1:
        x = x[:x.size // channels * channels].reshape(-1, channels).mean(axis=1)
    return rate, x


def _read_pcm_wav_interleaved(path: str):
    """(rate, channels, float32 samples as the file interleaves them) -- read_pcm_wav before the channels are averaged -- or None."""
    with open(path, "rb") as fh:
        raw = fh.read()
    if len(raw) < 44 or raw[:4] != b"RIFF" or raw[8:12] != b"WAVE":
        return None
    pos, fmt, data = 12, None, None
    while pos + 8 <= len(raw):
        cid, size = raw[pos:pos + 4], struct.unpack_from("<I", raw, pos + 4)[0]
        if cid == b"fmt ":
            fmt = struct.unpack_from("<HHIIHH", raw, pos + 8)
        elif cid == b"data":
            data = (pos + 8, min(size, len(raw) - pos - 8))
            break
        pos += 8 + size + (size & 1)
    if fmt is None or data is None:
        return None
    tag, channels, rate, _, _, bits = fmt
    if tag == 1 and bits == 16:
        x = np.frombuffer(raw, dtype="<i2", count=data[1] // 2, offset=data[0]).astype(np.float32)
        x *= np.float32(1.0 / 32768.0)
    elif tag == 1 and bits == 32:
        x = np.frombuffer(raw, dtype="<i4", count=data[1] // 4, offset=data[0]).astype(np.float32)
        x *= np.float32(1.0 / 2147483648.0)
    elif tag == 3 and bits == 32:
        x = np.frombuffer(raw, dtype="<f4", count=data[1] // 4, offset=data[0]).astype(np.float32)
    else:
        return None
    return int(rate), int(channels), x


def _decode_flac(path: str, pcm: bool):
    """(rate, bits per sample, samples) of a FLAC file through the library's host-side decoder -- bit-exact integer decoding with the
    frame CRCs and the STREAMINFO MD5 signature verified.  ``pcm``: the library's interleaved int32 output [n, channels]; otherwise its
    float32 mono output [n], scaled and mixed down by the library."""
    lib = _lib.load()
    with open(path, "rb") as fh:
        raw = fh.read()
    sr, ch, bits, total = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int64()
    if lib.loco_flac_info(raw, len(raw), C.byref(sr), C.byref(ch), C.byref(bits), C.byref(total)):
        raise RuntimeError(f"{path}: {lib.loco_flac_last_error().decode()}")
    cap = int(total.value) if total.value > 0 else 8 * len(raw)  # unknown length: FLAC rarely beats 8 samples per byte... retried below
    while True:
        out = np.empty((cap, ch.value), dtype=np.int32) if pcm else np.empty(cap, dtype=np.float32)
        ptr, n = out.ctypes.data_as(C.c_void_p), C.c_int64()
        rc = lib.loco_flac_decode(raw, len(raw), None if pcm else ptr, ptr if pcm else None, cap, C.byref(n), 1)
        if rc == -3 and total.value <= 0:
            cap *= 4
            continue
        if rc:
            raise RuntimeError(f"{path}: {lib.loco_flac_last_error().decode()}")
        return int(sr.value), int(bits.value), out[:n.value]


def read_flac(path: str):
    """(rate, float32 mono samples) of a FLAC file, scaled and mixed down as soundfile.read(dtype='float32').mean(axis=1) would."""
    sr, _, x = _decode_flac(path, pcm=False)
    return sr, x


def read_flac_channels(path: str):
    """(rate, float32 [channels, n]) of a FLAC file: the library's interleaved int32 ``pcm`` output times 2^-(bits-1), which is what
    soundfile.read(dtype='float32') gives per channel."""
    sr, bits, pcm = _decode_flac(path, pcm=True)
    x = pcm.T.astype(np.float32)
    x *= np.float32(2.0 ** -(bits - 1))
    return sr, np.ascontiguousarray(x)


def _decode_mono(path: str):
    global _soundfile
    if _soundfile is None:
        try:
            import soundfile
            _soundfile = soundfile
        except ImportError:
            _soundfile = False
    got = read_pcm_wav(path) if path.lower().endswith(".wav") else None
    if got is None and path.lower().endswith(".flac") and not _soundfile:
        got = read_flac(path)  # SLURP's own format, decoded by the library (include/loco_asr.h, loco_flac_decode): no libsndfile needed
    if got is not None:
        return got
    if _soundfile:
        x, sr = _soundfile.read(path, dtype="float32", always_2d=True)
        return sr, x.mean(axis=1)
    from scipy.io import wavfile
    if not path.lower().endswith(".wav"):
        raise RuntimeError("install soundfile for this format, or convert to WAV / FLAC")
    sr, x = wavfile.read(path)
    if x.dtype.kind == "i":
        x = x.astype(np.float32) / float(np.iinfo(x.dtype).max + 1)
    elif x.dtype.kind == "u":  # 8-bit PCM is unsigned
        x = (x.astype(np.float32) - 128.0) / 128.0
    x = x.astype(np.float32)
    return sr, (x.mean(axis=1) if x.ndim == 2 else x)


def _decode_channels(path: str):
    low = path.lower()
    if low.endswith(".wav"):
        got = _read_pcm_wav_interleaved(path)
        if got is None:
            raise RuntimeError("not 16 / 32-bit PCM or 32-bit float RIFF/WAVE")
        sr, channels, x = got
        return sr, np.ascontiguousarray(x[:x.size // channels * channels].reshape(-1, channels).T)
    if low.endswith(".flac"):
        return read_flac_channels(path)
    raise RuntimeError("per-channel reading takes .wav and .flac files")


def _at_16k(decode, path: str, device):
    try:
        sr, x = decode(path)
    except Exception as e:  # a corpus of 100 000 files: the message must say WHICH one
        raise RuntimeError(str(e) if path in str(e) else f"cannot decode {path}: {e}") from e
    if sr != 16000:
        from . import resample
        return resample.resample_to_16k(x, int(sr), device=device)
    return x


def load_audio_16k(path: str, device=None):
    """mono float32 at 16 kHz (the reference uses librosa.load(path, sr=16000), …base…py:56): files at another rate (Fisher:
    8 kHz, podcasts: 44.1 kHz) are converted ON THE DEVICE by loco_op_resample (resample.py) and come back as CUDA tensors,
    which the feature extractor pads on the device; 16 kHz files stay numpy arrays on the host.  `device` = the rank's GPU: this
    runs on loader threads, where torch.cuda.current_device() is 0 whatever the main thread selected."""
    return _at_16k(_decode_mono, path, device)


def load_audio_channels_16k(path: str, device=None):
    """float32 [channels, n] at 16 kHz: ``load_audio_16k`` without the mix-down, for recordings with one speaker per channel (a
    two-channel telephone call).  WAV (the formats of read_pcm_wav) and FLAC are decoded here; files at another rate are converted ON
    THE DEVICE with the channels as the resampler's batch rows and come back as a CUDA tensor, 16 kHz files stay a numpy array on the
    host.  The mean over the channels of the result is ``load_audio_16k``'s output."""
    return _at_16k(_decode_channels, path, device)
