"""Long-form segmentation on the device (csrc/segment.hip): a 16 kHz recording is cut into utterance-sized segments at
pauses, so that ``SpeechT5ForSpeechToTextMI355X.transcribe_long`` can hand each one to the decoder, whose rows end at 450 tokens.

    db = frame_energy_db(wave)             # f32 [F], the encoder's frames: frame t covers samples [320 t, 320 t + 400)
    seg = segment(wave, max_segment_s=15)  # Segments: frame and sample bounds on the device, count and threshold on the host
    seg = segment_channels(waves, crosstalk_db=15.0)  # [C, n], one speaker per channel: each channel cut on its own, ChannelSegments

Parity unpinned: the reference has no counterpart; the rules are pinned by the numpy restatement in tests/segment_ref.py.  CUDA
tensors only: without a GPU both functions raise.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, fields
from typing import Optional

import torch

from . import _lib

HOP, WINDOW, FRAME_RATE, SAMPLE_RATE = 320, 400, 50, 16000


@dataclass
class VadParams:
    """The fields of LocoVadParams (include/loco_asr.h); seconds become frames by round(s * 50)."""
    max_segment_s: float = 20.0
    min_segment_s: float = 1.0
    min_silence_s: float = 0.3
    min_speech_s: float = 0.1
    pad_s: float = 0.2
    noise_quantile: float = 0.10
    peak_quantile: float = 0.99
    margin_db: float = 10.0
    abs_floor_db: float = -60.0
    min_dynamic_db: float = 15.0
    trim: bool = True

    def to_c(self) -> _lib.LocoVadParams:
        p = _lib.LocoVadParams()
        p.struct_size = C.sizeof(_lib.LocoVadParams)
        p.trim = 1 if self.trim else 0
        for f in fields(self):
            if f.name != "trim":
                setattr(p, f.name, float(getattr(self, f.name)))
        return p

    def frames(self):
        """(max_frames, min_frames, min_silence, min_speech, pad) as the library derives them; ValueError naming a refused field."""
        out = (C.c_int32 * 5)()
        _lib.check(_lib.load().loco_vad_frames(C.byref(self.to_c()), out), "VadParams")
        return tuple(out)


def resolve_params(vad=None, **params) -> VadParams:
    """``vad``: None, a VadParams or a dict of its fields; keyword fields override it.  Checked on the host (ValueError by name)."""
    if isinstance(vad, VadParams):
        base = {f.name: getattr(vad, f.name) for f in fields(vad)}
    elif vad is None:
        base = {}
    else:
        base = dict(vad)
    base.update(params)
    known = {f.name for f in fields(VadParams)}
    for k in base:
        if k not in known:
            raise TypeError(f"unknown segmentation parameter '{k}' (known: {', '.join(sorted(known))})")
    p = VadParams(**base)
    p.frames()
    return p


@dataclass
class Segments:
    """What ``segment`` returns.  ``start_frames`` / ``end_frames`` i32 [count] on the device (end exclusive), ``start_samples`` /
    ``end_samples`` i64 [count] on the device with start = 320 start_frame and end = min(n, 320 end_frame + 80) -- the samples the
    segment's frames cover; ``threshold_db`` (+inf: a silent recording, -inf: no usable silence, every frame speech) and ``count`` on
    the host."""
    start_frames: torch.Tensor
    end_frames: torch.Tensor
    start_samples: torch.Tensor
    end_samples: torch.Tensor
    threshold_db: float
    count: int
    samples: int = 0  # of the waveform


MAX_CHANNELS = 8
DEFAULT_CROSSTALK_DB = 15.0  # this project's own rule, like the gate itself; not validated on real two-channel telephone audio


@dataclass
class ChannelSegments:
    """What ``segment_channels`` returns: the segments of all channels merged into (start, channel) order.  ``channel`` i32 [count],
    ``start_frames`` / ``end_frames`` i32 [count] (end exclusive), ``start_samples`` / ``end_samples`` i64 [count] as in Segments,
    ``overlap_frames`` i32 [count] -- the frames of the segment in which another channel's cleaned speech mask is set -- all on the
    device; ``threshold_db`` and ``counts``: one entry per channel, on the host; ``count`` = sum(counts)."""
    channel: torch.Tensor
    start_frames: torch.Tensor
    end_frames: torch.Tensor
    start_samples: torch.Tensor
    end_samples: torch.Tensor
    overlap_frames: torch.Tensor
    threshold_db: list
    counts: list
    count: int
    samples: int = 0  # of every channel
    channels: int = 0


# A mono recording is the one-channel case: everything below works on [C, ...] tensors, and with ``mono`` on the same tensors without
# the leading dimension -- C = 1, no extra view or row-0 operation on the way, the messages and the C entry point the mono function's own.
def _check_crosstalk(crosstalk_db):
    v = float(crosstalk_db)
    if not v >= 0.0:
        raise ValueError(f"crosstalk_db = {v:g} is NaN or negative (inf switches the gate off)")
    return v


def _waves(waves, what, mono=False):
    """The checked waveforms as contiguous f32 [C, samples]; ``mono``: [samples]."""
    if not torch.is_tensor(waves) or not waves.is_cuda:
        raise RuntimeError(f"{what} runs on an AMD GPU only: the waveform{'' if mono else 's'} must be a CUDA tensor (there is no CPU path)")
    if waves.dim() != (1 if mono else 2):
        raise ValueError(f"{what}: expected {'a 1-D waveform [samples]' if mono else 'waveforms [channels, samples]'}, got {tuple(waves.shape)}")
    if not mono and not 1 <= waves.shape[0] <= MAX_CHANNELS:
        raise ValueError(f"{what}: {waves.shape[0]} channels are outside 1 .. {MAX_CHANNELS}")
    if waves.shape[-1] < WINDOW:
        raise ValueError(f"{what}: {waves.shape[-1]} samples are shorter than one encoder frame ({WINDOW})")
    return waves.to(torch.float32).contiguous()


def _energy(waves, mono=False):
    """f32 [C, F] of checked waveforms [C, samples] in one launch."""
    lib = _lib.load()
    ch, n, F = 1 if mono else int(waves.shape[0]), int(waves.shape[-1]), int(lib.loco_output_frames(int(waves.shape[-1])))
    db = torch.empty((F,) if mono else (ch, F), dtype=torch.float32, device=waves.device)  # a plain tuple: a torch.Size parses slower
    with torch.cuda.device(waves.device):
        stream = torch.cuda.current_stream(waves.device).cuda_stream  # pointers go as plain integers: the argtypes say void*
        if mono:
            _lib.check(lib.loco_op_frame_energy_db(waves.data_ptr(), n, db.data_ptr(), stream), "loco_op_frame_energy_db")
        else:
            _lib.check(lib.loco_op_frame_energy_db_channels(waves.data_ptr(), ch, n, int(waves.stride(0)), db.data_ptr(), stream),
                       "loco_op_frame_energy_db_channels")
    return db


def _segments_from_db(db, params, crosstalk_db, max_segments, overlap, mono=False):
    """The segmentation launch (and the overlap launch) on a checked f32 [C, F] CUDA tensor: (start_frames i32 [C, max_segments],
    end_frames, overlap_frames or None, count i32 [C], threshold f32 [C]), all on the device and nothing read back."""
    db = db.contiguous()
    lib = _lib.load()
    ch, F = 1 if mono else int(db.shape[0]), int(db.shape[-1])
    maxf, minf = params.frames()[:2]
    if max_segments is None:  # every step but the last advances by at least min(min_frames + 1, max_frames // 2) frames
        max_segments = F // min(minf + 1, maxf // 2) + 1
    dev = db.device
    start = torch.empty((max(int(max_segments), 0),) if mono else (ch, max(int(max_segments), 0)), dtype=torch.int32, device=dev)
    end = torch.empty_like(start)
    over = torch.zeros_like(start) if overlap else None
    count = torch.empty(ch, dtype=torch.int32, device=dev)
    thr = torch.empty(ch, dtype=torch.float32, device=dev)
    ws_bytes = int(lib.loco_vad_workspace_bytes(F) if mono else lib.loco_vad_channels_workspace_bytes(ch, F))
    ws = torch.empty(max(ws_bytes, 16), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        par = C.byref(params.to_c())
        tail = (int(max_segments), count.data_ptr(), thr.data_ptr(), ws.data_ptr(), ws_bytes, torch.cuda.current_stream(dev).cuda_stream)
        if mono:
            _lib.check(lib.loco_op_vad_segments(db.data_ptr(), F, par, start.data_ptr(), end.data_ptr(), *tail), "loco_op_vad_segments")
        else:
            _lib.check(lib.loco_op_vad_segments_channels(db.data_ptr(), ch, F, par, crosstalk_db, start.data_ptr(), end.data_ptr(),
                                                         over.data_ptr() if overlap else None, *tail), "loco_op_vad_segments_channels")
    return start, end, over, count, thr


def _segment(waves, params, crosstalk_db, what, mono=False):
    """``segment_channels`` on checked arguments; ``mono``: one channel, no overlap launch and ``overlap_frames`` None."""
    ch, n = 1 if mono else int(waves.shape[0]), int(waves.shape[-1])
    db = _energy(waves, mono)
    start, end, over, count, thr = _segments_from_db(db, params, crosstalk_db, None, not mono, mono)
    if mono:
        start, end = start[None], end[None]
    host = torch.cat([count.to(torch.float64), thr.to(torch.float64)]).cpu().tolist()  # the one read-back: both are exact in float64
    counts, thrs = [int(v) for v in host[:ch]], host[ch:]
    for c, k in enumerate(counts):
        if k < 0:
            raise _lib.LocoError(f"{what}: {-k} segments{'' if mono else f' of channel {c}'} exceed the {start.shape[1]} the rules allow "
                                 f"for {db.shape[-1]} frames")
    dev = waves.device
    chan = torch.cat([torch.full((k,), c, dtype=torch.int32, device=dev) for c, k in enumerate(counts)])
    flat = lambda t: torch.cat([t[c, :k] for c, k in enumerate(counts)])  # noqa: E731
    start, end, over = flat(start), flat(end), None if mono else flat(over)
    if ch > 1:
        order = torch.argsort(start.to(torch.int64) * MAX_CHANNELS + chan.to(torch.int64))  # the keys are distinct: (start, channel) order
        chan, start, end, over = chan[order], start[order], end[order], over[order]
    return ChannelSegments(channel=chan, start_frames=start, end_frames=end, start_samples=start.to(torch.int64) * HOP,
                           end_samples=torch.clamp(end.to(torch.int64) * HOP + (WINDOW - HOP), max=n), overlap_frames=over,
                           threshold_db=thrs, counts=counts, count=sum(counts), samples=n, channels=ch)


def frame_energy_db_channels(waves: torch.Tensor) -> torch.Tensor:
    """f32 [C, F]: 10 log10(mean(x^2) + 1e-12) of every encoder frame of every row of a [C, samples] 16 kHz CUDA tensor in one launch; a
    row's bits do not depend on the rows beside it."""
    return _energy(_waves(waves, "frame_energy_db_channels"))


def frame_energy_db(wave: torch.Tensor) -> torch.Tensor:
    """f32 [F]: ``frame_energy_db_channels`` of a 1-D 16 kHz CUDA waveform, the one-channel case."""
    return _energy(_waves(wave, "frame_energy_db", mono=True), mono=True)


def segments_channels_from_db(db: torch.Tensor, params: VadParams, crosstalk_db: float = DEFAULT_CROSSTALK_DB,
                              max_segments: Optional[int] = None, overlap: bool = True):
    """The per-channel segmentation kernel (and the overlap kernel) on a given f32 [C, F] CUDA tensor: (start_frames i32
    [C, max_segments], end_frames, overlap_frames or None, count i32 [C], threshold f32 [C]), all on the device, nothing read back.
    ``max_segments`` None = the most the rules can produce for F frames."""
    crosstalk_db = _check_crosstalk(crosstalk_db)
    if not torch.is_tensor(db) or not db.is_cuda or db.dim() != 2 or db.dtype != torch.float32:
        raise RuntimeError("segments_channels_from_db: db must be a 2-D float32 CUDA tensor [channels, frames] (there is no CPU path)")
    return _segments_from_db(db, params, crosstalk_db, max_segments, overlap)


def segments_from_db(db: torch.Tensor, params: VadParams, max_segments: Optional[int] = None):
    """The one-channel case on a given f32 [F] CUDA tensor, without gate and overlap: (start_frames i32 [max_segments], end_frames,
    count i32 [1], threshold f32 [1])."""
    if not torch.is_tensor(db) or not db.is_cuda or db.dim() != 1 or db.dtype != torch.float32:
        raise RuntimeError("segments_from_db: db must be a 1-D float32 CUDA tensor (there is no CPU path)")
    start, end, _, count, thr = _segments_from_db(db, params, float("inf"), max_segments, False, mono=True)
    return start, end, count, thr


def segment_channels(waves: torch.Tensor, crosstalk_db: float = DEFAULT_CROSSTALK_DB, vad=None, **params) -> ChannelSegments:
    """Cut every channel of a [C, samples] 16 kHz CUDA tensor at its own pauses (one speaker per channel): three launches (energies,
    one workgroup per channel, overlap), then the counts and the thresholds are read back together.  A frame of a channel is not speech
    when another channel is louder there by more than ``crosstalk_db`` (inf: no gate).  Parameters: the fields of VadParams, as
    keywords or as ``vad`` (a VadParams or a dict)."""
    p = resolve_params(vad, **params)
    crosstalk_db = _check_crosstalk(crosstalk_db)
    return _segment(_waves(waves, "segment_channels"), p, crosstalk_db, "segment_channels")


def segment(wave: torch.Tensor, vad=None, **params) -> Segments:
    """Cut a 1-D 16 kHz CUDA waveform at pauses, the one-channel case: two launches (energy, segmentation), then the count and the
    threshold are read back together.  Parameters as ``segment_channels``."""
    p = resolve_params(vad, **params)
    s = _segment(_waves(wave, "segment", mono=True), p, float("inf"), "segment", mono=True)
    return Segments(start_frames=s.start_frames, end_frames=s.end_frames, start_samples=s.start_samples, end_samples=s.end_samples,
                    threshold_db=s.threshold_db[0], count=s.count, samples=s.samples)


@dataclass
class LongSegment:
    """One segment of a LongTranscript: ``start_s`` / ``end_s`` in recording time, ``ids`` a 1-D LongTensor (host) as ``generate_many``
    returns it; ``token_logprobs`` [len - 1] (device), ``logprob`` and ``avg_logprob`` with ``return_scores``; ``token_times`` f32
    [len - 1, 2] (host), start and end of every generated token in recording time, with ``timestamps``.  From ``transcribe_channels``
    also ``channel`` (the index of the segment's channel) and ``overlap_s``, the seconds of it in which another channel speaks."""
    start_s: float
    end_s: float
    ids: torch.Tensor
    token_logprobs: Optional[torch.Tensor] = None
    logprob: Optional[float] = None
    avg_logprob: Optional[float] = None
    token_times: Optional[torch.Tensor] = None
    channel: Optional[int] = None
    overlap_s: Optional[float] = None


@dataclass
class LongTranscript:
    """What ``transcribe_long`` returns: the segments in time order, the recording's length and the speech threshold used.  From
    ``transcribe_channels``: the segments of all channels in (start, channel) order and ``threshold_db`` a list, one per channel."""
    segments: list
    duration_s: float
    threshold_db: float
