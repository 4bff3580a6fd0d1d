"""CPU tests of the per-channel segmentation's host side: the C entry points' refusals by name (host memory stands in for the pointers:
every refusal comes before any launch), the workspace size, the per-channel readers, the Kaldi formatter and its round trip through
the language-model side's readers, and the flag combinations the CLI refuses."""
import ctypes as C
import importlib
import re
import wave as wave_module

import numpy as np
import pytest
import torch

import flac_writer as fw

la = importlib.import_module("loco-asr_amd")
seg = importlib.import_module("loco-asr_amd.segment")
lm = importlib.import_module("loco-asr_amd.lm")
audio_io = importlib.import_module("loco-asr_amd.audio_io")
transcribe = importlib.import_module("loco-asr_amd.transcribe")
_libmod = importlib.import_module("loco-asr_amd._lib")


def test_workspace_size():
    lib = _libmod.load()
    for F in (1, 8, 1023, 180000):
        one = lib.loco_vad_workspace_bytes(F)
        for ch in range(1, 9):
            got = lib.loco_vad_channels_workspace_bytes(ch, F)
            assert got % 16 == 0 and ch * one <= got <= ch * (one + 15)  # a mono workspace per channel, slices 16-byte aligned
    for ch, F in ((0, 8), (9, 8), (-1, 8), (2, 0), (2, -5), (2, 2 ** 24 + 1)):
        assert lib.loco_vad_channels_workspace_bytes(ch, F) == 0


def test_cabi_refusals_come_before_any_launch():
    lib = _libmod.load()
    err = lambda: lib.loco_last_error().decode()  # noqa: E731
    wav, db = (C.c_float * 2000)(), (C.c_float * 16)()
    p = _libmod.LocoVadParams()
    lib.loco_vad_default_params(C.byref(p))
    start, end, over, count, thr = (C.c_int32 * 8)(), (C.c_int32 * 8)(), (C.c_int32 * 8)(), (C.c_int32 * 2)(), (C.c_float * 2)()
    ws = (C.c_uint8 * 4096)()
    assert lib.loco_vad_channels_workspace_bytes(2, 8) <= 4096

    fn = "loco_op_frame_energy_db_channels"
    assert lib.loco_op_frame_energy_db_channels(None, 2, 1000, 1000, db, None) == -1 and f"{fn}: null argument" in err()
    assert lib.loco_op_frame_energy_db_channels(wav, 2, 1000, 1000, None, None) == -1 and f"{fn}: null argument" in err()
    for ch in (0, 9, -3):
        assert lib.loco_op_frame_energy_db_channels(wav, ch, 1000, 1000, db, None) == -1 and f"{fn}: C = {ch} is outside 1 .. 8 channels" in err()
    assert lib.loco_op_frame_energy_db_channels(wav, 2, 399, 1000, db, None) == -1 and "n = 399 samples is shorter than one frame (400)" in err()
    assert lib.loco_op_frame_energy_db_channels(wav, 2, 1000, 999, db, None) == -1 and "stride = 999 is below n = 1000" in err()

    fn = "loco_op_vad_segments_channels"
    good = [db, 2, 8, C.byref(p), 15.0, start, end, over, 4, count, thr, ws, 4096, None]
    for i in (0, 3, 5, 6, 9, 10, 11):
        args = list(good)
        args[i] = None
        assert lib.loco_op_vad_segments_channels(*args) == -1 and f"{fn}: null argument" in err(), i
    for ch in (0, 9, -1):
        args = list(good)
        args[1] = ch
        assert lib.loco_op_vad_segments_channels(*args) == -1 and f"{fn}: C = {ch} is outside 1 .. 8 channels" in err()
    for x, shown in ((float("nan"), "nan"), (-0.5, "-0.5"), (float("-inf"), "-inf")):
        args = list(good)
        args[4] = x
        assert lib.loco_op_vad_segments_channels(*args) == -1 and f"crosstalk_db = {shown} is NaN or negative" in err()
    for F in (0, -1, 2 ** 24 + 1):
        args = list(good)
        args[2] = F
        assert lib.loco_op_vad_segments_channels(*args) == -1 and f"F = {F} is outside" in err()
    for k in (0, -2):
        args = list(good)
        args[8] = k
        assert lib.loco_op_vad_segments_channels(*args) == -1 and f"max_segments = {k} must be >= 1" in err()
    args = list(good)
    args[12] = lib.loco_vad_channels_workspace_bytes(2, 8) - 1
    assert lib.loco_op_vad_segments_channels(*args) == -1 and f"{fn}: workspace {args[12]} < {args[12] + 1} bytes" in err()
    bad = _libmod.LocoVadParams()
    lib.loco_vad_default_params(C.byref(bad))
    bad.min_segment_s = 20.0
    args = list(good)
    args[3] = C.byref(bad)
    assert lib.loco_op_vad_segments_channels(*args) == -1 and "min_segment_s = 20 is not below max_segment_s = 20" in err()
    assert C.sizeof(_libmod.LocoVadParams) == 88  # crosstalk_db is an argument: the struct keeps its layout


def test_python_refusals():
    with pytest.raises(RuntimeError, match="no CPU path"):
        seg.frame_energy_db_channels(torch.zeros(2, 1000))
    with pytest.raises(RuntimeError, match="no CPU path"):
        seg.segment_channels(torch.zeros(2, 1000))
    for x in (float("nan"), -1.0):
        with pytest.raises(ValueError, match="crosstalk_db = .* is NaN or negative"):
            seg.segment_channels(torch.zeros(2, 1000), crosstalk_db=x)
    with pytest.raises(ValueError, match="min_segment_s"):  # parameters are checked before the tensor is looked at
        seg.segment_channels(torch.zeros(2, 1000), min_segment_s=30)
    model = la.SpeechT5ForSpeechToTextMI355X(layers=1, decoder_layers=1)
    with pytest.raises(ValueError, match="max_segment_s = 31 exceeds"):
        model.transcribe_channels(torch.zeros(2, 1000), vad=dict(max_segment_s=31))
    with pytest.raises(RuntimeError, match="no CPU path"):
        model.transcribe_channels(torch.zeros(2, 1000))
    with pytest.raises(RuntimeError, match="needs the decoder"):
        la.SpeechT5ForSpeechToTextMI355X(layers=1).transcribe_channels(torch.zeros(2, 1000))
    sg = seg.LongSegment(0.0, 1.0, torch.zeros(2, dtype=torch.long))  # the new fields trail and default to None
    assert sg.channel is None and sg.overlap_s is None


# ---- readers ---------------------------------------------------------------------------------------------------------------------------
def two_channel_pcm(n):
    x = np.stack([la.synth.clip(3, n), 0.5 * la.synth.clip(4, n)], axis=1).astype(np.float64)
    return np.clip(np.round(x * 32768.0 * 0.8), -32768, 32767).astype(np.int64)  # [n, 2]


def test_wav_reader_keeps_the_channels(tmp_path):
    pcm = two_channel_pcm(16000 + 123)
    path = str(tmp_path / "call.wav")
    with wave_module.open(path, "wb") as fh:
        fh.setnchannels(2)
        fh.setsampwidth(2)
        fh.setframerate(16000)
        fh.writeframes(pcm.astype("<i2").tobytes())
    x = audio_io.load_audio_channels_16k(path)
    assert isinstance(x, np.ndarray) and x.shape == (2, len(pcm)) and x.dtype == np.float32 and x.flags["C_CONTIGUOUS"]
    assert np.array_equal(x, (pcm.T.astype(np.float32) * np.float32(1 / 32768)))
    mono = audio_io.load_audio_16k(path)
    assert np.array_equal(x.mean(axis=0), mono) and mono.dtype == np.float32


def test_flac_reader_keeps_the_channels(tmp_path):
    pcm = two_channel_pcm(3 * 1152 + 200)
    frames, at, k = [], 0, 0
    while at < len(pcm):
        s = min(1152, len(pcm) - at)
        frames.append(dict(size=s, assignment=(1, 8, 10, 9)[k % 4], specs=[dict(kind="fixed", order=2, porder=0), dict(kind="fixed", order=1, porder=0)]))
        at, k = at + s, k + 1
    path = str(tmp_path / "call.flac")
    with open(path, "wb") as fh:
        fh.write(fw.write_stream(pcm, 16, 16000, frames))
    x = audio_io.load_audio_channels_16k(path)
    assert isinstance(x, np.ndarray) and x.shape == (2, len(pcm)) and x.dtype == np.float32 and x.flags["C_CONTIGUOUS"]
    assert np.array_equal(x, (pcm.T.astype(np.float32) * np.float32(1 / 32768)))
    assert np.array_equal(x.mean(axis=0), audio_io.load_audio_16k(path))
    with pytest.raises(RuntimeError, match="call.ogg"):
        audio_io.load_audio_channels_16k(str(tmp_path / "call.ogg"))


# ---- Kaldi text ------------------------------------------------------------------------------------------------------------------------
UTT_ID = re.compile(r"^[^\s-]+-[A-H]-\d{6}-\d{6}$")


def test_kaldi_formatter():
    assert transcribe.kaldi_rec_id("/data/fe_03-00001 a.wav") == "fe_03_00001_a" and transcribe.kaldi_rec_id("x.tar.flac") == "x.tar"
    assert [transcribe.channel_name(c) for c in range(8)] == list("ABCDEFGH")
    lines = transcribe.kaldi_text_lines("fe_03_00001", [(0, 0, 160, "hello there"), (1, 159, 161, "  yes \t indeed "), (0, 4800, 4801, ""),
                                                         (1, 16000 * 3600, 16000 * 3600 + 1, "late"), (0, 320, 480, "   ")])
    assert lines == ["fe_03_00001-A-000000-000001 hello there", "fe_03_00001-B-000000-000002 yes indeed", "fe_03_00001-B-360000-360001 late"]
    for line in lines:
        assert UTT_ID.match(line.split(" ", 1)[0])
    assert transcribe.kaldi_text_lines("r", []) == []


def test_kaldi_lines_round_trip_through_the_lm_readers(tmp_path):
    """A and B of one recording come back from lm.recordings in time order, whatever the order of the lines; the recording is the id up
    to the first '-'."""
    class WordTokenizer:
        eos_token_id = 0

        def __init__(self):
            self.words = {}

        def __call__(self, text):
            return {"input_ids": [self.words.setdefault(w, len(self.words) + 1) for w in text.split()]}

    segs = {"call-1": [(0, 1600, 30000, "a0"), (1, 20000, 50000, "b1"), (0, 60000, 90000, "a2"), (1, 61000, 70000, "b3"), (1, 1000000, 1100000, "b4")],
            "other": [(1, 0, 1000, "o0"), (0, 500, 2000, "o1")]}
    lines = []
    for name, rows in segs.items():
        lines += transcribe.kaldi_text_lines(transcribe.kaldi_rec_id(name + ".wav"), list(reversed(rows)))  # written out of order
    path = tmp_path / "text"
    path.write_text("".join(l + "\n" for l in lines))
    utts = lm.read_key_text(str(path))
    assert len(utts) == 7 and all(UTT_ID.match(k) for k in utts)
    assert {lm.rec_id_of(k) for k in utts} == {"call_1", "other"}
    tok = WordTokenizer()
    recs = lm.recordings(utts, tok)
    back = {v: k for k, v in tok.words.items()}
    assert list(recs) == ["call_1", "other"]
    assert [back[t] for t in recs["call_1"] if t] == ["a0", "b1", "a2", "b3", "b4"]  # by start, A and B interleaved
    assert [back[t] for t in recs["other"] if t] == ["o0", "o1"]


# ---- CLI -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("extra,match", [
    (["--crosstalk-db", "10"], "--crosstalk-db needs --channels split"),
    (["--channels", "mix", "--crosstalk-db", "10"], "--crosstalk-db needs --channels split"),
    (["--kaldi-text", "out.txt"], "--kaldi-text needs --channels split"),
    (["--channels", "mix", "--kaldi-text", "out.txt"], "--kaldi-text needs --channels split"),
    (["--channels", "split", "--crosstalk-db", "-3"], "crosstalk_db = -3 is NaN or negative"),
    (["--channels", "split", "--crosstalk-db", "nan"], "crosstalk_db = nan is NaN or negative"),
    (["--channels", "split", "--kaldi-text", "out.txt"], "--kaldi-text needs a tokenizer found on disk"),
    (["--channels", "split", "--kaldi-text", "out.txt", "--tokenizer", "/nonexistent/dir"], "--kaldi-text needs a tokenizer found on disk"),
    (["--channels", "split", "--max-segment-s", "45"], "max_segment_s = 45 exceeds"),
    (["--channels", "split", "--nbest", "2", "--slots", "4"], "--long does not go with --nbest"),
])
def test_cli_refuses_before_a_model_is_built(extra, match, monkeypatch, tmp_path):
    def no_model(args):
        raise AssertionError("a model was built")
    monkeypatch.setattr(transcribe, "build_model", no_model)
    monkeypatch.chdir(tmp_path)
    with pytest.raises(SystemExit, match=match):
        transcribe.main(["--long", "--random-init", "a.wav"] + extra)
    assert not (tmp_path / "out.txt").exists()


def test_cli_channel_flags_need_long(monkeypatch):
    monkeypatch.setattr(transcribe, "build_model", lambda args: (_ for _ in ()).throw(AssertionError("a model was built")))
    for flag in (["--channels", "split"], ["--channels", "mix"], ["--crosstalk-db", "12"], ["--kaldi-text", "t"]):
        with pytest.raises(SystemExit, match=f"{flag[0]} needs --long"):
            transcribe.main(["--random-init", "--synthetic", "2"] + flag)
    with pytest.raises(SystemExit):  # argparse: not one of mix, split
        transcribe.main(["--long", "--random-init", "a.wav", "--channels", "both"])
