"""CPU tests of the long-form segmentation's host side: parameters refused by name, the C entry points' answers that need no device
(host memory stands in for the pointers: every refusal comes before any launch), and the flag combinations the CLI refuses."""
import ctypes as C
import importlib

import pytest
import torch

import segment_ref as R

la = importlib.import_module("loco-asr_amd")
seg = importlib.import_module("loco-asr_amd.segment")
transcribe = importlib.import_module("loco-asr_amd.transcribe")
_libmod = importlib.import_module("loco-asr_amd._lib")


def test_defaults_are_the_documented_ones():
    lib = _libmod.load()
    p = _libmod.LocoVadParams()
    lib.loco_vad_default_params(C.byref(p))
    assert p.struct_size == C.sizeof(_libmod.LocoVadParams) and p.trim == 1
    got = {name: getattr(p, name) for name, _ in _libmod.LocoVadParams._fields_[2:]}
    assert got == {k: v for k, v in R.DEFAULTS.items() if k != "trim"}
    assert got == {k: getattr(seg.VadParams(), k) for k in got}
    assert seg.VadParams().frames() == (1000, 50, 15, 5, 10)
    # seconds -> frames: round(s * 50), ties to even, the same in the library and in the numpy restatement
    for s in (0.03, 0.25, 0.27, 0.29, 0.3, 0.31, 0.33, 0.35, 1.0, 2.5):
        assert seg.VadParams(min_silence_s=s, min_speech_s=s, pad_s=s).frames()[2:] == (R.to_frames(s),) * 3


@pytest.mark.parametrize("field,value,match", [
    ("min_segment_s", 20.0, "min_segment_s = 20 is not below max_segment_s = 20"),
    ("min_segment_s", 25.0, "min_segment_s = 25 is not below max_segment_s"),
    ("min_segment_s", 0.0, "min_segment_s = 0 is below one frame"),
    ("max_segment_s", 30.5, "max_segment_s = 30.5 exceeds 30 s"),
    ("max_segment_s", 0.02, "max_segment_s = 0.02 is below 2 frames"),
    ("max_segment_s", float("nan"), "max_segment_s = nan is not finite"),
    ("min_silence_s", 0.0, "min_silence_s = 0 is below one frame"),
    ("min_speech_s", -0.1, "min_speech_s = -0.1 is outside"),
    ("pad_s", -1.0, "pad_s = -1 is outside"),
    ("noise_quantile", 0.0, r"noise_quantile = 0 is outside \(0, 1\)"),
    ("noise_quantile", 1.0, r"noise_quantile = 1 is outside \(0, 1\)"),
    ("peak_quantile", 1.0, r"peak_quantile = 1 is outside \(0, 1\)"),
    ("peak_quantile", 0.05, "noise_quantile = 0.1 is not below peak_quantile = 0.05"),
    ("margin_db", -1.0, "margin_db = -1 is negative"),
    ("min_dynamic_db", -3.0, "min_dynamic_db = -3 is negative"),
    ("abs_floor_db", float("inf"), "abs_floor_db = inf is not finite"),
])
def test_refused_parameters_raise_by_name(field, value, match):
    with pytest.raises(ValueError, match=match):
        seg.resolve_params(None, **{field: value})
    with pytest.raises(ValueError, match=match):
        seg.resolve_params({field: value})


def test_unknown_parameters_and_cpu_tensors():
    with pytest.raises(TypeError, match="unknown segmentation parameter 'max_segment'"):
        seg.resolve_params(None, max_segment=3)
    assert seg.resolve_params(seg.VadParams(pad_s=0.1), trim=False) == seg.VadParams(pad_s=0.1, trim=False)
    for fn in (seg.frame_energy_db, seg.segment):
        with pytest.raises(RuntimeError, match="no CPU path"):
            fn(torch.zeros(1000))
    with pytest.raises(ValueError, match="min_segment_s"):  # parameters are checked before the tensor is looked at
        seg.segment(torch.zeros(1000), min_segment_s=30)
    model = la.SpeechT5ForSpeechToTextMI355X(layers=1, decoder_layers=1)
    with pytest.raises(ValueError, match="max_segment_s = 31 exceeds"):
        model.transcribe_long(torch.zeros(1000), vad=dict(max_segment_s=31))
    with pytest.raises(ValueError, match="max_length 451 exceeds"):
        model.transcribe_long(torch.zeros(1000), max_length=451)
    with pytest.raises(RuntimeError, match="no CPU path"):
        model.transcribe_long(torch.zeros(1000))
    with pytest.raises(RuntimeError, match="needs the decoder"):
        la.SpeechT5ForSpeechToTextMI355X(layers=1).transcribe_long(torch.zeros(1000))


def test_cabi_refusals_come_before_any_launch():
    lib = _libmod.load()
    err = lambda: lib.loco_last_error().decode()  # noqa: E731
    wav, db = (C.c_float * 1000)(), (C.c_float * 8)()
    p = _libmod.LocoVadParams()
    lib.loco_vad_default_params(C.byref(p))
    start, end, count, thr = (C.c_int32 * 4)(), (C.c_int32 * 4)(), (C.c_int32 * 1)(), (C.c_float * 1)()
    ws = (C.c_uint8 * 4096)()
    assert lib.loco_vad_workspace_bytes(8) >= 8 + 4 * 9 + 4 * 8 and lib.loco_vad_workspace_bytes(8) <= 4096
    assert lib.loco_vad_workspace_bytes(0) == 0 and lib.loco_vad_workspace_bytes(-5) == 0 and lib.loco_vad_workspace_bytes(2 ** 24 + 1) == 0
    assert lib.loco_vad_workspace_bytes(180000) < 10 * 180000

    assert lib.loco_op_frame_energy_db(None, 1000, db, None) == -1 and "loco_op_frame_energy_db: null" in err()
    assert lib.loco_op_frame_energy_db(wav, 1000, None, None) == -1 and "null" in err()
    assert lib.loco_op_frame_energy_db(wav, 399, db, None) == -1 and "n = 399 samples is shorter than one frame (400)" in err()
    assert lib.loco_op_frame_energy_db(wav, 0, db, None) == -1 and "shorter than one frame" in err()

    good = [db, 8, C.byref(p), start, end, 4, count, thr, ws, 4096, None]
    for i in (0, 2, 3, 4, 6, 7, 8):
        args = list(good)
        args[i] = None
        assert lib.loco_op_vad_segments(*args) == -1 and "loco_op_vad_segments: null argument" in err(), i
    for F in (0, -1, 2 ** 24 + 1):
        args = list(good)
        args[1] = F
        assert lib.loco_op_vad_segments(*args) == -1 and f"F = {F} is outside" in err()
    for k in (0, -2):
        args = list(good)
        args[5] = k
        assert lib.loco_op_vad_segments(*args) == -1 and f"max_segments = {k} must be >= 1" in err()
    args = list(good)
    args[9] = lib.loco_vad_workspace_bytes(8) - 1
    assert lib.loco_op_vad_segments(*args) == -1 and f"workspace {args[9]} < {args[9] + 1} bytes" in err()
    bad = _libmod.LocoVadParams()
    lib.loco_vad_default_params(C.byref(bad))
    bad.min_segment_s = 20.0
    args = list(good)
    args[2] = C.byref(bad)
    assert lib.loco_op_vad_segments(*args) == -1 and "min_segment_s = 20 is not below max_segment_s = 20" in err()
    bad.struct_size = 8
    assert lib.loco_op_vad_segments(*args) == -1 and "struct_size = 8" in err()
    assert lib.loco_vad_frames(None, (C.c_int32 * 5)()) == -1 and lib.loco_vad_frames(C.byref(p), None) == -1


@pytest.mark.parametrize("extra,match", [
    (["--split", "devel"], "--long does not go with --split"),
    (["--synthetic", "3"], "--long does not go with --synthetic"),
    (["--nbest", "2", "--slots", "4"], "--long does not go with --nbest"),
    (["--batch-size", "4"], "--long does not go with --batch-size"),
    (["--max-segment-s", "45"], "max_segment_s = 45 exceeds"),
    (["--min-silence-s", "0"], "min_silence_s = 0 is below one frame"),
    (["--vad-margin-db", "-2"], "margin_db = -2 is negative"),
    (["--slots", "65"], "--slots must be 1 .. 64"),
])
def test_cli_refuses_before_a_model_is_built(extra, match, monkeypatch):
    def no_model(args):
        raise AssertionError("a model was built")
    monkeypatch.setattr(transcribe, "build_model", no_model)
    with pytest.raises(SystemExit, match=match):
        transcribe.main(["--long", "--random-init", "a.wav"] + extra)


def test_cli_long_flags_need_long_and_files(monkeypatch):
    monkeypatch.setattr(transcribe, "build_model", lambda args: (_ for _ in ()).throw(AssertionError("a model was built")))
    with pytest.raises(SystemExit, match="--long needs audio FILES"):
        transcribe.main(["--long", "--random-init"])
    for flag in (["--max-segment-s", "5"], ["--min-silence-s", "0.2"], ["--vad-margin-db", "6"], ["--no-trim"]):
        with pytest.raises(SystemExit, match=f"{flag[0]} needs --long"):
            transcribe.main(["--random-init", "--synthetic", "2"] + flag)
