"""-m gpu: long-form segmentation (csrc/segment.hip, segment.py, transcribe_long, transcribe --long).

1. frame energies against numpy float64
2. segments bit for bit against tests/segment_ref.py, both fed the same fp32 db array
3. transcribe_long end to end on 2-layer random weights: its segments are generate_many / align_many on the same one-clip batches
4. the CLI

The recording of 3. and 4. (tests/segment_cases.py): 0.5 s of 1e-4 noise, four 2 s bursts (0.1-amplitude 440 Hz tone + 0.01 noise)
separated by 1 s of the same noise, 0.5 s of noise; max_segment_s = 3.5.  A frame sees 400 samples at a hop of 320, so a burst that ends at sample 40 000 leaves
frames 125 .. 173 silent (frame 174 already holds 80 samples of the next burst): the pauses are the runs [125, 174), [275, 324) and
[425, 474), whose centres (a + b) / 2 in integer arithmetic are 149, 299 and 449 -- the 150, 300, 450 one gets from the sample
positions alone, less the half frame that the 80-sample overlap takes from each pause.  thr = -60 dB (noise -80 dB + 10 is below the
floor).  tests/test_segment_ref.py confirms this on the host."""
import importlib
import json
import wave as wave_module

import numpy as np
import pytest
import torch

import decoder_pool_cases as pc
import segment_ref as R
from segment_cases import BURSTS, CONTRACT_F, CONTRACT_PARAMS, EDGE, LONG, SMALL, contract_inputs, recording

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gu():
    return importlib.import_module("gpu_util")


@pytest.fixture(scope="module")
def seg():
    return importlib.import_module("loco-asr_amd.segment")


# ---- 1. energy -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [400, 719, 720, 48123])
def test_frame_energy_against_float64(gu, seg, n):
    """Bar 1e-3 dB absolute, derived: fp32 accumulation of 400 squares is at most about 1e-4 dB, log10f adds a few ulp of 120; ten times
    their sum."""
    rng = np.random.default_rng(n)
    signals = {"zeros": np.zeros(n, np.float32), "full_scale": np.where(rng.integers(2, size=n) == 1, 1.0, -1.0).astype(np.float32),
               "noise_1e-4": (1e-4 * rng.standard_normal(n)).astype(np.float32)}
    for name, x in signals.items():
        got = seg.frame_energy_db(gu.dev(x)).cpu().numpy()
        ref = R.frame_energy_db(x)
        assert got.shape == ref.shape == ((n - 80) // 320,) and got.dtype == np.float32
        err = float(np.abs(got.astype(np.float64) - ref).max())
        print(f"frame_energy n={n} {name}: max abs error {err:.3e} dB")
        assert err <= 1e-3, (name, err)
        if name == "zeros":
            assert (got == np.float32(-120.0)).all()
        if name == "full_scale":
            assert np.abs(got).max() <= 1e-3  # mean(x^2) = 1 -> 0 dB


def test_frame_energy_is_position_independent(gu, seg):
    """A frame's value is a function of its 400 samples alone: the same samples at another frame index give the same bits."""
    rng = np.random.default_rng(7)
    x = (0.05 * rng.standard_normal(320 * 9 + 80)).astype(np.float32)
    a = seg.frame_energy_db(gu.dev(x)).cpu()
    b = seg.frame_energy_db(gu.dev(x[320 * 3:])).cpu()
    assert torch.equal(a[3:], b)


# ---- 2. segments -----------------------------------------------------------------------------------------------------------------------
def device_segments(gu, seg, db, params, max_segments=None):
    p = seg.resolve_params(None, **params)
    start, end, count, thr = seg.segments_from_db(gu.dev(np.asarray(db, np.float32)), p, max_segments)
    k = int(count.item())
    return list(zip(start[:max(k, 0)].cpu().tolist(), end[:max(k, 0)].cpu().tolist())), float(thr.item()), k


def assert_same(gu, seg, db, params):
    """Device == restatement with trim off and on; returns the trimmed segments."""
    for trim in (False, True):
        full = dict(params, trim=trim)
        want, thr = R.segments(np.asarray(db, np.float32), **full)
        got, got_thr, k = device_segments(gu, seg, db, full)
        assert k == len(want) and got == want, (full, got[:8], want[:8])
        assert np.float32(got_thr) == thr, (got_thr, thr)
    return want


@pytest.mark.parametrize("name", sorted(EDGE))
def test_segments_edge_cases_bit_exact(gu, seg, name):
    db, params = EDGE[name]
    want = assert_same(gu, seg, db, params)
    expected_empty = name in ("one_silent_frame", "one_frame_shorter_than_min_speech", "all_silence", "all_nan")
    assert (len(want) == 0) == expected_empty


@pytest.mark.parametrize("seed", range(20))
def test_segments_telegraph_bit_exact(gu, seg, seed):
    F = 4000 - 173 * seed
    params = dict(max_segment_s=1.5 + 0.5 * (seed % 6), min_segment_s=0.2 + 0.1 * (seed % 4), min_silence_s=0.06 + 0.06 * (seed % 5),
                  min_speech_s=0.04 * (seed % 4), pad_s=0.04 * (seed % 6)) if seed % 5 else {}
    db = R.telegraph(seed, F, mean_speech=20 + 11 * (seed % 7), mean_silence=4 + 5 * (seed % 5), jitter_db=3.0 + seed % 4)
    want = assert_same(gu, seg, db, params)
    assert len(want) >= 2


def test_segments_of_an_hour(gu, seg):
    """F = 180 000 (60 minutes), for sizes only: more frames than threads by far, thousands of runs, hundreds of cuts."""
    want = assert_same(gu, seg, R.telegraph(99, 180000), {})
    assert len(want) > 200


def test_overflow_is_reported_not_written(gu, seg):
    db = EDGE["all_speech_forced_cuts"][0]
    want, _ = R.segments(db, **SMALL)
    assert len(want) > 2
    p = seg.resolve_params(None, **SMALL)
    lib, C = gu.lib(), importlib.import_module("ctypes")
    d = gu.dev(db)
    start = torch.full((8,), -777, dtype=torch.int32, device="cuda")
    end = torch.full((8,), -778, dtype=torch.int32, device="cuda")
    count = torch.full((2,), -779, dtype=torch.int32, device="cuda")
    thr = torch.zeros(2, device="cuda")
    ws = torch.empty(int(lib.loco_vad_workspace_bytes(len(db))), dtype=torch.uint8, device="cuda")
    gu.check(lib.loco_op_vad_segments(gu.ptr(d), len(db), C.byref(p.to_c()), gu.ptr(start), gu.ptr(end), 2, gu.ptr(count), gu.ptr(thr), gu.ptr(ws),
                                      ws.numel(), gu.stream()), "loco_op_vad_segments")
    assert count.cpu().tolist() == [-len(want), -779]
    assert start.cpu().tolist() == [want[0][0], want[1][0]] + [-777] * 6
    assert end.cpu().tolist() == [want[0][1], want[1][1]] + [-778] * 6


GUARD = 0xA5


def guarded(n, dtype, words):
    """A device buffer of n elements followed by ``words`` guard elements, every byte GUARD; (the buffer, the bytes from the guard on)."""
    size = torch.empty(0, dtype=dtype).element_size()
    raw = torch.full(((n + words) * size,), GUARD, dtype=torch.uint8, device="cuda")
    return raw, raw[n * size:]


@pytest.mark.parametrize("F", CONTRACT_F)
def test_mono_entry_workspace_and_output_contract(gu, seg, F):
    """loco_op_vad_segments given exactly loco_vad_workspace_bytes(F) bytes: the bits of the restatement, and not a byte written behind
    the workspace (256 guard bytes), seg_start / seg_end [max_segments] (8 guard words each), count and threshold_db (one each)."""
    lib, C = gu.lib(), importlib.import_module("ctypes")
    p = seg.resolve_params(None, **CONTRACT_PARAMS)
    maxf, minf = p.frames()[:2]
    max_segments = F // min(minf + 1, maxf // 2) + 1
    ws_bytes = int(lib.loco_vad_workspace_bytes(F))
    assert ws_bytes >= 9 * F + 4 and (F != 601 or ws_bytes % 16 != 0)
    for name, db in contract_inputs(F).items():
        want, want_thr = R.segments(db, **CONTRACT_PARAMS)
        assert len(want) <= max_segments
        if F >= 601:
            assert {"silent": len(want) == 0 and want_thr == np.inf, "all_speech": want_thr == -np.inf, "telegraph": len(want) >= 2}[name]
        d = gu.dev(db)
        start, start_g = guarded(max_segments, torch.int32, 8)
        end, end_g = guarded(max_segments, torch.int32, 8)
        count, count_g = guarded(1, torch.int32, 1)
        thr, thr_g = guarded(1, torch.float32, 1)
        ws, ws_g = guarded(ws_bytes, torch.uint8, 256)
        gu.check(lib.loco_op_vad_segments(gu.ptr(d), F, C.byref(p.to_c()), gu.ptr(start), gu.ptr(end), max_segments, gu.ptr(count), gu.ptr(thr),
                                          gu.ptr(ws), ws_bytes, gu.stream()), "loco_op_vad_segments")
        k = len(want)
        assert count.view(torch.int32)[:1].cpu().tolist() == [k], (name, F)
        assert thr.view(torch.float32)[:1].cpu().numpy().view(np.uint32)[0] == np.float32(want_thr).view(np.uint32), (name, F)
        got = list(zip(start.view(torch.int32)[:k].cpu().tolist(), end.view(torch.int32)[:k].cpu().tolist()))
        assert got == want, (name, F, got[:8], want[:8])
        for what, g in (("seg_start", start_g), ("seg_end", end_g), ("count", count_g), ("threshold_db", thr_g), ("workspace", ws_g)):
            assert bool((g == GUARD).all()), (name, F, what)


@pytest.mark.parametrize("n", [400, 719, 48123])
def test_mono_energy_entry_is_row_0_of_the_channel_entry(gu, n):
    """loco_op_frame_energy_db writes db[F] and nothing behind it, the bits of loco_op_frame_energy_db_channels with C = 1 on the same
    samples at a row stride larger than n."""
    lib = gu.lib()
    F = (n - 80) // 320
    rng = np.random.default_rng(n)
    x = gu.dev((0.05 * rng.standard_normal(n)).astype(np.float32))
    wide = torch.full((1, n + 37), float("nan"), device="cuda")
    wide[0, :n] = x
    db, db_g = guarded(F, torch.float32, 64)
    gu.check(lib.loco_op_frame_energy_db(gu.ptr(x), n, gu.ptr(db), gu.stream()), "loco_op_frame_energy_db")
    row, row_g = guarded(F, torch.float32, 64)
    gu.check(lib.loco_op_frame_energy_db_channels(gu.ptr(wide), 1, n, n + 37, gu.ptr(row), gu.stream()), "loco_op_frame_energy_db_channels")
    size = 4 * F
    assert torch.equal(db[:size], row[:size]) and bool(torch.isfinite(db[:size].view(torch.float32)).all())
    assert bool((db_g == GUARD).all()) and bool((row_g == GUARD).all())


# ---- 3. end to end ---------------------------------------------------------------------------------------------------------------------
_cache = {}


def small_model(gu):
    if "model" not in _cache:
        la = gu.la
        pre, enc = la.synth.split_state_dict(la.synth.encoder_state_dict(0, pc.ENC_LAYERS))
        dec, post = la.synth.split_decoder_state_dict(la.synth.decoder_state_dict(pc.DEC_SEED, layers=pc.DEC_LAYERS))
        t = lambda d: {k: torch.from_numpy(v) for k, v in d.items()}  # noqa: E731
        _cache["model"] = la.SpeechT5ForSpeechToTextMI355X.from_state_dicts(t(pre), t(enc), layers=pc.ENC_LAYERS, decoder_state_dict=t(dec),
                                                                            postnet_state_dict=t(post)).to("cuda")
    return _cache["model"]


def test_transcribe_long_end_to_end(gu, seg):
    model, x = small_model(gu), recording()
    wave = gu.dev(x)
    got = seg.segment(wave, **LONG)
    want, thr = R.segments(seg.frame_energy_db(wave).cpu().numpy(), **LONG)
    assert got.count == 4 and got.threshold_db == -60.0 == float(thr)
    assert list(zip(got.start_frames.cpu().tolist(), got.end_frames.cpu().tolist())) == want == [(14, 135), (164, 285), (314, 435), (464, 585)]
    bounds = list(zip(got.start_samples.cpu().tolist(), got.end_samples.cpu().tolist()))
    assert bounds == [(320 * a, 320 * b + 80) for a, b in want]
    for k, (s, e) in enumerate(bounds):  # exactly one burst's samples: all of burst k, none of another
        assert s <= BURSTS[k][0] and BURSTS[k][1] <= e
        assert all(b <= s or e <= a for j, (a, b) in enumerate(BURSTS) if j != k)

    res = model.transcribe_long(wave, vad=LONG, max_length=12, slots=64, pack=8, return_scores=True, timestamps=True)
    assert len(res.segments) == 4 and res.duration_s == 12.0 and res.threshold_db == -60.0
    batches = [dict(input_values=wave[s:e][None], attention_mask=torch.ones((1, e - s), dtype=torch.int32, device="cuda")) for s, e in bounds]
    ids, scores = model.generate_many(batches, max_length=12, slots=64, pack=8, return_scores=True)
    als = model.align_many(batches, [r[1:] for r in ids], pack=8)
    for k, sg in enumerate(res.segments):
        assert (sg.start_s, sg.end_s) == (bounds[k][0] / 16000, bounds[k][1] / 16000)
        assert torch.equal(sg.ids, ids[k]) and 2 <= sg.ids.shape[0] <= 12 and sg.ids[0] == 2
        assert torch.equal(sg.token_logprobs, scores[k]) and sg.token_logprobs.shape[0] == sg.ids.shape[0] - 1
        assert sg.logprob == float(scores[k].double().sum()) and sg.avg_logprob == sg.logprob / (sg.ids.shape[0] - 1)
        times = torch.stack([als[k].start_times, als[k].end_times], dim=1).cpu() + sg.start_s
        assert torch.equal(sg.token_times, times) and sg.token_times.shape == (sg.ids.shape[0] - 1, 2)
        assert float(sg.token_times.min()) >= sg.start_s - 1e-5 and float(sg.token_times.max()) <= sg.end_s + 1e-5  # fp32 sums
    one = model.transcribe_long(wave, vad=LONG, max_length=12, slots=1, pack=8, return_scores=True, timestamps=True)
    assert len(one.segments) == 4
    for a, b in zip(one.segments, res.segments):
        assert (a.start_s, a.end_s) == (b.start_s, b.end_s) and torch.equal(a.ids, b.ids)
        assert torch.equal(a.token_logprobs, b.token_logprobs) and torch.equal(a.token_times, b.token_times)


def test_transcribe_long_of_silence_and_of_one_short_clip(gu):
    model = small_model(gu)
    res = model.transcribe_long(torch.zeros(16000, device="cuda"), max_length=4)
    assert res.segments == [] and res.duration_s == 1.0 and res.threshold_db == float("inf")
    res = model.transcribe_long(gu.dev(recording()[8000:12800]), max_length=4)  # 0.3 s inside a burst: one segment, all 14 frames
    assert len(res.segments) == 1 and (res.segments[0].start_s, res.segments[0].end_s) == (0.0, 0.285) and res.threshold_db == float("-inf")


# ---- 4. the CLI ------------------------------------------------------------------------------------------------------------------------
def test_transcribe_long_cli(gu, tmp_path, monkeypatch):
    tr = importlib.import_module("loco-asr_amd.transcribe")
    model = small_model(gu)
    monkeypatch.setattr(tr, "build_model", lambda args: model)  # the CLI's own path from the arguments on; 2-layer weights keep it quick
    path = tmp_path / "call.wav"
    with wave_module.open(str(path), "wb") as fh:
        fh.setnchannels(1)
        fh.setsampwidth(2)
        fh.setframerate(16000)
        fh.writeframes(np.round(recording() * 32767.0).astype("<i2").tobytes())
    out = tmp_path / "long.jsonl"
    assert tr.main(["--long", "--random-init", "--scores", "--timestamps", "--max-segment-s", "3.5", "--max-length", "12", str(path),
                    "--out", str(out)]) == 0
    lines = out.read_text().splitlines()
    assert len(lines) == 1
    rec = json.loads(lines[0])
    assert set(rec) == {"id", "duration_s", "threshold_db", "segments"}  # no tokenizer on disk: no "text"
    assert rec["id"] == "call" and rec["duration_s"] == 12.0 and rec["threshold_db"] == -60.0 and len(rec["segments"]) == 4
    prev_end = 0.0
    for k, sg in enumerate(rec["segments"]):
        assert set(sg) == {"start_s", "end_s", "token_ids", "logprob", "avg_logprob", "token_times"}
        assert prev_end <= sg["start_s"] < sg["end_s"] <= 12.0
        assert sg["start_s"] <= BURSTS[k][0] / 16000 and BURSTS[k][1] / 16000 <= sg["end_s"]
        prev_end = sg["end_s"]
        n = len(sg["token_ids"]) - 1
        assert 1 <= n <= 11 and sg["token_ids"][0] == 2 and len(sg["token_times"]) == n
        assert sg["logprob"] < 0 and abs(sg["avg_logprob"] - sg["logprob"] / n) < 1e-12
        t = sg["start_s"]
        for a, b in sg["token_times"]:  # monotone, inside the segment
            assert t - 1e-4 <= a <= b <= sg["end_s"] + 1e-4
            t = a
