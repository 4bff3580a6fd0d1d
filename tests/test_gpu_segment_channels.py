"""-m gpu: per-channel long-form segmentation with the cross-talk gate (csrc/segment.hip, segment.py, transcribe_channels,
transcribe --long --channels split).

1. batched frame energies: every row's bits are the mono operator's
2. segments, thresholds and overlap counts bit for bit against tests/segment_channels_ref.py, both fed the same fp32 db array
3. transcribe_channels end to end on 2-layer random weights: a segment's ids are generate_many on its own slice
4. the CLI: JSON, Kaldi text, and --channels mix = no flag, byte for byte

The call of 3. (tests/segment_channels_cases.py): 24 s, two channels of 1e-4 noise; A speaks in 1 - 3.5 s, 8 - 10.5 s and 15 - 18 s, B in
4.5 - 7 s, 11.5 - 14 s and 16.5 - 19.5 s (synth.clip bursts, -20 dB), and B carries A at -25 dB: where only A speaks B sits at -45 dB, above
its -60 dB threshold and 25 dB below A -- speech to the plain rule, gated at 15 dB."""
import importlib
import json
import re
import wave as wave_module

import numpy as np
import pytest
import torch

import decoder_pool_cases as pc
import segment_channels_ref as CR
from segment_channels_cases import CALL_BURSTS, CALL_LEAK_DB, CALL_SECONDS, CALL_VAD, GATES, GRID_C, GRID_F, GRID_PARAMS, PLANTED, grid_db

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gu():
    return importlib.import_module("gpu_util")


@pytest.fixture(scope="module")
def seg():
    return importlib.import_module("loco-asr_amd.segment")


# ---- 1. energies -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [400, 719, 720, 48123])
def test_channel_energies_are_the_mono_bits(gu, seg, n):
    rng = np.random.default_rng(n)
    x = np.stack([(0.05 * rng.standard_normal(n)).astype(np.float32), (1e-4 * rng.standard_normal(n)).astype(np.float32)])
    x[1, : n // 2] = 0.0  # frames of zeros: exactly -120
    waves = gu.dev(x)
    got = seg.frame_energy_db_channels(waves)
    assert got.shape == (2, (n - 80) // 320) and got.dtype == torch.float32
    for c in range(2):
        assert torch.equal(got[c], seg.frame_energy_db(waves[c]))
    assert (got[1, : max((n // 2 - 400) // 320, 0)] == -120.0).all()
    wide = gu.dev(np.concatenate([x, np.full((2, 37), 9.0, np.float32)], axis=1))[:, :n]  # a row stride beyond n: the tail is never read
    lib = gu.lib()
    out = torch.empty_like(got)
    gu.check(lib.loco_op_frame_energy_db_channels(gu.ptr(wide), 2, n, wide.stride(0), gu.ptr(out), gu.stream()), "loco_op_frame_energy_db_channels")
    assert wide.stride(0) == n + 37 and torch.equal(out, got)


# ---- 2. segments -----------------------------------------------------------------------------------------------------------------------
def device_channels(gu, seg, db, params, gate, max_segments=None):
    p = seg.resolve_params(None, **params)
    start, end, over, count, thr = seg.segments_channels_from_db(gu.dev(np.asarray(db, np.float32)), p, gate, max_segments)
    start, end, over, counts, thrs = start.cpu().tolist(), end.cpu().tolist(), over.cpu().tolist(), count.cpu().tolist(), thr.cpu().numpy()
    segs = [list(zip(start[c][:k], end[c][:k])) for c, k in enumerate(counts)]
    return segs, thrs, [over[c][:k] for c, k in enumerate(counts)], counts


def assert_same(gu, seg, db, params):
    """Device == restatement for every gate, trim off and on: starts, ends, counts, thresholds, overlap."""
    db = np.asarray(db, np.float32)
    for gate in GATES:
        for trim in (False, True):
            full = dict(params, trim=trim)
            want, want_thr, want_over, _ = CR.segments_channels(db, gate, **full)
            got, thr, over, counts = device_channels(gu, seg, db, full, gate)
            assert counts == [len(w) for w in want], (gate, trim, counts)
            assert got == want, (gate, trim)
            assert over == want_over, (gate, trim)
            assert thr.dtype == np.float32 and thr.tobytes() == np.asarray(want_thr, np.float32).tobytes(), (gate, trim, thr, want_thr)
    return want, want_over


@pytest.mark.parametrize("C", GRID_C)
@pytest.mark.parametrize("F", GRID_F)
def test_channels_grid_bit_exact(gu, seg, F, C):
    db = grid_db(F, C)
    want, over = assert_same(gu, seg, db, GRID_PARAMS)
    if F >= 6000:
        assert all(len(w) >= F // 200 for w in want)  # the walk took many steps
        assert C == 1 or sum(map(sum, over)) > 0
    if C == 1:  # one channel: also the mono kernel, exactly
        for trim in (False, True):
            p = seg.resolve_params(None, **dict(GRID_PARAMS, trim=trim))
            d = gu.dev(db)
            s1, e1, k1, t1 = seg.segments_from_db(d[0], p)
            s2, e2, o2, k2, t2 = seg.segments_channels_from_db(d, p, 15.0)
            k = int(k1.item())
            assert k == int(k2.item()) and torch.equal(s1[:k], s2[0, :k]) and torch.equal(e1[:k], e2[0, :k])
            assert t1.cpu().numpy().tobytes() == t2.cpu().numpy().tobytes() and not o2[0, :k].any()


@pytest.mark.parametrize("name", sorted(PLANTED))
def test_channels_planted_cases_bit_exact(gu, seg, name):
    db, params = PLANTED[name]
    assert_same(gu, seg, db, params)
    segs, thrs, _, masks = CR.segments_channels(db, 15.0, **params)
    if name == "silent_channel":
        assert segs[1] == [] and thrs[1] == np.inf and len(segs[0]) > 2 and len(segs[2]) > 2
    if name == "all_speech_channel":
        assert thrs[0] == -np.inf
    if name == "exact_tie":
        assert masks[0][40:60].all() and not masks[0][60:80].any()


def test_channels_overflow_and_no_overlap_output(gu, seg):
    """max_segments too small: the count is minus what is needed, only the first max_segments are written (and counted for overlap);
    overlap = NULL: nothing is written for it."""
    db = grid_db(6000, 2)
    want, _, want_over, _ = CR.segments_channels(db, 15.0, **GRID_PARAMS)
    p = seg.resolve_params(None, **GRID_PARAMS)
    start, end, over, count, _ = seg.segments_channels_from_db(gu.dev(db), p, 15.0, max_segments=3)
    assert count.cpu().tolist() == [-len(w) for w in want] and min(len(w) for w in want) > 3
    for c in range(2):
        assert list(zip(start[c].cpu().tolist(), end[c].cpu().tolist())) == want[c][:3] and over[c].cpu().tolist() == want_over[c][:3]
    start2, end2, none, count2, _ = seg.segments_channels_from_db(gu.dev(db), p, 15.0, overlap=False)
    assert none is None and count2.cpu().tolist() == [len(w) for w in want]


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


def call(gu, rate=16000, seconds=CALL_SECONDS, bursts=CALL_BURSTS):
    """f32 [2, seconds * rate]: the bursts (given in 16 kHz samples) scaled to ``rate``; B carries A at CALL_LEAK_DB."""
    rng = np.random.default_rng(77)
    x = 1e-4 * rng.standard_normal((2, seconds * rate))
    for k, (c, a, b) in enumerate(bursts):
        a, b = a * rate // 16000, b * rate // 16000
        if b <= x.shape[1]:
            x[c, a:b] += gu.la.synth.clip(50 + k, b - a)
    x[1] += 10.0 ** (CALL_LEAK_DB / 20.0) * x[0]
    return x.astype(np.float32)


def a_only_stretches(margin=4000):
    """[a, b) in samples where A's bursts run and none of B's does, widened by 0.25 s: the pad of 0.2 s and the frames at the edges."""
    out = []
    for c, a, b in CALL_BURSTS:
        if c == 0:
            hi = min([b] + [a2 for c2, a2, b2 in CALL_BURSTS if c2 == 1 and a < a2 < b])
            out.append((a - margin, hi + margin))
    return out


def inside_a_only(s, e):
    return any(a <= s and e <= b for a, b in a_only_stretches())


def test_transcribe_channels_end_to_end(gu, seg):
    model, waves = small_model(gu), gu.dev(call(gu))
    got = seg.segment_channels(waves, 15.0, CALL_VAD)
    db = seg.frame_energy_db_channels(waves).cpu().numpy()
    want, thr, over, _ = CR.segments_channels(db, 15.0, **CALL_VAD)
    merged = CR.merged(want, over)
    assert got.counts == [len(w) for w in want] and got.count == len(merged) >= 6 and got.threshold_db == [-60.0, -60.0] == [float(t) for t in thr]
    rows = list(zip(got.start_frames.cpu().tolist(), got.channel.cpu().tolist(), got.end_frames.cpu().tolist(), got.overlap_frames.cpu().tolist()))
    assert rows == merged and rows == sorted(rows)  # (start, channel) order
    bounds = list(zip(got.channel.cpu().tolist(), got.start_samples.cpu().tolist(), got.end_samples.cpu().tolist()))
    assert bounds == [(c, 320 * a, min(320 * b + 80, waves.shape[1])) for a, c, b, _ in merged]
    for k, (c, a, b) in enumerate(CALL_BURSTS):  # every burst lies inside one segment of its own channel
        assert any(ch == c and s <= a and b <= e for ch, s, e in bounds), (k, bounds)
    assert not any(inside_a_only(s, e) for ch, s, e in bounds if ch == 1)
    assert sum(o for _, _, _, o in merged) > 0 and all((o > 0) == (s < 288000 and e > 264000) for (ch, s, e), (_, _, _, o) in zip(bounds, merged))
    plain = seg.segment_channels(waves, float("inf"), CALL_VAD)  # without the gate B repeats A's turns
    assert any(inside_a_only(s, e) for ch, s, e in zip(plain.channel.cpu().tolist(), plain.start_samples.cpu().tolist(), plain.end_samples.cpu().tolist())
               if ch == 1)

    res = model.transcribe_channels(waves, vad=CALL_VAD, max_length=12, slots=64, pack=8, return_scores=True, timestamps=True)
    assert len(res.segments) == len(bounds) and res.duration_s == float(CALL_SECONDS) and res.threshold_db == [-60.0, -60.0]
    batches = [dict(input_values=waves[c, s:e][None], attention_mask=torch.ones((1, e - s), dtype=torch.int32, device="cuda")) for c, s, e in bounds]
    ids, scores = model.generate_many(batches, max_length=12, slots=64, pack=8, return_scores=True)
    als = model.align_many(batches, [r[1:] for r in ids], pack=8)
    for k, sg in enumerate(res.segments):
        assert (sg.channel, sg.start_s, sg.end_s, sg.overlap_s) == (bounds[k][0], bounds[k][1] / 16000, bounds[k][2] / 16000, merged[k][3] / 50)
        assert torch.equal(sg.ids, ids[k]) and 2 <= sg.ids.shape[0] <= 12 and sg.ids[0] == 2
        assert torch.equal(sg.token_logprobs, scores[k]) and sg.logprob == float(scores[k].double().sum())
        times = torch.stack([als[k].start_times, als[k].end_times], dim=1).cpu() + sg.start_s
        assert torch.equal(sg.token_times, times)
    k = next(i for i, (c, _, _) in enumerate(bounds) if c == 1)  # a segment alone gives the same ids: they depend on its samples only
    alone = model.generate_many([batches[k]], max_length=12, slots=1, pack=1)
    assert torch.equal(alone[0], res.segments[k].ids)


def test_transcribe_channels_of_silence_and_of_one_channel(gu):
    model = small_model(gu)
    res = model.transcribe_channels(torch.zeros(2, 16000, device="cuda"), max_length=4)
    assert res.segments == [] and res.duration_s == 1.0 and res.threshold_db == [float("inf")] * 2
    x = gu.dev(call(gu)[:1, :128000])
    one, mono = model.transcribe_channels(x, vad=CALL_VAD, max_length=6), model.transcribe_long(x[0], vad=CALL_VAD, max_length=6)
    assert len(one.segments) == len(mono.segments) >= 1 and one.threshold_db == [mono.threshold_db]
    for a, b in zip(one.segments, mono.segments):
        assert (a.start_s, a.end_s, a.channel, a.overlap_s) == (b.start_s, b.end_s, 0, 0.0) and torch.equal(a.ids, b.ids)


# ---- 4. the CLI ------------------------------------------------------------------------------------------------------------------------
CHARS = "abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ0123456789.,;:!?'\"-()&%$"  # 76 and the space: 77 characters


def char_tokenizer(tmp_path):
    import sentencepiece as spm
    corpus = tmp_path / "corpus.txt"
    corpus.write_text("\n".join(" ".join(CHARS[(k + 3 * j) % len(CHARS):][:5] + CHARS[:k % 7 + 1] for j in range(6)) for k in range(200)) + "\n")
    spm.SentencePieceTrainer.train(input=str(corpus), model_prefix=str(tmp_path / "spm_char"), model_type="char", vocab_size=81, character_coverage=1.0,
                                   bos_id=0, pad_id=1, eos_id=2, unk_id=3, minloglevel=2)
    assert spm.SentencePieceProcessor(model_file=str(tmp_path / "spm_char.model")).get_piece_size() == 81
    return str(tmp_path / "spm_char.model")


UTT = re.compile(r"^call_8k-([AB])-(\d{6})-(\d{6}) \S.*$")


def test_transcribe_channels_cli(gu, tmp_path, monkeypatch):
    tr = importlib.import_module("loco-asr_amd.transcribe")
    model = small_model(gu)
    monkeypatch.setattr(tr, "build_model", lambda args: model)  # the CLI's own path from the arguments on; 2-layer weights keep it quick
    bursts = [(0, 16000, 56000), (1, 72000, 112000), (0, 128000, 176000), (1, 152000, 184000)]
    x = call(gu, rate=8000, seconds=12, bursts=bursts)
    path = tmp_path / "call-8k.wav"
    with wave_module.open(str(path), "wb") as fh:
        fh.setnchannels(2)
        fh.setsampwidth(2)
        fh.setframerate(8000)
        fh.writeframes(np.round(x.T * 32767.0).astype("<i2").tobytes())
    tokenizer = char_tokenizer(tmp_path)
    out, text = tmp_path / "split.jsonl", tmp_path / "text"
    common = ["--long", "--random-init", "--max-segment-s", "4", "--max-length", "12", str(path)]
    assert tr.main(common + ["--channels", "split", "--scores", "--tokenizer", tokenizer, "--kaldi-text", str(text), "--out", str(out)]) == 0
    lines = out.read_text().splitlines()
    assert len(lines) == 1
    rec = json.loads(lines[0])
    assert set(rec) == {"id", "duration_s", "threshold_db", "segments", "text"}
    assert rec["id"] == "call-8k" and rec["duration_s"] == 12.0 and rec["threshold_db"] == [-60.0, -60.0]
    segs = rec["segments"]
    assert len(segs) >= 4 and {sg["channel"] for sg in segs} == {"A", "B"}
    keys = [(sg["start_s"], sg["channel"]) for sg in segs]
    assert keys == sorted(keys)
    for sg in segs:
        assert set(sg) == {"channel", "start_s", "end_s", "overlap_s", "token_ids", "text", "logprob", "avg_logprob"}
        assert 0.0 <= sg["start_s"] < sg["end_s"] <= 12.0 and 0.0 <= sg["overlap_s"] <= sg["end_s"] - sg["start_s"] + 0.02
        assert sg["token_ids"][0] == 2 and 2 <= len(sg["token_ids"]) <= 12 and isinstance(sg["text"], str)
    for c, a, b in bursts:  # every burst inside a segment of its channel; only the last two overlap
        assert any(sg["channel"] == "AB"[c] and sg["start_s"] <= a / 16000 and b / 16000 <= sg["end_s"] for sg in segs)
    assert [sg["overlap_s"] > 0 for sg in segs if sg["end_s"] < 7.5] == [False] * len([sg for sg in segs if sg["end_s"] < 7.5])
    assert any(sg["overlap_s"] > 0 for sg in segs)
    kaldi = text.read_text().splitlines()
    spoken = [sg for sg in segs if sg["text"].strip()]
    assert len(kaldi) == len(spoken) >= 1
    for line, sg in zip(kaldi, spoken):  # the JSON's order; ids by the pattern, centiseconds from the samples
        m = UTT.match(line)
        assert m, line
        assert m.group(1) == sg["channel"] and line.split(" ", 1)[1] == " ".join(sg["text"].split())
        s, e = round(sg["start_s"] * 16000), round(sg["end_s"] * 16000)
        assert (int(m.group(2)), int(m.group(3))) == (s // 160, -(-e // 160))
    lm = importlib.import_module("loco-asr_amd.lm")
    assert {lm.rec_id_of(k) for k in lm.read_key_text(str(text))} == {"call_8k"}

    plain, mix = tmp_path / "plain.jsonl", tmp_path / "mix.jsonl"
    assert tr.main(common + ["--scores", "--out", str(plain)]) == 0
    assert tr.main(common + ["--scores", "--channels", "mix", "--out", str(mix)]) == 0
    assert plain.read_bytes() == mix.read_bytes() and len(plain.read_bytes()) > 0
    mono = json.loads(plain.read_text())
    assert set(mono) == {"id", "duration_s", "threshold_db", "segments"} and "channel" not in mono["segments"][0]
