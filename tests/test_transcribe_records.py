"""transcribe.py above the model, on the host alone: the records (key order is part of the bytes), the writer's padding, the regrouping
of a window's Lines into reference batches, the flag checks from parsed arguments, and the recording-id rule score_errors shares."""
import importlib
import io
import json
import types

import pytest
import torch

tr = importlib.import_module("loco-asr_amd.transcribe")
se = importlib.import_module("loco-asr_amd.score_errors")


class Tok:
    """decode: the ids as letters -- 3 is "a"."""

    def decode(self, ids):
        return "".join(chr(ord("a") + i - 3) for i in ids)


ERR = {"cer": 0.5, "sub": 1, "del": 0, "ins": 0, "ref_len": 2}


def dumps(line, tok=None, width=0):
    return json.dumps(tr.utterance_record(line, tok, width))


def test_token_fields_in_the_order_written():
    f = tr.token_fields
    assert json.dumps(f(None, [2, 3, 2])) == '{"token_ids": [2, 3, 2]}'
    assert json.dumps(f(Tok(), [2, 3, 4, 2, 1])) == '{"token_ids": [2, 3, 4, 2, 1], "text": "ab"}'
    assert json.dumps(f(None, [2, 3, 2], -1.5, -0.75)) == '{"token_ids": [2, 3, 2], "logprob": -1.5, "avg_logprob": -0.75}'
    assert json.dumps(f(None, [2, 3, 2], times=[[0.0, 0.1], [0.1, 0.2]])) == '{"token_ids": [2, 3, 2], "token_times": [[0.0, 0.1], [0.1, 0.2]]}'
    assert json.dumps(f(Tok(), [2, 3, 2], -1.5, -0.5, [[0.0, 0.1]])) == \
        '{"token_ids": [2, 3, 2], "text": "a", "logprob": -1.5, "avg_logprob": -0.5, "token_times": [[0.0, 0.1]]}'  # avg: the caller's own


def test_utterance_record_for_every_combination_of_optional_fields():
    L = tr.Line
    assert dumps(L("u", [2, 3, 2])) == '{"id": "u", "token_ids": [2, 3, 2]}'
    assert dumps(L("u", [2, 3, 2]), Tok()) == '{"id": "u", "token_ids": [2, 3, 2], "text": "a"}'
    assert dumps(L("u", [2, 3, 4, 2], logprob=(-1.5, 3))) == '{"id": "u", "token_ids": [2, 3, 4, 2], "logprob": -1.5, "avg_logprob": -0.5}'
    assert dumps(L("u", [2, 3, 2], times=[[0.0, 0.02], [0.02, 0.04]])) == '{"id": "u", "token_ids": [2, 3, 2], "token_times": [[0.0, 0.02], [0.02, 0.04]]}'
    assert dumps(L("u", [2, 3, 2], errors=ERR)) == '{"id": "u", "token_ids": [2, 3, 2], "errors": ' + json.dumps(ERR) + '}'
    nbest = tr.nbest_records([torch.tensor([2, 3, 2])], [-0.5], None)
    assert dumps(L("u", [2, 3, 2], nbest=nbest)) == '{"id": "u", "token_ids": [2, 3, 2], "nbest": [{"ids": [2, 3, 2], "logprob": -0.5, "avg_logprob": -0.25}]}'
    full = L("u", [2, 3, 2], (-1.0, 2), [[0.0, 0.02], [0.02, 0.04]], tr.nbest_records([torch.tensor([2, 3, 2])], [-1.0], Tok(), [0.25]), ERR)
    assert dumps(full, Tok(), 4) == ('{"id": "u", "token_ids": [2, 3, 2, 1], "text": "a", "logprob": -1.0, "avg_logprob": -0.5, '
                                     '"token_times": [[0.0, 0.02], [0.02, 0.04]], "nbest": [{"ids": [2, 3, 2], "logprob": -1.0, "avg_logprob": -0.5, '
                                     '"text": "a", "mbr_risk": 0.25}], "errors": ' + json.dumps(ERR) + '}')


def test_nbest_records_sort_by_logprob_and_break_ties_by_hypothesis_index():
    hyps = [torch.tensor(r) for r in ([2, 3, 2], [2, 4, 5, 2], [2, 6, 2], [2, 7, 8, 9])]
    recs = tr.nbest_records(hyps, [-2.0, -1.0, -2.0, -1.0], None)
    assert [r["ids"][1] for r in recs] == [4, 7, 3, 6]  # -1.0 before -2.0; within a tie hypothesis 1 before 3, 0 before 2
    assert json.dumps(recs[0]) == '{"ids": [2, 4, 5, 2], "logprob": -1.0, "avg_logprob": ' + repr(-1.0 / 3) + '}'
    with_risk = tr.nbest_records(hyps, [-2.0, -1.0, -2.0, -1.0], Tok(), [0.0, 1.0, 2.0, 3.0])
    assert [list(r) for r in with_risk] == [["ids", "logprob", "avg_logprob", "text", "mbr_risk"]] * 4
    assert [r["mbr_risk"] for r in with_risk] == [1.0, 3.0, 0.0, 2.0] and with_risk[1]["text"] == "efg"  # a risk stays with its hypothesis


def segment(channel=1):
    return types.SimpleNamespace(ids=torch.tensor([2, 3, 4, 2]), start_s=1.23456789, end_s=2.5, channel=channel, overlap_s=0.33339,
                                 logprob=-1.5, avg_logprob=-0.4, token_times=torch.tensor([[1.25, 1.5], [1.5, 1.75], [1.75, 2.0]]))


def test_segment_and_recording_records():
    assert json.dumps(tr.segment_record(segment(), None, False, False, False)) == '{"start_s": 1.2346, "end_s": 2.5, "token_ids": [2, 3, 4, 2]}'
    assert json.dumps(tr.segment_record(segment(), Tok(), True, True, True)) == (
        '{"channel": "B", "start_s": 1.2346, "end_s": 2.5, "overlap_s": 0.3334, "token_ids": [2, 3, 4, 2], "text": "ab", "logprob": -1.5, '
        '"avg_logprob": -0.4, "token_times": [[1.25, 1.5], [1.5, 1.75], [1.75, 2.0]]}')  # the average is the segment's own, not sum / n
    assert json.dumps(tr.segment_record(segment(), None, False, True, False)) == \
        '{"start_s": 1.2346, "end_s": 2.5, "token_ids": [2, 3, 4, 2], "logprob": -1.5, "avg_logprob": -0.4}'
    res = types.SimpleNamespace(segments=[segment(0), segment(1)], duration_s=9.87654321, threshold_db=float("-inf"))
    one = '{"start_s": 1.2346, "end_s": 2.5, "token_ids": [2, 3, 4, 2]}'
    assert json.dumps(tr.recording_record("call", res, None, False, False, False)) == \
        '{"id": "call", "duration_s": 9.8765, "threshold_db": null, "segments": [' + one + ", " + one + "]}"
    res.threshold_db = [-41.5, float("inf")]
    rec = tr.recording_record("call", res, Tok(), True, False, False)
    assert list(rec) == ["id", "duration_s", "threshold_db", "segments", "text"] and rec["threshold_db"] == [-41.5, None]
    assert rec["text"] == "ab ab" and [list(s) for s in rec["segments"]] == [["channel", "start_s", "end_s", "overlap_s", "token_ids", "text"]] * 2
    assert [s["channel"] for s in rec["segments"]] == ["A", "B"]


def test_the_writer_pads_a_batch_to_its_longest_row():
    fh = io.StringIO()
    tr.write_lines(fh, [tr.Line("a", [2, 3, 2], logprob=(-3.0, 2)), tr.Line("b", [2, 3, 4, 5, 2], logprob=(-3.0, 4)), tr.Line("c", [2, 2])], None)
    tr.write_lines(fh, [tr.Line("d", [2, 2])], None)  # the next batch has its own width
    assert fh.getvalue().splitlines() == ['{"id": "a", "token_ids": [2, 3, 2, 1, 1], "logprob": -3.0, "avg_logprob": -1.5}',  # 2 generated, not 4
                                          '{"id": "b", "token_ids": [2, 3, 4, 5, 2], "logprob": -3.0, "avg_logprob": -0.75}',
                                          '{"id": "c", "token_ids": [2, 2, 1, 1, 1]}', '{"id": "d", "token_ids": [2, 2]}']


def test_a_windows_lines_regroup_into_reference_batches_with_their_own_fields():
    def line(u):
        return tr.Line(f"u{u}", [2] + [3 + u] * (u + 1) + [2], (-float(u), u + 2), [[u, u + 0.5]], [{"ids": [2, u, 2]}], {"sub": u})
    batches = tr.batches_of([line(u) for u in range(5)], 2)
    assert [[l.uid for l in b] for b in batches] == [["u0", "u1"], ["u2", "u3"], ["u4"]]
    assert [l for b in batches for l in b] == [line(u) for u in range(5)]  # a shifted field would put another uid's value here
    assert tr.batches_of([], 2) == [] and [len(b) for b in tr.batches_of([line(0)] * 4, 2)] == [2, 2]


def test_span_sums_is_fsum_per_tensor():
    spans = [torch.tensor([0.1, 0.2, 0.3]), torch.tensor([]), torch.tensor([1e8, 1.0, -1e8])]
    assert tr.span_sums(spans) == [__import__("math").fsum(t.tolist()) for t in spans] and tr.span_sums(spans)[2] == 1.0


def parsed(argv):
    ap = tr.build_parser()
    return ap.parse_args(argv), ap


S = ["--random-init", "--synthetic", "2"]


@pytest.mark.parametrize("argv,match", [
    (S + ["--max-segment-s", "5"], "--max-segment-s needs --long"), (S + ["--min-silence-s", "1"], "--min-silence-s needs --long"),
    (S + ["--vad-margin-db", "6"], "--vad-margin-db needs --long"), (S + ["--no-trim"], "--no-trim needs --long"),
    (S + ["--channels", "mix"], "--channels needs --long"), (S + ["--crosstalk-db", "3"], "--crosstalk-db needs --long"),
    (S + ["--kaldi-text", "t"], "--kaldi-text needs --long"), (S + ["--batch-size", "0"], "--batch-size must be >= 1"),
    (S + ["--slots", "-1"], "--slots must be >= 0 and --pack >= 1"), (S + ["--slots", "2", "--pack", "0"], "--slots must be >= 0 and --pack >= 1"),
    (S + ["--nbest", "2"], "--nbest needs --slots"), (S + ["--slots", "2", "--nbest", "-1"], "--nbest must be >= 0"),
    (S + ["--slots", "2", "--nbest", "2", "--top-p", "0"], "--nbest / --temperature / --top-k / --top-p / --seed: top_p"),
])
def test_check_args_refuses_from_the_parsed_arguments_alone(argv, match):
    with pytest.raises(SystemExit, match=match):
        tr.check_args(*parsed(argv))


def test_check_args_argparse_errors_and_the_seed(capsys):
    for argv, text in ((S + ["--select", "mbr"], "--select needs --nbest"), (S + ["--ref", "a", "--ref-ids", "b"], "give --ref or --ref-ids, not both"),
                       (["--long", "a.wav", "--ref", "a", "--ref-ids", "b"], "give --ref or --ref-ids, not both")):
        with pytest.raises(SystemExit) as e:
            tr.check_args(*parsed(argv))
        assert e.value.code == 2 and text in capsys.readouterr().err
    args, ap = parsed(S + ["--slots", "2", "--nbest", "2"])
    tr.check_args(args, ap)
    assert type(args.seed) is int  # drawn once for the corpus
    args, ap = parsed(S + ["--slots", "2", "--nbest", "2", "--seed", "11"])
    tr.check_args(args, ap)
    assert args.seed == 11
    args, ap = parsed(S)
    tr.check_args(args, ap)
    assert args.seed is None and args.slots == 0


L = ["--long", "--random-init", "a.wav"]


@pytest.mark.parametrize("argv,match", [
    (L + ["--split", "devel"], "--long does not go with --split"), (L + ["--synthetic", "3"], "--long does not go with --synthetic"),
    (L + ["--nbest", "2"], "--long does not go with --nbest"), (L + ["--batch-size", "4"], "--long does not go with --batch-size"),
    (L + ["--ref", "r"], "--long does not go with --ref / --ref-ids"), (L + ["--ref-ids", "r"], "--long does not go with --ref / --ref-ids"),
    (["--long", "--random-init"], "--long needs audio FILES"), (L + ["--slots", "65"], "--slots must be 1 .. 64 and --pack >= 1"),
    (L + ["--pack", "0"], "--slots must be 1 .. 64 and --pack >= 1"),
    (L + ["--max-segment-s", "45"], "--max-segment-s / --min-silence-s / --vad-margin-db: .*max_segment_s = 45 exceeds"),
    (L + ["--crosstalk-db", "10"], "--crosstalk-db needs --channels split"), (L + ["--channels", "mix", "--kaldi-text", "t"], "--kaldi-text needs --channels split"),
    (L + ["--channels", "split", "--crosstalk-db", "-3"], "--crosstalk-db: crosstalk_db = -3 is NaN or negative"),
    (L + ["--channels", "split", "--crosstalk-db", "nan"], "--crosstalk-db: crosstalk_db = nan is NaN or negative"),
])
def test_check_long_args_refuses_from_the_parsed_arguments_alone(argv, match):
    args, ap = parsed(argv)
    tr.check_args(args, ap)  # the checks every command line gets pass
    with pytest.raises(SystemExit, match=match):
        tr.check_long_args(args, ap)


def test_check_long_args_resolves_the_defaults():
    args, ap = parsed(L + ["--channels", "split"])
    vad = tr.check_long_args(args, ap)
    assert args.slots == 64 and args.crosstalk_db == 15.0 and type(args.crosstalk_db) is float and vad is not None
    args, ap = parsed(L + ["--slots", "8", "--channels", "split", "--crosstalk-db", "inf"])
    tr.check_long_args(args, ap)
    assert args.slots == 8 and args.crosstalk_db == float("inf")
    args, ap = parsed(L)
    tr.check_long_args(args, ap)
    assert args.slots == 64 and args.crosstalk_db is None  # no gate where no segment has a channel
    with pytest.raises(SystemExit, match="--kaldi-text needs a tokenizer found on disk"):
        tr.load_long_tokenizer(parsed(L + ["--channels", "split", "--kaldi-text", "t", "--tokenizer", "/nonexistent/dir"])[0])
    assert tr.load_long_tokenizer(parsed(L)[0]) is None


def test_load_references_refusals_need_no_model(tmp_path):
    with pytest.raises(SystemExit, match="--ref needs a tokenizer found on disk"):
        tr.load_references(parsed(S + ["--ref", "r"])[0], None)
    with pytest.raises(SystemExit, match="--ref without a FILE needs --split"):
        tr.load_references(parsed(S + ["--ref"])[0], Tok())
    bad = tmp_path / "bad.ids"
    bad.write_text("u1 5 six 7\n")
    with pytest.raises(SystemExit, match="the line of u1 is not 'utt_id id id ...'"):
        tr.load_references(parsed(S + ["--ref-ids", str(bad)])[0], None)
    assert tr.load_references(parsed(S)[0], None) is None


def test_one_recording_id_rule(tmp_path):
    assert tr.kaldi_rec_id("a/b/call-8k one.wav") == "call_8k_one" == se.rec_key("call-8k one")
    p = tmp_path / "out.jsonl"
    p.write_text('{"id": "call-8k one", "segments": [{"start_s": 0.0, "text": "hi"}]}\n')
    assert list(se.read_hyp(str(p), True)) == ["call_8k_one"]  # score_errors maps the JSON id as --kaldi-text wrote the file's
