"""The edit-distance rule on the host: the numpy restatement (tests/edit_distance_ref.py) against a brute-force enumeration of all
alignments and a plain Levenshtein, the rule's identities, and the host side of the feature -- symbol mapping, the Kaldi line, the
CLIs' flag surfaces and the C ABI's refusals by name (made before any HIP call, so they need no GPU)."""
import importlib
import itertools
import random

import numpy as np
import pytest

import edit_distance_ref as ref

_lib = importlib.import_module("loco-asr_amd._lib")
metrics = importlib.import_module("loco-asr_amd.metrics")


def brute(a, b):
    """The least (cost, S) over ALL alignments of a and b, enumerated one by one (no table, no memo)."""
    def walk(i, j):
        if i == len(a) and j == len(b):
            yield (0, 0)
            return
        if i < len(a) and j < len(b):
            step = (0, 0) if a[i] == b[j] else (1, 1)
            for c, s in walk(i + 1, j + 1):
                yield (c + step[0], s + step[1])
        if i < len(a):
            for c, s in walk(i + 1, j):
                yield (c + 1, s)
        if j < len(b):
            for c, s in walk(i, j + 1):
                yield (c + 1, s)
    return min(walk(0, 0))


def levenshtein(a, b):
    prev = list(range(len(b) + 1))
    for i in range(1, len(a) + 1):
        cur = [i] + [0] * len(b)
        for j in range(1, len(b) + 1):
            cur[j] = min(prev[j - 1] + (a[i - 1] != b[j - 1]), prev[j] + 1, cur[j - 1] + 1)
        prev = cur
    return prev[len(b)]


def test_restatement_equals_brute_force_over_all_binary_pairs():
    seqs = [s for n in range(6) for s in itertools.product((0, 1), repeat=n)]
    assert len(seqs) == 63
    for a in seqs:
        for b in seqs:
            key = ref.edit_key(a, b)
            assert (key >> 32, key & 0xffffffff) == brute(a, b), (a, b)


def test_cost_equals_plain_levenshtein():
    rng = random.Random(7)
    for _ in range(200):
        k = rng.choice((2, 3, 30))
        a = [rng.randrange(k) for _ in range(rng.randrange(0, 40))]
        b = [rng.randrange(k) for _ in range(rng.randrange(0, 40))]
        S, D, I, hits = ref.edit_counts(a, b)
        assert S + D + I == levenshtein(a, b), (a, b)
        assert hits + S + D == len(a) and hits + S + I == len(b) and min(S, D, I, hits) >= 0
        S2, D2, I2, hits2 = ref.edit_counts(b, a)  # a swap keeps cost, S and hits and exchanges D with I
        assert (S2, D2, I2, hits2) == (S, I, D, hits)


def test_identities_and_the_tie_rule():
    a = [5, 1, 4, 1, 5, 9, 2, 6]
    assert ref.edit_counts(a, a) == (0, 0, 0, len(a))
    assert ref.edit_counts(a, []) == (0, len(a), 0, 0)
    assert ref.edit_counts([], a) == (0, 0, len(a), 0)
    assert ref.edit_counts([], []) == (0, 0, 0, 0)
    # cost 2 either way: two substitutions, or a deletion and an insertion around one hit -- most correct symbols wins
    assert ref.edit_counts([1, 2], [2, 1]) == (0, 1, 1, 1)


def test_risk_restatement():
    hyps = [[1, 2, 3], [1, 2, 3], [1, 3], [4]]
    risk, best = ref.nbest_risk(hyps)
    assert risk == [(0 + 1 + 3) / 4, (0 + 1 + 3) / 4, (1 + 1 + 2) / 4, (3 + 3 + 2) / 4] and best == 0  # an exact tie: the lowest index
    risk, best = ref.nbest_risk(hyps, [0.0, 0.0, 0.0, 1.0])
    assert risk == [3.0, 3.0, 2.0, 0.0] and best == 3
    assert ref.nbest_risk([[1, 2]]) == ([0.0], 0)
    assert ref.nbest_pairs(3) == [(0, 1), (0, 2), (1, 2)]


def test_strip_specials():
    assert metrics.strip_specials([2, 10, 11, 2, 1, 1]).tolist() == [10, 11]
    assert metrics.strip_specials([2, 10, 1, 11]).tolist() == [10, 11]  # never ended: the whole row, <pad> dropped
    assert metrics.strip_specials([10, 11, 2]).tolist() == [10, 11]    # no start token to drop
    assert metrics.strip_specials([2, 2]).tolist() == [] and metrics.strip_specials([]).tolist() == []
    import torch
    assert metrics.strip_specials(torch.tensor([2, 7, 2])).tolist() == [7]
    with pytest.raises(ValueError, match="1-D"):
        metrics.strip_specials([[1, 2]])


def test_words_of_and_text_units():
    w = metrics.words_of([[4, 7, 8, 4, 9, 4, 4, 7, 8], [9, 4], [], [4]], delimiter_id=4)
    assert [x.tolist() for x in w] == [[0, 1, 0], [1], [], []] and all(x.dtype == np.int32 for x in w)
    with pytest.raises(ValueError, match="delimiter_id is required"):
        metrics.words_of([[1]], None)
    t = metrics.text_units(["the cat  sat", "cat the", ""], "word")
    assert [x.tolist() for x in t] == [[0, 1, 2], [1, 0], []]
    c = metrics.text_units(["ab", "é"], "char")
    assert [x.tolist() for x in c] == [[97, 98], [233]]
    with pytest.raises(ValueError, match="not 'word' or 'char'"):
        metrics.text_units(["a"], "token")


def test_kaldi_line_format():
    assert metrics.format_kaldi_line("WER", 73, 40, 10, 997) == "%WER 12.34 [ 123 / 997, 10 ins, 40 del, 73 sub ]"
    assert metrics.format_kaldi_line("CER", 0, 0, 0, 5) == "%CER 0.00 [ 0 / 5, 0 ins, 0 del, 0 sub ]"
    assert metrics.format_kaldi_line("WER", 0, 0, 0, 0).startswith("%WER nan [ 0 / 0,")


def test_unit_arguments_are_refused_before_any_device_work():
    with pytest.raises(ValueError, match="needs delimiter_id"):
        metrics.mbr_select([[[2, 5, 2]]], unit="word")
    with pytest.raises(ValueError, match="not 'token' or 'word'"):
        metrics.mbr_select([[[2, 5, 2]]], unit="char")
    with pytest.raises(ValueError, match="at least one hypothesis"):
        metrics.mbr_select([[]])
    with pytest.raises(ValueError, match="scores="):
        metrics.mbr_select([[[2, 5, 2]]], weights="logprob")
    with pytest.raises(ValueError, match="1 references for 2"):
        metrics.edit_counts([[1]], [[1], [2]])


def test_flag_surfaces():
    tr = importlib.import_module("loco-asr_amd.transcribe")
    flags = {s for a in tr.build_parser()._actions for s in a.option_strings}
    assert {"--select", "--ref", "--ref-ids", "--nbest", "--kaldi-text"} <= flags
    args = tr.build_parser().parse_args(["--random-init", "--synthetic", "2"])
    assert (args.select, args.ref, args.ref_ids) == (None, None, None)
    assert tr.build_parser().parse_args(["--split", "devel", "--ref"]).ref == ""
    se = importlib.import_module("loco-asr_amd.score_errors")
    flags = {s for a in se.build_parser()._actions for s in a.option_strings}
    assert {"--ref", "--hyp", "--unit", "--per-utt", "--long"} <= flags
    with pytest.raises(SystemExit):
        se.build_parser().parse_args(["--ref", "a", "--hyp", "b", "--unit", "token"])


def test_select_without_nbest_is_an_argparse_error(capsys):
    tr = importlib.import_module("loco-asr_amd.transcribe")
    for choice in ("mbr", "first"):
        with pytest.raises(SystemExit) as e:
            tr.main(["--random-init", "--synthetic", "2", "--select", choice])
        assert e.value.code == 2 and "--select needs --nbest" in capsys.readouterr().err


def test_score_errors_joins_recordings_in_time_order(tmp_path):
    se = importlib.import_module("loco-asr_amd.score_errors")
    utts = {"rec1-B-000300-000400": "c", "rec1-A-000100-000200": "a b", "rec2-x": "later", "rec2-w": "sooner", "rec1-A-000300-000350": "d"}
    assert se.join_recordings(utts) == {"rec1": "a b d c", "rec2": "later sooner"}
    p = tmp_path / "out.jsonl"
    p.write_text('{"id": "my-call", "segments": [{"start_s": 2.0, "text": "world"}, {"start_s": 0.5, "text": "hello"}]}\n')
    assert se.read_hyp(str(p), True) == {"my_call": "hello world"}
    p.write_text('{"id": "u1", "token_ids": [2, 5, 2], "text": "hi"}\n')
    assert se.read_hyp(str(p), False) == {"u1": "hi"}


def test_host_side_refusals_by_name():
    lib = _lib.load()
    assert lib.loco_edit_max_len() == 16384
    good, off = 0x10000, 0x10002  # never dereferenced: every refusal below is made before any HIP call

    def refused(rc, word):
        assert rc == -1 and word in lib.loco_last_error().decode(), (rc, lib.loco_last_error())

    ed = lib.loco_op_edit_distance
    refused(ed(None, 8, good, 1, 64, good, None), "symbols is null")
    refused(ed(good, 8, None, 1, 64, good, None), "spans is null")
    refused(ed(good, 8, good, 1, 64, None, None), "counts is null")
    refused(ed(good, 8, good, -1, 64, good, None), "P = -1")
    refused(ed(good, -8, good, 1, 64, good, None), "n_symbols = -8")
    refused(ed(good, 2 ** 31, good, 1, 64, good, None), "n_symbols = 2147483648")
    refused(ed(good, 8, good, 1, -1, good, None), "max_len = -1")
    refused(ed(good, 8, good, 1, 16385, good, None), "max_len = 16385")
    refused(ed(off, 8, good, 1, 64, good, None), "symbols is not 4-byte aligned")
    refused(ed(good, 8, good + 8, 1, 64, good, None), "spans is not 16-byte aligned")
    refused(ed(good, 8, good, 1, 64, off, None), "counts is not 4-byte aligned")
    nr = lib.loco_op_nbest_risk
    refused(nr(None, good, None, 1, good, good, None), "counts is null")
    refused(nr(good, None, None, 1, good, good, None), "group_offsets is null")
    refused(nr(good, good, None, 1, None, good, None), "risk is null")
    refused(nr(good, good, None, 1, good, None, None), "best is null")
    refused(nr(good, good, None, -2, good, good, None), "U = -2")
    refused(nr(good, good, good + 4, 1, good, good, None), "weights is not 8-byte aligned")
    refused(nr(good, good, None, 1, good + 4, good, None), "risk is not 8-byte aligned")
    refused(nr(good, off, None, 1, good, good, None), "group_offsets is not 4-byte aligned")
