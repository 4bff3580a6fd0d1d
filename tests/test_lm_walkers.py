"""The two corpus walkers of loco-asr_amd/lm.py against what the reference's own dataset classes yielded (fixture lm_windows.json,
recorded by tests/golden/make_lm_goldens.py), id for id, and the per-recording fold's bookkeeping.  CPU only."""
import importlib
import json
import os

import numpy as np

import lm_ref
from conftest import GOLDEN

lm = importlib.import_module("loco-asr_amd.lm")


def fixture():
    with open(os.path.join(GOLDEN, "lm_windows.json")) as fh:
        return json.load(fh)


def utts_of(fx, tmp_path):
    p = tmp_path / "text"
    p.write_text("".join(f"{u} {t}\n" for u, t in fx["lines"]))
    return lm.read_key_text(str(p))


def test_indep_walker_matches_the_reference(tmp_path):
    fx = fixture()
    tok = lm.TokenizedLines(eos_token_id=fx["eos"], bos_token_id=fx["bos"])
    utts = utts_of(fx, tmp_path)
    assert len(utts) == len(fx["lines"]) - 1                     # the duplicate utt_id keeps its first line
    keys, ids, batches = lm.indep_plan(utts, tok, fx["bsize"])
    assert keys == fx["indep"]["utt_ids"]
    assert [ids[a:b] for a, b in batches] == fx["indep"]["batches"]
    for a, b in batches:                                          # at most bsize utterances of EQUAL length
        assert 1 <= b - a <= fx["bsize"] and len({len(t) for t in ids[a:b]}) == 1
    rkeys, rb = lm_ref.indep_batches(fx["lines"], tok, fx["bsize"])
    assert rkeys == keys and rb == fx["indep"]["batches"]


def test_max_len_walker_matches_the_reference(tmp_path):
    fx = fixture()
    tok = lm.TokenizedLines(eos_token_id=fx["eos"], bos_token_id=fx["bos"])
    recs = lm.recordings(utts_of(fx, tmp_path), tok)
    assert {k: len(v) for k, v in recs.items()} == fx["recording_tokens"]
    got = []
    for rec, seq in recs.items():
        for starts, first, last in lm.max_len_plan(len(seq), fx["max_len"], fx["bsize"]):
            S = min(len(seq), fx["max_len"])
            got.append({"batch": [seq[o:o + S] for o in starts], "rec_ids": [rec] * len(starts), "first": first, "last": last})
    assert got == fx["max_len_batches"]
    ref = [{"batch": b, "rec_ids": r, "first": f, "last": l} for b, r, f, l in lm_ref.max_len_batches(fx["lines"], tok, fx["max_len"], fx["bsize"])]
    assert ref == fx["max_len_batches"]


def test_the_two_quirks_and_the_option_that_lifts_them():
    fx = fixture()
    n = fx["max_len"]
    assert list(lm.max_len_plan(n, n, 2)) == []                                           # exactly n_positions tokens: nothing
    assert "rC" not in {r for b in fx["max_len_batches"] for r in b["rec_ids"]} and fx["recording_tokens"]["rC"] == n
    last_start = max(max(s) for s, _, _ in lm.max_len_plan(13, n, 2))
    assert last_start + n - 1 == 13 - 2                                                   # the final token (index 12) is never a target
    assert list(lm.max_len_plan(n, n, 2, strict_reference=False)) == [([0], True, True)]
    assert max(max(s) for s, _, _ in lm.max_len_plan(13, n, 2, strict_reference=False)) + n - 1 == 12
    assert list(lm.max_len_plan(n - 1, n, 2)) == [([0], True, True)]                      # shorter: one sequence, in full


def test_fold_bookkeeping_against_a_hand_case():
    # items: a-1 (2 tokens), b-1 (1), a-2 (3): recording a owns flat positions 0, 1, 3, 4, 5 and b owns 2
    names, perm, offsets = lm.fold_offsets(["a", "b", "a"], [2, 1, 3])
    assert names == ["a", "b"] and perm.tolist() == [0, 1, 3, 4, 5, 2] and offsets.tolist() == [0, 5, 6]
    nll = np.asarray([1.0, 2.0, 7.0, 3.0, 4.0, 5.0])
    rec, ppl = lm_ref.fold([[1.0, 2.0], [7.0], [3.0, 4.0, 5.0]], ["a-x", "b-x", "a-y"])
    assert rec == {"a": [1.0, 2.0, 3.0, 4.0, 5.0], "b": [7.0]}
    assert nll[perm][offsets[0]:offsets[1]].tolist() == rec["a"]
    assert abs(ppl["a"] - np.exp(3.0)) < 1e-12 and abs(ppl["b"] - np.exp(7.0)) < 1e-9
    assert lm.rec_id_of("fe_03_00001-A-000123-000456") == "fe_03_00001"
