"""The n-gram rule and its shallow fusion on the CPU (include/loco_asr.h, "n-gram language model"; NOT validated against KenLM/SRILM
binaries -- the rule is this project's own and tests/ngram_ref.py pins it).

1. tests/ngram_ref.py on a corpus small enough to do by hand: the Witten-Bell probabilities as exact fractions.
2. Normalisation: |sum_w exp(log P(w | h)) - 1| <= 1e-12 at orders 1, 2, 5, 8 over seen contexts, wholly unseen ones, ones with an
   unseen id in the middle and ones shorter than order - 1 that start at <s>.
3. The product's trainer (loco-asr_amd/ngram.py) against the restatement: the same grams, values within 1e-12; ARPA written and read
   back reproduces the table to 1e-15 relative; the reader's refusals by name.
4. tests/decoder_fusion_ref.py against tests/decoder_beam_ref.py: with a zero bonus (and with none) every array is identical through
   40 scripted steps; a bonus changes the order of the candidates.
5. The model the GPU test fuses (fusion_cases.fusion_model) changes what the float64 decoder oracle's beam search returns.
6. The host side's refusals: beam_search_many's arguments and the command line's flags.
"""
import importlib
import math
from fractions import Fraction

import numpy as np
import pytest
import torch

import decoder_beam_ref as ref
import decoder_fusion_ref as fref
import fusion_cases as fc
import ngram_ref as ng

ORDERS = [1, 2, 5, 8]


def product():
    return importlib.import_module("loco-asr_amd.ngram")


# ---- 1. by hand ---------------------------------------------------------------------------------------------------------------------
def test_witten_bell_by_hand():
    """V = 4, sentences <s> 3 3 </s> and <s> 3 </s>.  Unigrams: c(3) = 3, c(</s>) = 2, c() = 5, T() = 2, so P(w) = (c(w) + 2/4) / 7.
    After <s>: c = 2, T = 1, P(3|<s>) = (2 + 1/2) / 3.  After 3: c = 3, T = 2, P(3|3) = (1 + 2 * 1/2) / 5, P(</s>|3) = (2 + 2 * 5/14) / 5."""
    prob, bo = ng.wb_probabilities([[3, 3], [3]], 2, 4, exact=True)
    assert prob == {(0,): Fraction(1, 14), (1,): Fraction(1, 14), (2,): Fraction(5, 14), (3,): Fraction(1, 2),
                    (4, 3): Fraction(5, 6), (3, 3): Fraction(2, 5), (3, 2): Fraction(19, 35)}
    assert bo == {(): Fraction(2, 7), (4,): Fraction(1, 3), (3,): Fraction(2, 5)}
    m = ng.train([[3, 3], [3]], 2, 4)
    assert set(m.logp) == set(prob) | {(4,)}
    for g, p in prob.items():
        assert abs(m.logp[g] - math.log(p)) <= 1e-15
    assert abs(m.bo[(3,)] - math.log(2 / 5)) <= 1e-15 and abs(m.bo[(4,)] - math.log(1 / 3)) <= 1e-15 and m.bo[(3, 2)] == 0.0
    # the chain: an unseen successor of a seen context backs off with the context's weight, P(0|3) = 2/5 * 1/14
    assert abs(ng.logprob(m, [4, 3], 0) - math.log(Fraction(1, 35))) <= 1e-15
    assert ng.logprob(m, [4, 3], 3) == m.logp[(3, 3)]
    # a context that is no gram adds no weight: P(3 | 0) = P(3)
    assert ng.logprob(m, [4, 0], 3) == m.logp[(3,)]
    assert ng.next_logprobs(m, [2]).tolist() == [ng.logprob(m, [4], w) for w in range(4)]


# ---- 2. normalisation ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", ORDERS)
def test_probabilities_sum_to_one(order):
    V = 30
    seqs = ng.corpus(order, 200, fc.SEEN_IDS)
    m = ng.train(seqs, order, V)
    worst = 0.0
    for kind, rows in fc.probe_rows(seqs, order, V).items():
        assert rows, kind
        for row in rows:
            worst = max(worst, abs(float(np.exp(ng.next_logprobs(m, row)).sum()) - 1.0))
    print(f"order {order}: worst |sum - 1| = {worst:.3e}")
    assert worst <= 1e-12


# ---- 3. the product's host side -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", ORDERS)
def test_product_trainer_matches_the_restatement(order):
    seqs = ng.corpus(100 + order, 150, fc.SEEN_IDS)
    want = ng.train(seqs, order, 30)
    got = product().NgramLM.train(seqs, order, 30).grams()
    assert set(got) == set(want.logp)
    assert max(abs(got[g][0] - want.logp[g]) for g in got) <= 1e-12 and max(abs(got[g][1] - want.bo[g]) for g in got) <= 1e-12


def test_arpa_round_trip(tmp_path):
    P = product()
    seqs = ng.corpus(3, 80, fc.SEEN_IDS)
    lm = P.NgramLM.train(seqs, 4, 30)
    lm.to_arpa(tmp_path / "a.arpa")
    back = P.NgramLM.from_arpa(tmp_path / "a.arpa", 30)
    a, b = lm.grams(), back.grams()
    assert set(a) == set(b) and back.order == 4 and back.vocab == 30
    for g in a:
        for x, y in zip(a[g], b[g]):
            assert abs(x - y) <= 1e-15 * abs(x), (g, x, y)
    # the restatement reads the product's file and the product the restatement's
    m = ng.read_arpa(tmp_path / "a.arpa", 30)
    assert set(m.logp) == set(a) and all(m.logp[g] == b[g][0] and m.bo[g] == b[g][1] for g in b)
    ng.write_arpa(ng.train(seqs, 4, 30), tmp_path / "b.arpa")
    c = P.NgramLM.from_arpa(tmp_path / "b.arpa", 30).grams()
    assert set(c) == set(a) and max(abs(c[g][0] - a[g][0]) for g in a) <= 1e-12


def test_arpa_reader_refusals(tmp_path):
    P = product()
    head = "\\data\\\nngram 1=3\n\n\\1-grams:\n"
    path = tmp_path / "x.arpa"
    path.write_text(head + "-1\t0\n-1\t1\n-1\t</s>\n-1\t2\n\\end\\\n")
    with pytest.raises(ValueError, match="beside </s>"):
        P.NgramLM.from_arpa(path, 3)
    path.write_text(head + "-1\t0\n-1\t</s>\n\\end\\\n")
    with pytest.raises(ValueError, match="id 1 has no unigram"):
        P.NgramLM.from_arpa(path, 3)
    path.write_text(head + "-1\t0\n-1\t</s>\n-2.5\t<unk>\n\\end\\\n")
    lm = P.NgramLM.from_arpa(path, 3)
    assert lm.grams()[(1,)] == (-2.5 * math.log(10.0), 0.0) and len(lm) == 3
    path.write_text(head + "-1\t0\n-1\t7\n\\end\\\n")
    with pytest.raises(ValueError, match="'7'"):
        P.NgramLM.from_arpa(path, 3)
    for kwargs, word in [(dict(order=9, vocab=30), "order"), (dict(order=2, vocab=128), "vocab")]:
        with pytest.raises(ValueError, match=word):
            P.NgramLM.train([[4, 5]], **kwargs)
    with pytest.raises(RuntimeError, match="no CPU path"):
        P.NgramLM.train([[4, 5]], 2, 30).to("cpu")


def test_command_line_trains_from_id_lines(tmp_path):
    P = product()
    ids = tmp_path / "ref.ids"
    ids.write_text("utt1 2 5 6 7 2\nutt2 5 6 1 1\n\nutt3 2 8 5 6 2 1\n")
    assert P.main(["--ids", str(ids), "--order", "3", "--vocab", "30", "--out", str(tmp_path / "lm.arpa")]) == 0
    got = P.NgramLM.from_arpa(tmp_path / "lm.arpa", 30).grams()
    want = ng.train([[5, 6, 7], [5, 6], [8, 5, 6]], 3, 30)  # <s>, </s> and <pad> stripped
    assert set(got) == set(want.logp) and max(abs(got[g][0] - want.logp[g]) for g in got) <= 1e-12


# ---- 4. the fused restatement ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 3, 4])
def test_zero_bonus_is_the_plain_rule(K):
    V, S = 32, 12
    rng = np.random.default_rng(K)
    steps, groups = 0, 0
    while steps < 40:
        lp_pen, early = [(1.0, False), (0.0, True), (2.0, "never")][groups % 3]
        a = ref.BeamGroup(K, V, S, 5 + groups % 7, lp_pen, early)
        b = fref.FusedBeamGroup(K, V, S, 5 + groups % 7, lp_pen, early)
        c = fref.FusedBeamGroup(K, V, S, 5 + groups % 7, lp_pen, early)
        while a.open and steps < 40:
            lp = torch.log_softmax(torch.from_numpy(rng.standard_normal((K, V)).astype(np.float32) * 3), -1).numpy()
            lp[:, ref.EOS] += np.float32(rng.uniform(-2, 3))
            assert a.step(lp) and b.step(lp, np.zeros((K, V))) and c.step(lp)
            a.reorder(), b.reorder(), c.reorder()
            for n in ref.BeamGroup.ARRAYS:
                assert np.array_equal(getattr(a, n), getattr(b, n), equal_nan=True), n
                assert np.array_equal(getattr(a, n), getattr(c, n), equal_nan=True), n
            steps += 1
        groups += 1
    assert groups >= 3


def test_a_bonus_reorders_the_candidates_and_ties_go_to_the_lower_index():
    K, V, S = 2, 8, 6
    lp = np.log(np.array([[.4, .3, .05, .05, .05, .05, .05, .05]] * K, np.float32))
    plain, fused = fref.FusedBeamGroup(K, V, S, 6), fref.FusedBeamGroup(K, V, S, 6)
    bonus = np.zeros((K, V))
    bonus[0, 5] = 3.0
    assert plain.step(lp) and fused.step(lp, bonus)
    assert plain.tokens[:, 1].tolist() == [0, 1] and fused.tokens[:, 1].tolist() == [5, 0]
    assert fused.run[0] == (0.0 + np.float64(lp[0, 5])) + 3.0 and fused.tlp[0, 1] == lp[0, 5]  # the score is fused, the token's log P is not
    tie = fref.FusedBeamGroup(K, V, S, 6)
    b = np.zeros((K, V))
    b[0, 1] = np.float64(lp[0, 0]) - np.float64(lp[0, 1])  # exactly lifts column 1 to column 0's score when the sum is exact
    assert tie.step(lp, b)
    s0, s1 = np.float64(lp[0, 0]) + 0.0, np.float64(lp[0, 1]) + b[0, 1]
    assert (tie.tokens[:, 1].tolist() == [0, 1]) == (s0 >= s1)


# ---- 5. the fused model of the GPU test, on the float64 oracle ---------------------------------------------------------------------------
def test_the_fused_search_differs_from_the_plain_one_on_the_oracle(synth):
    """What tests/test_gpu_decoder_fusion.py asks of the device, confirmed here with the float64 decoder oracle driving the restatement
    (as tests/test_decoder_beam_ref.py drives it): with fusion_cases.fusion_model at weight 1 and bonus 0.3 the lists differ from the
    plain search's and the hypotheses have at least two lengths."""
    import speecht5_decoder_oracle as dec_oracle
    from test_decoder_beam_ref import encoder_rows
    sd = ref.beam_weights(synth, 3.0)
    model = fc.fusion_model()
    K, V = 4, fc.V_MODEL
    differ, lengths = 0, set()
    for u, cap in enumerate([12, 8]):
        enc = encoder_rows(synth, u)

        def logprobs(rows):
            logits = dec_oracle.forward(np.repeat(enc, rows.shape[0], 0), None, rows, sd, torch.float64)[:, -1]
            return torch.log_softmax(logits, -1).numpy()

        plain = fref.search(logprobs, K, V, cap, dtype=np.float64).finished()
        fused = fref.search(logprobs, K, V, cap, ng, model, fc.LM_WEIGHT, fc.LM_BONUS, dtype=np.float64).finished()
        differ += [h[0] for h in plain] != [h[0] for h in fused]
        lengths |= {len(h[0]) for h in fused}
        for tok, score, total, tlp in fused:  # the identity the device is held to: fused sum = acoustic + w * lm + b * (len - 1)
            lm = ng.token_logprobs(model, tok)
            want = float(np.float64(tlp[1:]).sum() + fc.LM_WEIGHT * lm.sum() + fc.LM_BONUS * (len(tok) - 1))
            # here the history keeps the oracle's float64 log-probabilities as float32: half an ulp of float32 per token
            assert abs(total - want) <= 2.0 ** -24 * float(np.abs(np.float64(tlp)).sum()) + 1e-12, (total, want)
    assert differ >= 1 and len(lengths) >= 2, (differ, lengths)


# ---- 5b. the generated code -------------------------------------------------------------------------------------------------------------
def test_the_fused_bonus_is_a_product_and_a_sum_in_the_generated_code(tmp_path):
    """bonus = weight * lm + token_bonus rounds twice: the gfx950 code of csrc/ngram.hip, compiled with the Makefile's flags, multiplies
    and adds in double and holds no fused multiply-add (hipcc contracts by default; csrc/ngram.hip, ngram_fuse).  The fused kernel is
    the only place of the file that multiplies doubles."""
    import shutil
    import subprocess
    from test_isa_patterns import CSRC, makefile_flags
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    out = str(tmp_path / "ngram.s")
    subprocess.run([hipcc] + makefile_flags() + ["-S", "--cuda-device-only", CSRC + "/ngram.hip", "-o", out], check=True, capture_output=True)
    body, name = {}, None
    for line in open(out):
        if line.startswith("_ZN4loco") and ":" in line:
            name = line.split(":")[0]
        elif name and line.startswith("\t") and not line.startswith("\t."):
            body.setdefault(name, []).append(line.split()[0])
    fused = [n for n in body if "ngram_logprobs_kernelILb1E" in n]
    assert len(fused) == 1 and len(body) >= 3, list(body)
    assert not any(op.startswith("v_fma_f64") or op.startswith("v_fmac_f64") for ops in body.values() for op in ops)
    assert body[fused[0]].count("v_mul_f64") == 1 and "v_add_f64" in body[fused[0]]
    assert not any(op == "v_mul_f64" for n, ops in body.items() if n != fused[0] for op in ops)


# ---- 6. the host side's refusals --------------------------------------------------------------------------------------------------------
def test_check_fusion_args_names_the_offender():
    dec = importlib.import_module("loco-asr_amd.decoder")
    lm = product().NgramLM.train([[4, 5]], 2, 30)
    assert dec.check_fusion_args(None) is None
    assert dec.check_fusion_args(lm, 0.5, 0.25, vocab=30) == (lm, 0.5, 0.25)
    for args, word in [((lm, 1.0, 0.0, 81), "vocab"), ((lm, float("nan"), 0.0, 30), "lm_weight"), ((lm, 1.0, float("inf"), 30), "lm_bonus"),
                       ((lm, "x", 0.0, 30), "lm_weight"), ((object(), 1.0, 0.0, 30), "NgramLM"), ((None, 1.0, 0.0, 30), "lm=")]:
        with pytest.raises(ValueError, match=word):
            dec.check_fusion_args(*args)


def test_ngram_flags():
    from test_decoder_beam_ref import parse
    common = ["--random-init", "--synthetic", "2", "--slots", "8"]
    args = parse(common + ["--beams", "4", "--ngram", "lm.arpa", "--lm-weight", "0.5", "--lm-bonus", "0.1", "--scores"])
    assert (args.ngram, args.lm_weight, args.lm_bonus) == ("lm.arpa", 0.5, 0.1)
    assert parse(common + ["--beams", "4"]).ngram is None
    for flags in (["--ngram", "lm.arpa"], ["--beams", "4", "--lm-weight", "0.5"], ["--beams", "4", "--lm-bonus", "0.5"],
                  ["--beams", "4", "--ngram", "lm.arpa", "--lm-weight", "nan"], ["--beams", "4", "--ngram", "lm.arpa", "--lm-bonus", "inf"]):
        with pytest.raises(SystemExit) as e:
            parse(common + flags)
        assert e.value.code == 2


def test_nbest_records_carry_lm_logprob():
    tr = importlib.import_module("loco-asr_amd.transcribe")
    hyps = [torch.tensor([2, 5, 2]), torch.tensor([2, 7, 8, 2])]
    recs = tr.nbest_records(hyps, [-3.0, -2.0], None, None, [-1.5, -2.0 / 3], [-4.0, -5.0])
    assert [list(r) for r in recs] == [["ids", "score", "logprob", "avg_logprob", "lm_logprob"]] * 2 and recs[1]["lm_logprob"] == -5.0
    line = tr.Line("u", [2, 5, 2], (-3.0, 2), None, None, None, -4.0)
    assert tr.utterance_record(line, None)["lm_logprob"] == -4.0 and "lm_logprob" not in tr.utterance_record(tr.Line("u", [2, 5, 2]), None)
