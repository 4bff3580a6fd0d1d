"""The beam-search rule on the CPU: tests/decoder_beam_ref.py drives the float64 decoder oracle and must return what HuggingFace's
``generate(num_beams=K, num_return_sequences=K)`` returns in float64 -- the same hypotheses in the same order, scores to 1e-9 -- on
weights whose hypotheses end at different steps.  Also the host side: argument errors by name, the ``--beams`` flags of the command
line, and ``generate`` / ``generate_many`` refusing ``num_beams`` as before."""
import importlib

import numpy as np
import pytest
import torch

import decoder_beam_ref as ref
import speecht5_decoder_oracle as dec_oracle

SEED, T, V, UTTERANCES = 13, 20, 81, 4
CASES = [(4, 1.0, False, 16), (3, 0.0, True, 12), (5, 2.0, "never", 10), (2, 1.0, False, 24)]  # K, length_penalty, early_stopping, max_length
BETAS = [2.5, 3.0, 3.5]
_seen = {"lengths": set(), "capped": 0, "cases": 0}


def encoder_rows(synth, u):
    return synth.hashed_uniform(f"beam_ref/{u}", (1, T, 768), SEED).astype(np.float32)


def oracle_search(sd, enc, K, length_penalty, early_stopping, cap):
    def logprobs(rows):
        logits = dec_oracle.forward(np.repeat(enc, rows.shape[0], 0), None, rows, sd, torch.float64)[:, -1]
        return torch.log_softmax(logits, -1).numpy()  # float64: the restatement adds them to float64 scores

    g = ref.BeamGroup(K, V, cap, cap, length_penalty, early_stopping)
    while g.open:
        cur = int(g.pos[0]) + 1
        lp = logprobs(g.tokens[:, :cur].copy())
        assert g.step64(lp)
        g.reorder()
    return g


@pytest.fixture(scope="module")
def hf():
    tr = pytest.importorskip("transformers")
    return tr


@pytest.mark.parametrize("beta", BETAS)
@pytest.mark.parametrize("K,length_penalty,early_stopping,cap", CASES)
def test_restatement_matches_hf_generate(hf, synth, K, length_penalty, early_stopping, cap, beta):
    from transformers.modeling_outputs import BaseModelOutput
    sd = ref.beam_weights(synth, beta)
    model = hf.SpeechT5ForSpeechToText(hf.SpeechT5Config(encoder_layers=1, decoder_layers=2, tie_word_embeddings=False)).eval()
    hf_sd = {(k if k.startswith("text_decoder_postnet.") else "speecht5." + k): torch.from_numpy(np.array(v)) for k, v in sd.items()}
    missing, unexpected = model.load_state_dict(hf_sd, strict=False)
    assert not unexpected and not any((".decoder." in k and "embed_positions" not in k) or "lm_head" in k for k in missing), (missing, unexpected)
    model = model.double()
    enc = np.concatenate([encoder_rows(synth, u) for u in range(UTTERANCES)])
    with torch.no_grad():
        out = model.generate(encoder_outputs=BaseModelOutput(last_hidden_state=torch.from_numpy(enc).double()), num_beams=K, num_return_sequences=K,
                             length_penalty=length_penalty, early_stopping=early_stopping, max_length=cap, do_sample=False,
                             return_dict_in_generate=True, output_scores=True)
    # HF reads every step's logits as fp32 and carries its beam scores in fp32 whatever the model's dtype, so sequences_scores is a
    # float32 tensor.  The float64 reference for a score is therefore HF's float64 model teacher-forced on the hypothesis HF returned:
    # the sum of its tokens' log-probabilities over generated ** length_penalty, HF's definition of sequences_scores.  HF's own fp32
    # tensor must agree with that to fp32's rounding of a sum of at most cap terms.
    ids = out.sequences
    ended = torch.cat([torch.zeros_like(ids[:, :1]), (ids[:, 1:] == ref.EOS).cumsum(1)], 1)  # > 0 from the row's </s> on
    counted = (ended[:, :-1] == 0)[:, :ids.shape[1] - 1]  # token t + 1 counts until and including the first </s> after the start
    with torch.no_grad():
        logits = model(encoder_outputs=BaseModelOutput(last_hidden_state=torch.from_numpy(np.repeat(enc, K, 0)).double()),
                       decoder_input_ids=ids[:, :-1]).logits
    assert logits.dtype == torch.float64 and out.sequences_scores.dtype == torch.float32
    token_lp = torch.log_softmax(logits, -1).gather(2, ids[:, 1:, None])[:, :, 0] * counted
    exact = token_lp.sum(1) / counted.sum(1).double() ** length_penalty
    assert bool(((exact - out.sequences_scores.double()).abs() <= cap * 2.0 ** -23 * exact.abs().clamp(min=1.0)).all())
    seqs, scores = out.sequences.view(UTTERANCES, K, -1), exact.view(UTTERANCES, K)
    for u in range(UTTERANCES):
        g = oracle_search(sd, enc[u:u + 1], K, length_penalty, early_stopping, cap)
        got = g.finished()
        assert len(got) == K
        for h, (tok, score, total, _) in enumerate(got):
            row = seqs[u, h].tolist()
            assert row[:len(tok)] == tok and all(t == ref.PAD for t in row[len(tok):]), (u, h, tok, row)
            assert abs(score - float(scores[u, h])) <= 1e-9, (u, h, score, float(scores[u, h]))
            _seen["lengths"].add(len(tok))
            _seen["capped"] += int(len(tok) == cap and tok[-1] != ref.EOS)
    _seen["cases"] += 1


def test_cases_are_not_the_trivial_regime():
    """Runs after the comparison above (file order): its cases hold hypotheses of at least three lengths and one ended by its cap."""
    if not _seen["cases"]:
        pytest.importorskip("transformers")
    assert len(_seen["lengths"]) >= 3 and _seen["capped"] >= 1, _seen


def test_float32_steps_follow_the_same_rule():
    """``step`` (float32 log-probabilities, what the device hands out) is ``step64`` on the same values."""
    rng = np.random.default_rng(5)
    a, b = ref.BeamGroup(3, 32, 8, 7, 0.5, "never"), ref.BeamGroup(3, 32, 8, 7, 0.5, "never")
    while a.open:
        lp = torch.log_softmax(torch.from_numpy(rng.standard_normal((3, 32)).astype(np.float32) * 3), -1).numpy()
        assert a.step(lp) and b.step64(lp.astype(np.float64))
        a.reorder(), b.reorder()
        for n in ref.BeamGroup.ARRAYS:
            assert np.array_equal(getattr(a, n), getattr(b, n), equal_nan=True), n
    assert not b.open and a.finished()


def test_total_order_and_stable_list():
    nan = float("nan")
    cands = [(nan, 7), (1.0, 9), (nan, 2), (1.0, 3), (-np.inf, 0), (2.0, 50), (-0.0, 5), (0.0, 4)]
    assert [c[1] for c in sorted(cands, key=lambda c: ref.candidate_key(*c))] == [50, 3, 9, 4, 5, 0, 2, 7]
    assert ref.score_above(1.0, nan) and not ref.score_above(nan, 1.0) and not ref.score_above(nan, nan) and not ref.score_above(1.0, 1.0)
    assert ref.den_table(2.0, 5).tolist() == [1.0, 1.0, 4.0, 9.0, 16.0] and ref.den_table(0.0, 3).tolist() == [1.0, 1.0, 1.0]


# ---- the host side ------------------------------------------------------------------------------------------------------------------------
def test_check_beam_args_names_the_offender():
    dec = importlib.import_module("loco-asr_amd.decoder")
    lib = importlib.import_module("loco-asr_amd._lib")
    k, n, cfg = dec.check_beam_args(4, None, 1.0, False, vocab=81)
    assert (k, n, cfg.num_beams, cfg.length_penalty, cfg.early_stopping, cfg.struct_size) == (4, 1, 4, 1.0, 0, 24)
    assert isinstance(cfg, lib.BeamConfig)
    assert dec.check_beam_args(16, 16, -0.5, "never")[2].early_stopping == 2 and dec.check_beam_args(1, 1, 0, True)[2].early_stopping == 1
    for kwargs, word in [(dict(num_beams=0), "num_beams"), (dict(num_beams=17), "num_beams"), (dict(num_beams=2.5), "num_beams"),
                         (dict(num_beams=4, vocab=7), "num_beams"), (dict(num_beams=4, num_return_sequences=5), "num_return_sequences"),
                         (dict(num_beams=4, num_return_sequences=0), "num_return_sequences"), (dict(num_beams=4, length_penalty=float("nan")), "length_penalty"),
                         (dict(num_beams=4, length_penalty=float("inf")), "length_penalty"), (dict(num_beams=4, length_penalty="x"), "length_penalty"),
                         (dict(num_beams=4, early_stopping="sometimes"), "early_stopping"), (dict(num_beams=4, early_stopping=1), "early_stopping"),
                         (dict(num_beams=4, early_stopping=None), "early_stopping")]:
        with pytest.raises(ValueError, match=word):
            dec.check_beam_args(**kwargs)


def test_generate_still_refuses_num_beams():
    dec = importlib.import_module("loco-asr_amd.decoder")
    with pytest.raises(NotImplementedError, match="num_beams"):
        dec.check_generate_kwargs(dict(num_beams=4))
    dec.check_generate_kwargs(dict(num_beams=1))


def parse(argv):
    tr = importlib.import_module("loco-asr_amd.transcribe")
    ap = tr.build_parser()
    args = ap.parse_args(argv)
    tr.check_args(args, ap)
    return args


def test_beams_flags():
    tr = importlib.import_module("loco-asr_amd.transcribe")
    common = ["--random-init", "--synthetic", "2"]
    args = parse(common + ["--slots", "64", "--beams", "4", "--nbest", "3", "--length-penalty", "0.5", "--early-stopping", "never", "--select", "mbr"])
    assert (args.beams, args.nbest, args.length_penalty, args.early_stopping, args.seed) == (4, 3, 0.5, "never", None)
    assert tr.beam_early_stopping(args.early_stopping) == "never" and tr.beam_early_stopping(None) is False and tr.beam_early_stopping("true") is True
    assert parse(common).beams is None
    for flags in (["--temperature", "0.7"], ["--top-k", "5"], ["--top-p", "0.9"], ["--seed", "3"], ["--greedy-first"]):
        with pytest.raises(SystemExit) as e:  # argparse's error: exit status 2
            parse(common + ["--slots", "8", "--beams", "4", "--nbest", "2"] + flags)
        assert e.value.code == 2
    for flags in (["--length-penalty", "2"], ["--early-stopping", "true"]):
        with pytest.raises(SystemExit) as e:
            parse(common + ["--slots", "8"] + flags)
        assert e.value.code == 2
    with pytest.raises(SystemExit, match="--beams needs --slots"):
        parse(common + ["--beams", "4"])
    with pytest.raises(SystemExit, match="is below --beams"):
        parse(common + ["--beams", "4", "--slots", "3"])
    with pytest.raises(SystemExit, match="num_return_sequences"):
        parse(common + ["--beams", "4", "--slots", "8", "--nbest", "5"])
    with pytest.raises(SystemExit, match="num_beams"):
        parse(common + ["--beams", "17", "--slots", "64"])


def test_nbest_records_keep_the_beam_order():
    tr = importlib.import_module("loco-asr_amd.transcribe")
    hyps = [torch.tensor([2, 5, 2]), torch.tensor([2, 7, 8, 2])]
    recs = tr.nbest_records(hyps, [-3.0, -2.0], None, None, [-1.5, -2.0 / 3])
    assert [r["ids"] for r in recs] == [[2, 5, 2], [2, 7, 8, 2]] and [list(r) for r in recs] == [["ids", "score", "logprob", "avg_logprob"]] * 2
    assert recs[0]["score"] == -1.5 and recs[1]["avg_logprob"] == -2.0 / 3
    assert [r["ids"] for r in tr.nbest_records(hyps, [-3.0, -2.0], None)] == [[2, 7, 8, 2], [2, 5, 2]]  # sampled lists: by logprob, as before
