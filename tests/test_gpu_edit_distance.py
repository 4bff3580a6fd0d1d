"""-m gpu: loco_op_edit_distance / loco_op_nbest_risk (csrc/edit_distance.hip), metrics.py, mbr_many and the CLIs' --select / --ref-ids,
against the numpy restatement of the rule (tests/edit_distance_ref.py).  Everything is integer and compared for equality; the risks
are doubles summed in a written-down order (h' ascending, every product and sum rounded on its own) and compared bit for bit.

The shapes are the smallest at which the striped sweep can go wrong: lengths {0, 1, 2, 63, 64, 65, 127, 128, 129, 300} squared put
the lane stripe at c = 1, 2, 3 and 5 columns on both sides of every edge, with empty sides, one-lane pairs, n >> m and m >> n (the
kernel swaps the sides there); alphabet 2 ties everywhere, which is what the (cost, S) min is for.  All pairs go through ONE launch
in shuffled order -- four pairs of very different lengths share a workgroup and its waves leave at different times -- and then
each alone: the numbers are the same."""
import importlib
import json

import numpy as np
import pytest
import torch

import decoder_pool_cases as pc
import edit_distance_ref as ref

pytestmark = pytest.mark.gpu

LENGTHS = (0, 1, 2, 63, 64, 65, 127, 128, 129, 300)
GUARD = 64
FILL = 0x5a5a5a5a


@pytest.fixture(scope="module")
def gu():
    return importlib.import_module("gpu_util")


@pytest.fixture(scope="module")
def metrics():
    return importlib.import_module("loco-asr_amd.metrics")


def related(rng, a, k, m):
    """A hypothesis of m symbols for the reference a: a copy cut or padded to m with a fifth of its symbols redrawn (an alignment
    with long runs of hits), so that the distance is not simply the length."""
    b = np.resize(a, m) if len(a) else rng.integers(0, k, m)
    flip = rng.random(m) < 0.2
    return np.where(flip, rng.integers(0, k, m), b).astype(np.int64)


@pytest.fixture(scope="module")
def cases():
    """[(a, b)] and their (S, D, I, hits) by the restatement, computed once."""
    rng = np.random.default_rng(20240611)
    pairs = []
    for k in (2, 81):
        for n in LENGTHS:
            for m in LENGTHS:
                a = rng.integers(0, k, n).astype(np.int64)
                pairs.append((a, related(rng, a, k, m) if (n + m) % 2 else rng.integers(0, k, m).astype(np.int64)))
    wide = np.array([-2 ** 31, 2 ** 31 - 1, -1, 0, 1, 2 ** 31 - 2, -2 ** 31 + 1, 65536, -65536], dtype=np.int64)
    a = rng.choice(wide, 150)
    pairs.append((a, related(rng, a, 3, 131)))  # negative and large int32 symbols
    a = rng.integers(0, 4, 1024).astype(np.int64)
    pairs.append((a, related(rng, a, 4, 1023)))
    want = np.array([ref.edit_counts(a, b) for a, b in pairs], dtype=np.int32)
    return pairs, want


def layout(pairs, order, gap, fill):
    """One symbol buffer holding every sequence of ``pairs`` with ``gap`` filler symbols before, between and behind them, and the
    spans [P, 4] of the pairs in ``order``."""
    chunks, at, pos = [np.full(gap, fill, dtype=np.int64)], [], gap
    for a, b in pairs:
        for s in (a, b):
            at.append((pos, len(s)))
            chunks += [np.asarray(s, dtype=np.int64), np.full(gap, fill, dtype=np.int64)]
            pos += len(s) + gap
    spans = np.array([[*at[2 * p], *at[2 * p + 1]] for p in order], dtype=np.int32).reshape(-1, 4)
    return np.concatenate(chunks).astype(np.int32), spans


def raw(gu, symbols, spans, max_len, n_symbols=None):
    """loco_op_edit_distance on host arrays: counts [P, 4] (host); a guard band around ``counts`` must come back untouched."""
    sym = torch.from_numpy(np.ascontiguousarray(symbols, dtype=np.int32)).cuda()
    sp = torch.from_numpy(np.ascontiguousarray(spans, dtype=np.int32)).cuda()
    P = int(sp.shape[0])
    buf = torch.full((GUARD + 4 * P + GUARD,), FILL, dtype=torch.int32, device="cuda")
    out = buf[GUARD:GUARD + 4 * P]
    gu.check(gu.lib().loco_op_edit_distance(gu.ptr(sym), int(sym.numel()) if n_symbols is None else n_symbols, gu.ptr(sp), P, int(max_len),
                                            gu.ptr(out), gu.stream()), "loco_op_edit_distance")
    host = buf.cpu()
    assert bool((host[:GUARD] == FILL).all()) and bool((host[GUARD + 4 * P:] == FILL).all()), "the guard band around counts was written"
    return host[GUARD:GUARD + 4 * P].reshape(P, 4).numpy()


def test_one_shuffled_launch_equals_the_restatement(gu, cases):
    pairs, want = cases
    order = np.random.default_rng(5).permutation(len(pairs))
    sym, spans = layout(pairs, order, gap=3, fill=7)
    got = raw(gu, sym, spans, 2048)
    bad = np.flatnonzero((got != want[order]).any(axis=1))
    assert bad.size == 0, [(int(order[p]), len(pairs[order[p]][0]), len(pairs[order[p]][1]), got[p].tolist(), want[order[p]].tolist()) for p in bad[:5]]
    # the symbols outside every span are never read: another filler, the same numbers
    sym2, spans2 = layout(pairs, order, gap=3, fill=-123456)
    assert np.array_equal(spans, spans2) and np.array_equal(raw(gu, sym2, spans, 2048), got)
    # the row state sized by the cap (the one-wave-per-workgroup form): the same numbers
    assert np.array_equal(raw(gu, sym, spans, 16384), got)


def test_each_pair_alone_equals_the_shuffled_launch(gu, metrics, cases):
    pairs, want = cases
    sym, spans = layout(pairs, np.arange(len(pairs)), gap=1, fill=0)
    for p in range(len(pairs)):
        got = raw(gu, sym, spans[p:p + 1], max(64, min(spans[p, 1], spans[p, 3])))
        assert got[0].tolist() == want[p].tolist(), (p, len(pairs[p][0]), len(pairs[p][1]))
    # the Python entry: bucketed launches, host arrays and device tensors mixed
    refs = [torch.from_numpy(a).cuda() if p % 3 == 0 else a for p, (a, _) in enumerate(pairs)]
    hyps = [torch.from_numpy(b) if p % 2 else b.tolist() for p, (_, b) in enumerate(pairs)]
    c = metrics.edit_counts(refs, hyps)
    assert all(t.is_cuda and t.dtype == torch.int32 and t.shape == (len(pairs),) for t in (c.sub, c.dele, c.ins, c.hits, c.ref_len))
    assert np.array_equal(torch.stack([c.sub, c.dele, c.ins, c.hits], dim=1).cpu().numpy(), want)
    assert c.ref_len.cpu().tolist() == [len(a) for a, _ in pairs]
    er = metrics.error_rate(refs, hyps)
    S, D, I = (int(want[:, f].sum()) for f in range(3))
    N = sum(len(a) for a, _ in pairs)
    assert er.sub.dtype == torch.int64 and er.sub.is_cuda and (int(er.sub), int(er.dele), int(er.ins), int(er.ref_len), er.pairs) == (S, D, I, N, len(pairs))
    assert float(er.rate) == (S + D + I) / N
    assert er.kaldi_line() == f"%WER {100.0 * (S + D + I) / N:.2f} [ {S + D + I} / {N}, {I} ins, {D} del, {S} sub ]"


def test_the_cap(gu, metrics):
    cap = metrics.max_len()
    assert cap == 16384
    rng = np.random.default_rng(11)
    a = rng.integers(0, 4, cap).astype(np.int64)
    b = related(rng, a, 4, cap)
    want = ref.edit_counts(a, b)
    c = metrics.edit_counts([a], [b])
    assert (int(c.sub[0]), int(c.dele[0]), int(c.ins[0]), int(c.hits[0])) == tuple(int(v) for v in want)
    with pytest.raises(ValueError, match=r"pair 1: a reference of 3 and a hypothesis of 16385 symbols exceed the 16384"):
        metrics.edit_counts([[1], [1, 2, 3]], [[1], np.zeros(cap + 1, dtype=np.int64)])
    # the raw operator: the pair past the cap gets -1 x 4 and nothing of it is read (its span lies outside n_symbols as well for the
    # hypothesis of pair 3); the pairs beside them are untouched
    sym = np.concatenate([a[:200], b[:200], np.zeros(cap + 1, dtype=np.int64)]).astype(np.int32)
    spans = np.array([[0, 200, 200, 128],        # fine
                      [0, 5, 400, cap + 1],      # a length above the cap
                      [10, 100, 250, 60],        # fine
                      [0, 10, sym.size - 4, 5],  # leaves [0, n_symbols)
                      [0, -1, 0, 5],             # a negative length
                      [-1, 3, 0, 5],             # a negative start
                      [0, 200, 200, 129],        # min(ref_len, hyp_len) > max_len = 128
                      [0, 129, 200, 64]], dtype=np.int32)
    got = raw(gu, sym, spans, 128)
    for p in range(len(spans)):
        if p in (0, 2, 7):
            rs, rn, hs, hn = spans[p]
            assert got[p].tolist() == [int(v) for v in ref.edit_counts(sym[rs:rs + rn], sym[hs:hs + hn])], p
        else:
            assert got[p].tolist() == [-1, -1, -1, -1], p
    # P = 0 does nothing: the counts stay what they were
    out = torch.full((4,), FILL, dtype=torch.int32, device="cuda")
    gu.check(gu.lib().loco_op_edit_distance(gu.ptr(gu.dev(sym, torch.int32)), int(sym.size), gu.ptr(gu.dev(spans, torch.int32)), 0, 128, gu.ptr(out),
                                            gu.stream()), "loco_op_edit_distance")
    assert out.cpu().tolist() == [FILL] * 4
    assert metrics.edit_counts([], []).sub.shape == (0,) and metrics.error_rate([], []).pairs == 0


def test_overlapping_and_coinciding_spans(gu):
    rng = np.random.default_rng(3)
    sym = rng.integers(0, 3, 700).astype(np.int32)
    spans = np.array([[100, 300, 100, 300], [0, 0, 0, 0], [50, 129, 60, 129], [0, 700, 350, 350], [200, 65, 180, 130], [5, 1, 5, 1]], dtype=np.int32)
    got = raw(gu, sym, spans, 512)
    assert got[0].tolist() == [0, 0, 0, 300] and got[1].tolist() == [0, 0, 0, 0] and got[5].tolist() == [0, 0, 0, 1]
    for p, (rs, rn, hs, hn) in enumerate(spans):
        assert got[p].tolist() == [int(v) for v in ref.edit_counts(sym[rs:rs + rn], sym[hs:hs + hn])], p


def bits(x):
    return np.asarray(x, dtype=np.float64).view(np.int64).tolist()


def test_nbest_risk_equals_the_restatement_bit_for_bit(gu, metrics):
    rng = np.random.default_rng(17)
    lists = []
    for N in (1, 2, 3, 16, 64, 3):
        base = rng.integers(3, 9, rng.integers(5, 30))
        lists.append([related(rng, base, 9, int(rng.integers(0, 40))) % 6 + 3 for _ in range(N)])  # ids 3 .. 8: no <s>, </s>, <pad>
    lists[-1] = [lists[-1][0], lists[-1][1], lists[-1][0]]  # hypotheses 0 and 2 are one sequence: an exact tie between them
    weights = [[float(w) for w in rng.random(len(per)) * 3] for per in lists]
    weights[3][5] = 0.0
    for w in (None, weights):
        sel = metrics.mbr_select(lists, weights=w)
        assert sel.best.dtype == torch.int32 and sel.best.is_cuda and all(r.dtype == torch.float64 and r.is_cuda for r in sel.risk)
        best = sel.best.cpu().tolist()
        for u, per in enumerate(lists):
            risk, b = ref.nbest_risk(per, None if w is None else w[u])
            assert bits(sel.risk[u].cpu().numpy()) == bits(risk), (u, w is not None)
            assert best[u] == b, (u, w is not None)
    risk = metrics.mbr_select(lists).risk
    assert float(risk[0][0]) == 0.0 and float(risk[5][0]) == float(risk[5][2])  # one hypothesis: risk 0; the tie is exact
    # weights="logprob": the softmax of the sequence log-probabilities within the list
    scores = [[torch.tensor(-rng.random(4) * 5).cuda() for _ in per] for per in lists]
    soft = [np.exp(s - s.max()) / np.exp(s - s.max()).sum() for s in (np.array([float(t.double().sum()) for t in per]) for per in scores)]
    a, b = metrics.mbr_select(lists, weights="logprob", scores=scores), metrics.mbr_select(lists, weights=[s.tolist() for s in soft])
    assert torch.equal(a.best, b.best) and all(torch.equal(x, y) for x, y in zip(a.risk, b.risk))


def test_a_tie_goes_to_the_lowest_index_and_words(gu, metrics):
    # hypotheses 1 and 3 are one sequence and share the least risk, 3/4; 0 and 2 have 4/4 and 6/4
    lists = [[[3, 4, 5, 6], [3, 4, 5], [7, 4, 5, 8], [3, 4, 5]]]
    risk, best = ref.nbest_risk(lists[0])
    assert risk[1] == risk[3] == min(risk) and best == 1
    sel = metrics.mbr_select(lists)
    assert sel.best.cpu().tolist() == [1] and sel.risk[0].cpu().tolist() == risk
    # word units: ids between the delimiter 4 are one symbol; <s> = </s> = 2 and <pad> = 1 are stripped first
    a, b, c = [2, 5, 6, 4, 7, 2, 1, 1], [2, 5, 6, 4, 8, 8, 2], [2, 5, 4, 7, 2]
    sel = metrics.mbr_select([[a, b, c]], unit="word", delimiter_id=4)
    words = metrics.words_of([metrics.strip_specials(s) for s in (a, b, c)], 4)
    assert [w.tolist() for w in words] == [[0, 1], [0, 2], [3, 1]]
    risk, best = ref.nbest_risk(words)
    assert sel.risk[0].cpu().tolist() == risk == [2 / 3, 3 / 3, 3 / 3] and sel.best.cpu().tolist() == [best] == [0]
    # the oracle error rate: per utterance the first hypothesis of least cost
    o = metrics.oracle_error_rate([[3, 4, 5], [6, 7]], [[[3, 4], [3, 9, 5], [3, 4, 5, 5]], [[7, 6], [6, 7], [6, 7]]])
    assert (int(o.sub), int(o.dele), int(o.ins), int(o.ref_len), o.pairs) == (0, 1, 0, 5, 2)


_cache = {}


def one_layer_model(gu):
    """--random-init's generators with one encoder and one decoder layer: sampled rows never end, so the cap sets their length."""
    if "model" not in _cache:
        la = gu.la
        pre, enc = la.synth.split_state_dict(la.synth.encoder_state_dict(0, 1))
        dec, post = la.synth.split_decoder_state_dict(la.synth.decoder_state_dict(pc.DEC_SEED, layers=1))
        t = lambda d: {k: torch.from_numpy(v) for k, v in d.items()}  # noqa: E731
        _cache["model"] = la.SpeechT5ForSpeechToTextMI355X.from_state_dicts(t(pre), t(enc), layers=1, decoder_state_dict=t(dec),
                                                                            postnet_state_dict=t(post)).to("cuda")
    return _cache["model"]


def test_mbr_many_is_sample_many_then_the_restatements_choice(gu, metrics):
    model = one_layer_model(gu)
    clips = pc.oracle_clips(gu.la.synth)[:6]
    batches = [dict(input_values=gu.dev(x), attention_mask=gu.dev(m, torch.int32)) for x, m in pc.pairs(gu.la.synth, clips)]
    caps = [9, 12, 5, 14, 7, 10]
    kw = dict(num_return_sequences=6, temperature=8.0, top_k=3, seed=41, greedy_first=True, max_length=caps)
    hyps = model.sample_many(batches, slots=4, **kw)
    out = model.mbr_many(batches, slots=4, **kw)
    assert isinstance(out, metrics.MbrTranscripts) and out.seed == 41 and len(out.ids) == len(out.best) == len(out.risk) == 6
    distinct = 0
    for u in range(6):
        assert all(torch.equal(x, y) for x, y in zip(out.hypotheses[u], hyps[u])), u
        units = [metrics.strip_specials(h) for h in hyps[u]]
        distinct += len({tuple(s.tolist()) for s in units}) > 1
        risk, best = ref.nbest_risk(units)
        assert out.best[u] == best and torch.equal(out.ids[u], hyps[u][best]), u
        assert bits(out.risk[u].cpu().numpy()) == bits(risk), u
    assert distinct >= 3, "the hypotheses of most utterances never differ: the choice is not exercised"
    wide = model.mbr_many(batches, slots=64, return_scores=True, **kw)  # the same seed, the same choice at any slots
    assert wide.best == out.best and all(torch.equal(x, y) for x, y in zip(wide.ids, out.ids))
    assert all(torch.equal(x, y) for x, y in zip(wide.risk, out.risk)) and len(wide.scores) == 6 and out.scores is None
    with pytest.raises(ValueError, match="needs delimiter_id"):
        model.mbr_many(batches, unit="word", **kw)


def test_score_errors_cli(tmp_path, capsys):
    se = importlib.import_module("loco-asr_amd.score_errors")
    r, h, per = tmp_path / "ref.txt", tmp_path / "out.jsonl", tmp_path / "per.txt"
    r.write_text("u1 the cat sat\nu2 a b c d\nu3 only here\n")
    h.write_text('{"id": "u1", "text": "the cat  sat"}\n{"id": "u2", "text": "a x c"}\n{"id": "u4", "text": "zzz"}\n')
    assert se.main(["--ref", str(r), "--hyp", str(h), "--per-utt", str(per)]) == 0
    out = capsys.readouterr().out.splitlines()
    assert out == ["%WER 28.57 [ 2 / 7, 0 ins, 1 del, 1 sub ]", "%CER 16.67 [ 3 / 18, 0 ins, 2 del, 1 sub ]",
                   "scored 2 utterances; 1 only in --ref, 1 only in --hyp"]
    assert per.read_text().splitlines() == ["u1 %WER 0.00 [ 0 / 3, 0 ins, 0 del, 0 sub ]", "u2 %WER 50.00 [ 2 / 4, 0 ins, 1 del, 1 sub ]",
                                            "u1 %CER 0.00 [ 0 / 11, 0 ins, 0 del, 0 sub ]", "u2 %CER 42.86 [ 3 / 7, 0 ins, 2 del, 1 sub ]"]
    h.write_text("u2 a x c\nu9 nothing\n")  # Kaldi text on both sides, one unit
    assert se.main(["--ref", str(r), "--hyp", str(h), "--unit", "word"]) == 0
    assert capsys.readouterr().out.splitlines()[0] == "%WER 50.00 [ 2 / 4, 0 ins, 1 del, 1 sub ]"
    h.write_text("u9 nothing\n")
    assert se.main(["--ref", str(r), "--hyp", str(h)]) == 1 and "no utterances matched" in capsys.readouterr().err


def run_cli(tr, argv, path):
    assert tr.main(argv + ["--out", str(path)]) == 0
    return path.read_text()


def test_transcribe_select_and_ref_ids(gu, metrics, tmp_path, monkeypatch, capsys):
    tr = importlib.import_module("loco-asr_amd.transcribe")
    model = one_layer_model(gu)
    monkeypatch.setattr(tr, "build_model", lambda args: model)  # the CLI's own path from the arguments on; 1-layer weights keep it quick
    common = ["--random-init", "--synthetic", "4", "--slots", "8", "--nbest", "4", "--seed", "3"]
    plain = run_cli(tr, common, tmp_path / "plain.jsonl")
    assert run_cli(tr, common + ["--select", "first"], tmp_path / "first.jsonl") == plain  # byte for byte
    chosen = [json.loads(l) for l in run_cli(tr, common + ["--select", "mbr"], tmp_path / "mbr.jsonl").splitlines()]
    base = [json.loads(l) for l in plain.splitlines()]
    assert len(chosen) == len(base) == 4
    for line, was in zip(chosen, base):
        nbest = line["nbest"]
        assert [{k: v for k, v in r.items() if k != "mbr_risk"} for r in nbest] == was["nbest"]  # the list itself is what it was
        sel = metrics.mbr_select([[r["ids"] for r in nbest]])  # every sample weighs 1: the sums are of integers, exact in any order
        assert bits([r["mbr_risk"] for r in nbest]) == bits(sel.risk[0].cpu().numpy())
        least = min(r["mbr_risk"] for r in nbest)
        mine = line["token_ids"][:tr.row_length(line["token_ids"])]
        assert any(r["ids"] == mine and r["mbr_risk"] == least for r in nbest), line["id"]
        assert nbest[int(sel.best[0])]["mbr_risk"] == least
    # --ref-ids built from a run's own output: zero errors; one id changed per line: exactly that many substitutions
    # (with synthetic weights a greedy row ends at its first token or never; at temperature 8 a sampled row is a near-uniform draw)
    greedy = common + ["--temperature", "8"]
    lines = [json.loads(l) for l in run_cli(tr, greedy, tmp_path / "greedy.jsonl").splitlines()]
    own = {l["id"]: metrics.strip_specials(l["token_ids"]).tolist() for l in lines}
    full = [k for k, v in own.items() if len(v) >= 2]
    assert len(full) >= 2, own
    same, changed = tmp_path / "same.ids", tmp_path / "changed.ids"
    same.write_text("".join(f"{k} {' '.join(map(str, own[k]))}\n" for k in full))
    changed.write_text("".join(f"{k} {' '.join(map(str, own[k][:1] + [5 if own[k][1] != 5 else 6] + own[k][2:]))}\n" for k in full[:-1]))
    capsys.readouterr()
    scored = [json.loads(l) for l in run_cli(tr, greedy + ["--ref-ids", str(same)], tmp_path / "same.jsonl").splitlines()]
    for line, was in zip(scored, lines):
        if line["id"] in full:
            assert line.pop("errors") == {"cer": 0.0, "sub": 0, "del": 0, "ins": 0, "ref_len": len(own[line["id"]])}
        assert line == was
    total = sum(len(own[k]) for k in full)
    assert f"%CER 0.00 [ 0 / {total}, 0 ins, 0 del, 0 sub ]" in capsys.readouterr().err
    scored = [json.loads(l) for l in run_cli(tr, greedy + ["--ref-ids", str(changed)], tmp_path / "changed.jsonl").splitlines()]
    for line in scored:
        if line["id"] in full[:-1]:
            n = len(own[line["id"]])
            assert line["errors"] == {"cer": 1 / n, "sub": 1, "del": 0, "ins": 0, "ref_len": n}
        else:
            assert "errors" not in line  # no reference: named once, not counted
    err = capsys.readouterr().err
    k, total = len(full) - 1, sum(len(own[u]) for u in full[:-1])
    assert f"[ {k} / {total}, 0 ins, 0 del, {k} sub ]" in err and err.count(f"no reference for {full[-1]}") == 1
    assert f"scored {k} utterances, {4 - k} without a reference" in err


def test_transcribe_paths_write_the_same_lines_from_one_record(gu, tmp_path, monkeypatch):
    """Both decode paths produce transcribe.Line records for one writer: five utterances, so the last batch is a single one.  Per line
    id, token_ids and errors are equal between the pair path and the pool; the floats are each path's own (test_gpu_decoder_score.py
    says how they relate) and only their presence and lengths are looked at.  With --nbest --scores the line's logprob IS the chosen
    hypothesis's sum in the list -- one double, written twice."""
    tr = importlib.import_module("loco-asr_amd.transcribe")
    model = one_layer_model(gu)
    monkeypatch.setattr(tr, "build_model", lambda args: model)
    common = ["--random-init", "--synthetic", "5", "--synthetic-seconds", "1", "--max-length", "8"]
    # references built from a first run's own ids.  With these weights a greedy row ends at its first token and leaves no id to
    # write down, so line k's reference is its own ids with k + 1 more behind them: no two lines expect the same counts, whatever
    # the model wrote, and line 1 gets no reference at all
    first = [json.loads(l) for l in run_cli(tr, common, tmp_path / "first.jsonl").splitlines()]
    assert len(first) == 5
    ref_ids = {l["id"]: tr.strip_special(l["token_ids"]) + [10 + k] * (k + 1) for k, l in enumerate(first) if k != 1}
    refs = tmp_path / "own.ids"
    refs.write_text("".join(f"{k} {' '.join(map(str, v))}\n" for k, v in ref_ids.items()))
    flags = common + ["--scores", "--timestamps", "--ref-ids", str(refs)]
    pair = [json.loads(l) for l in run_cli(tr, flags, tmp_path / "pair.jsonl").splitlines()]
    pool = [json.loads(l) for l in run_cli(tr, flags + ["--slots", "4", "--pack", "2"], tmp_path / "pool.jsonl").splitlines()]
    assert len(pair) == len(pool) == 5
    for a, b, was in zip(pair, pool, first):
        assert a["id"] == b["id"] == was["id"] and a["token_ids"] == b["token_ids"] == was["token_ids"]
        want = {}
        if a["id"] in ref_ids:
            r = ref_ids[a["id"]]
            S, D, I, _ = ref.edit_counts(r, tr.strip_special(a["token_ids"]))
            want = {"errors": {"cer": (S + D + I) / len(r), "sub": S, "del": D, "ins": I, "ref_len": len(r)}}
        generated = tr.row_length(a["token_ids"]) - 1
        for line in (a, b):
            assert list(line) == ["id", "token_ids", "logprob", "avg_logprob", "token_times"] + list(want)
            assert {k: line[k] for k in want} == want, line["id"]
            assert line["avg_logprob"] == line["logprob"] / generated
            assert len(line["token_times"]) == generated and all(len(p) == 2 for p in line["token_times"])
    mbr = common + ["--slots", "4", "--nbest", "3", "--seed", "3", "--greedy-first", "--scores", "--select", "mbr"]
    for line in (json.loads(l) for l in run_cli(tr, mbr, tmp_path / "mbr.jsonl").splitlines()):
        mine = line["token_ids"][:tr.row_length(line["token_ids"])]
        assert any(r["ids"] == mine and r["logprob"] == line["logprob"] for r in line["nbest"]), line["id"]  # exact: one double
