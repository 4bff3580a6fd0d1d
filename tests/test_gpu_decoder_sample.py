"""-m gpu: sampling in the text decoder -- loco_op_sample_tokens (csrc/decoder_sample.hip), the sampling slot pool
(loco_decoder_pool_admit_samples / _step_sample, decoder.DecoderPool(sample=)), sample_many, sample and transcribe --nbest.  2 + 2 layer
synthetic weights (tests/decoder_pool_cases.py).

1. the operator's exact parts: the uniform against the CPU Philox bit for bit, greedy rows against the scoring kernel's argmax,
   degenerate rows, a row stride wider than the row
2. the operator's keep mask and draw against float64 (tests/decoder_sample_ref.py) on the same fp32 logits.  A mask element is left out
   when |A_i - (1 - top_p)| <= band, a draw when u lies within band of a prefix boundary of a kept column; everything else is equal.
   band = max(4 e_torch, 2^-21): e_torch is the largest difference between torch's own CPU fp32 softmax / cumsum and float64 on the
   case's rows (the reference's fp32 error, never the kernel's; the 4 allows another summation order), 2^-21 is 4 ulp of a mass near 1.
   At most 1 % of a case's elements and of its draws may be left out.  The draw is referred to the device's own keep mask, which the
   mask comparison holds to the reference: no draw is left out on account of the mask.  Frequencies of 64 x 257 draws of one row
   against the float64 probabilities by a chi-square with a fixed seed, bound = the 1 - 1e-6 quantile.
3. the model: a hypothesis does not depend on slots, admission order or projected / copied cross caches, bit for bit; seeds;
   greedy_first; top_k = 1; greedy decoding is what it was before and after a sampled call
4. sample's layout and scores; 5. the CLI"""
import ctypes as C
import importlib
import json

import numpy as np
import pytest
import torch

import decoder_pool_cases as pc
import decoder_sample_ref as ref
from conftest import record_figure
from test_gpu_decoder_pool import batches_of, encode, small_model
from test_gpu_decoder_score import GAP, floor_of, padded, score_op

pytestmark = pytest.mark.gpu

SEED = 0x9e3779b97f4a7c15


@pytest.fixture(scope="module")
def gu():
    return importlib.import_module("gpu_util")


@pytest.fixture(scope="module")
def dec():
    return importlib.import_module("loco-asr_amd.decoder")


def config(gu, temperature=1.0, top_k=0, top_p=1.0, seed=SEED):
    return gu._libmod.SampleConfig(C.sizeof(gu._libmod.SampleConfig), temperature, top_k, top_p, seed)


def sample_op(gu, rows, V, cfg, counters, greedy=None):
    """loco_op_sample_tokens on ``rows`` f32 [M, ld] (host): host tensors tokens i64 [M], keep bool [M, V], uniform f32 [M]."""
    rows = torch.as_tensor(rows)
    M, ld = rows.shape
    x, c = gu.dev(rows), torch.from_numpy(np.ascontiguousarray(counters, dtype=np.uint32).view(np.int32)).cuda()  # the u32 bit patterns
    assert c.shape == (M, 3)
    g = gu.dev(greedy, torch.int32) if greedy is not None else None
    tokens = torch.full((M,), -7, dtype=torch.int32, device="cuda")
    keep = torch.full((M, V), -7, dtype=torch.int32, device="cuda")
    uniform = torch.full((M,), 123.0, device="cuda")
    gu.check(gu.lib().loco_op_sample_tokens(gu.ptr(x), ld, M, V, C.byref(cfg), gu.ptr(c), gu.ptr(g), gu.ptr(tokens), gu.ptr(keep), gu.ptr(uniform),
                                            gu.stream()), "loco_op_sample_tokens")
    torch.cuda.synchronize()
    assert torch.equal(x.cpu().view(torch.int32), rows.contiguous().view(torch.int32))  # the logits are only read
    keep = keep.cpu()
    assert bool(((keep == 0) | (keep == 1)).all())
    return tokens.cpu().long(), keep.bool(), uniform.cpu()


def counters_for(M, rng):
    c = np.stack([rng.integers(0, 2 ** 32, M), rng.integers(0, 64, M), 1 + rng.integers(0, 449, M)], -1).astype(np.uint32)
    c[0] = (0xffffffff, 0xffffffff, 0xffffffff)
    return c


def cpu_uniform(cfg, counters):
    return torch.tensor([ref.uniform(int(cfg.seed), *(int(v) for v in c)) for c in counters], dtype=torch.float32)


WIDTHS = [1, 2, 63, 64, 65, 81, 129, 1000]  # one lane, around the wave's 64, the vocabulary, 16 columns per lane
ROWS = [1, 64, 257]                         # below and above the 4 rows of a workgroup; 65 workgroups


# ---- 1. the operator, exact parts ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pad", [0, 7])
def test_op_uniform_greedy_rows_and_range(gu, pad):
    rng = np.random.default_rng(100 + pad)
    cfg = config(gu, 0.9, 5, 0.9)
    for V in WIDTHS:
        for M in ROWS:
            x = torch.from_numpy((rng.standard_normal((M, V)) * 4).astype(np.float32))
            rows = padded(x, V + pad)
            counters = counters_for(M, rng)
            greedy = (np.arange(M) % 3 == 1).astype(np.int32)
            tokens, keep, uniform = sample_op(gu, rows, V, cfg, counters, greedy)
            assert torch.equal(uniform, cpu_uniform(cfg, counters)), (V, M)  # bit for bit: 24-bit values are exact in fp32
            assert bool(((tokens >= 0) & (tokens < V)).all())
            assert bool(keep[torch.arange(M), tokens].all()), "a token outside its row's keep mask"
            g = torch.from_numpy(greedy).bool()
            chosen = score_op(gu, rows, V, 1, M, None, chosen=True, reduce=False)["chosen"][0].long()
            assert torch.equal(tokens[g], chosen[g]), (V, M)
            assert torch.equal(keep[g], torch.nn.functional.one_hot(chosen[g], V).bool())
            again, _, _ = sample_op(gu, rows, V, cfg, counters)  # no flags: as flags of 0 everywhere -- and the same draw twice
            assert torch.equal(again[~g], tokens[~g])


@pytest.mark.parametrize("pad", [0, 7])
def test_op_degenerate_rows(gu, pad):
    nan, inf = float("nan"), float("inf")
    rng = np.random.default_rng(5)
    cfg = config(gu, 0.7, 3, 0.9)
    for V in WIDTHS:
        base = (rng.standard_normal(V) * 4).astype(np.float32)
        rows = []
        for edit in ({0: nan}, {V - 1: nan}, {0: nan, V - 1: nan}, {V // 2: inf}, {0: inf, V - 1: inf}, {V - 1: nan, V // 2: inf}):
            r = base.copy()
            for i, v in edit.items():
                r[i] = v
            rows.append(r)
        rows.append(np.full(V, -inf, np.float32))
        r = np.full(V, -inf, np.float32)
        r[V // 3] = 1.5  # one finite column: not degenerate, and the only token there is
        rows.append(r)
        x = torch.from_numpy(np.stack(rows))
        M = x.shape[0]
        tokens, keep, _ = sample_op(gu, padded(x, V + pad), V, cfg, counters_for(M, rng))
        want = [ref.argmax_rule(r) for r in x]
        assert tokens.tolist() == want, (V, tokens.tolist(), want)
        assert torch.equal(keep, torch.nn.functional.one_hot(tokens, V).bool())
        assert tokens.tolist() == [ref.sample_row(r, 0.7, 3, 0.9, SEED, 1, 2, 3) for r in x]


# ---- 2. keep mask and draw against float64 -------------------------------------------------------------------------------------------
SHAPES = [(2, 257, 0), (63, 64, 7), (64, 64, 0), (65, 257, 7), (81, 257, 0), (81, 64, 7), (129, 64, 7), (1000, 64, 0), (1000, 1, 7)]
MAX_LEFT_OUT = 0.01


@pytest.mark.parametrize("V,M,pad", SHAPES)
def test_op_keep_mask_and_draw_against_float64(gu, V, M, pad):
    rng = np.random.default_rng(1000 * V + M)
    x = torch.from_numpy((rng.standard_normal((M, V)) * 4).astype(np.float32))
    rows, counters = padded(x, V + pad), counters_for(M, rng)
    for T in (0.7, 1.0, 8.0):
        e_torch = ref.reference_error(x, T)
        band = max(4 * e_torch, 2.0 ** -21)
        for top_k in (0, 1, 5, V):
            for top_p in (1.0, 0.9, 0.3):
                cfg = config(gu, T, top_k, top_p)
                tokens, keep, uniform = sample_op(gu, rows, V, cfg, counters)
                want_keep, A = ref.keep_mask_rows(x, T, top_k, top_p)
                near = torch.zeros_like(want_keep) if top_p == 1.0 else (A - (1 - float(np.float32(top_p)))).abs() <= band  # NaN: False
                assert torch.equal(keep[~near], want_keep[~near]), (T, top_k, top_p, (keep != want_keep).nonzero()[:4])
                want_tokens, margin, _ = ref.draw_rows(x, T, keep, uniform.double())
                close = margin <= band
                assert torch.equal(tokens[~close], want_tokens[~close]), (T, top_k, top_p, (tokens != want_tokens).nonzero()[:4])
                left_mask, left_draw = float(near.float().mean()), float(close.float().mean())
                print(f"V {V} M {M} T {T} top_k {top_k} top_p {top_p}: e_torch {e_torch:.3e} band {band:.3e} left out: mask {left_mask:.4%} draws {left_draw:.4%}")
                record_figure("decoder_sample_parity", V=V, M=M, pad=pad, temperature=T, top_k=top_k, top_p=top_p, e_torch=e_torch, band=band,
                              mask_left_out=left_mask, draws_left_out=left_draw)
                assert left_mask <= MAX_LEFT_OUT and left_draw <= MAX_LEFT_OUT, (left_mask, left_draw)


def test_op_frequencies_chi_square(gu):
    """V = 81, T = 1, one row, 64 x 257 draws with the counters (utterance < 64, hypothesis < 257, t = 1): the chi-square statistic of
    the counts against the float64 probabilities (columns whose expected count is below 5 pooled into one bin) stays below the
    1 - 1e-6 quantile: a correct kernel fails one seed in a million, and this seed is fixed."""
    V, n = 81, 64 * 257
    rng = np.random.default_rng(81)
    row = torch.from_numpy((rng.standard_normal(V) * 4).astype(np.float32))
    counters = ref.counters(np.arange(n) // 257, np.arange(n) % 257, 1)
    tokens, keep, _ = sample_op(gu, row[None].repeat(n, 1), V, config(gu), counters)
    assert bool(keep.all())
    expect = torch.softmax(row.double(), 0) * n
    counts = torch.bincount(tokens, minlength=V).double()
    big = expect >= 5
    obs = torch.cat([counts[big], counts[~big].sum()[None]])
    exp = torch.cat([expect[big], expect[~big].sum()[None]])
    stat = float(((obs - exp) ** 2 / exp).sum())
    bound = ref.chi2_quantile(1 - 1e-6, obs.numel() - 1)
    print(f"chi-square {stat:.2f} over {obs.numel()} bins (bound {bound:.2f})")
    record_figure("decoder_sample_chi_square", V=V, draws=n, bins=int(obs.numel()), statistic=stat, bound=bound)
    assert stat <= bound, (stat, bound)


# ---- 3. the model -----------------------------------------------------------------------------------------------------------------------
N, TEMPERATURE = 5, 8.0


def hypotheses(items, greedy_first=False):
    """N hypotheses of every PoolItem, siblings consecutive; key = utterance * N + hypothesis."""
    return [type(it)(key=it.key * N + h, enc_out=it.enc_out, frames=it.frames, clip=it.clip, rows=it.rows, cap=it.cap, utterance=it.key, hypothesis=h,
                     greedy=greedy_first and h == 0) for it in items for h in range(N)]


def decode_samples(dec, model, items, slots, cfg, poll_steps=8):
    """{key: (ids, step logits, scores)} on the host, through a fresh sampling pool."""
    pool = dec.DecoderPool(model.speecht5.encoder, slots, max(it.rows for it in items), max(it.cap for it in items), torch.device("cuda", 0),
                           poll_steps=poll_steps, return_logits=True, return_scores=True, sample=cfg)
    pool.submit(list(items))
    return {k: (ids, lg.cpu(), sc.cpu()) for k, ids, lg, sc in pool.drain()}


def same(a, b):
    return a.keys() == b.keys() and all(all(torch.equal(x, y) for x, y in zip(a[k], b[k])) for k in a)


@pytest.fixture(scope="module")
def sampled(gu, dec):
    model = small_model(gu)
    clips, caps = pc.neighbour_clips(gu.la.synth), pc.NEIGHBOUR_CAPS
    items, _, _ = encode(gu, model, clips, caps)
    cfg = config(gu, TEMPERATURE)
    hyps = hypotheses(items)
    return model, items, hyps, cfg, decode_samples(dec, model, hyps, 2, cfg)


def test_hypotheses_do_not_depend_on_slots_or_order(gu, dec, sampled):
    model, items, hyps, cfg, base = sampled
    assert sorted(base) == list(range(12 * N))
    for k, (ids, lg, sc) in base.items():
        cap, n = items[k // N].cap, len(ids)
        assert ids[0] == 2 and 2 <= n <= cap and (n == cap or ids[-1] == 2) and 2 not in ids[1:-1].tolist()
        assert lg.shape == (n - 1, 81) and sc.shape == (n - 1,) and bool(torch.isfinite(lg).all())
    # at 2 slots no utterance's 5 hypotheses are admitted together (projected and copied caches in every mix); at 64 all are
    for slots in pc.NEIGHBOUR_SLOTS[1:]:
        assert same(base, decode_samples(dec, model, hyps, slots, cfg)), slots
    assert same(base, decode_samples(dec, model, hyps[::-1], 5, cfg)), "reversed"
    assert same(base, decode_samples(dec, model, hyps, 5, cfg, poll_steps=3)), "another poll rhythm"
    distinct = {tuple(base[u * N + h][0].tolist()) for u in range(12) for h in range(N)}
    assert len(distinct) > 12, "the hypotheses of an utterance never differ: temperature 8 does not spread these logits"


def test_hypotheses_equal_the_operator_alone(gu, sampled):
    """Every token is loco_op_sample_tokens of its step's logits with the counter (utterance, hypothesis, t); every score the scoring
    kernel's log P of that token on the same logits."""
    _, _, _, cfg, base = sampled
    for k, (ids, lg, sc) in base.items():
        n = len(ids)
        tokens, _, _ = sample_op(gu, lg, 81, cfg, ref.counters(k // N, k % N, np.arange(1, n)))
        assert tokens.tolist() == ids[1:].tolist(), k
        alone = score_op(gu, lg, 81, 1, n - 1, ids[1:].to(torch.int32), reduce=False)
        assert torch.equal(alone["lp"][0], sc), k


def test_seeds_greedy_first_and_top_k_1(gu, sampled):
    model, items, _, cfg, base = sampled
    clips, caps = pc.neighbour_clips(gu.la.synth), pc.NEIGHBOUR_CAPS
    batches = batches_of(gu, clips)
    # greedy decoding before any sampled call of this test
    g_ids0, g_lg0, g_sc0 = model.generate_many(batches, max_length=caps, slots=5, return_logits=True, return_scores=True)
    gen0 = model.generate(**batches[2], max_length=12, return_logits=True)
    kw = dict(num_return_sequences=N, temperature=TEMPERATURE, max_length=caps, slots=5)
    a = model.sample_many(batches, seed=SEED, return_logits=True, return_scores=True, **kw)
    b = model.sample_many(batches, seed=SEED, return_logits=True, return_scores=True, **dict(kw, slots=64))
    assert a.seed == b.seed == SEED and a[0].seed == SEED
    flat = lambda res: [t for field in res for per in field for t in per]  # noqa: E731
    assert len(a[0]) == 12 and all(len(per) == N for per in a[0])
    assert all(torch.equal(x, y) for x, y in zip(flat(a), flat(b))), "two calls with one seed"
    # the pool driven directly on one packed forward of the same batches is the same computation
    assert all(torch.equal(a[0][u][h], base[u * N + h][0]) and torch.equal(a[2][u][h].cpu(), base[u * N + h][2]) for u in range(12) for h in range(N))
    c = model.sample_many(batches, seed=SEED + 1, **kw)
    assert any(not torch.equal(x, y) for x, y in zip(flat([a[0]]), flat([c]))), "two seeds give the same hypotheses"
    torch.manual_seed(31)
    d = model.sample_many(batches, **kw)
    torch.manual_seed(31)
    e = model.sample_many(batches, **kw)
    assert d.seed == e.seed and all(torch.equal(x, y) for x, y in zip(flat([d]), flat([e])))
    assert d.seed != model.sample_many(batches[:1], **dict(kw, max_length=3)).seed  # the generator moved on
    # greedy_first: hypothesis 0 is generate_many's transcript and scores, bit for bit; the others are the seed's
    f, f_sc = model.sample_many(batches, seed=SEED, greedy_first=True, return_scores=True, **kw)
    for u in range(12):
        assert torch.equal(f[u][0], g_ids0[u]) and torch.equal(f_sc[u][0], g_sc0[u]), u
        assert all(torch.equal(f[u][h], a[0][u][h]) for h in range(1, N)), u
    # top_k = 1: every hypothesis is the greedy one
    one = model.sample_many(batches, seed=SEED, top_k=1, **kw)
    assert all(torch.equal(one[u][h], g_ids0[u]) for u in range(12) for h in range(N))
    # greedy decoding after the sampled calls: what it was
    g_ids1, g_lg1, g_sc1 = model.generate_many(batches, max_length=caps, slots=5, return_logits=True, return_scores=True)
    gen1 = model.generate(**batches[2], max_length=12, return_logits=True)
    assert all(torch.equal(x, y) for x, y in zip(g_ids0 + g_lg0 + g_sc0, g_ids1 + g_lg1 + g_sc1))
    assert torch.equal(gen0[0], gen1[0]) and torch.equal(gen0[1], gen1[1])


def test_greedy_and_sampled_slots_in_one_pool(gu, dec, sampled):
    """A slot admitted through loco_decoder_pool_admit is greedy under loco_decoder_pool_step_sample; loco_decoder_pool_step refuses a
    pool that holds a slot which draws, by LOCO_E_STATE, until the pool is initialised again."""
    model, items, hyps, cfg, base = sampled
    short = [it for it in items if it.rows <= 49 and it.cap <= 17]
    greedy = dec.DecoderPool(model.speecht5.encoder, 4, 49, 17, torch.device("cuda", 0), return_logits=True, return_scores=True)
    greedy.submit(list(short))
    want = {k: (ids, lg.cpu(), sc.cpu()) for k, ids, lg, sc in greedy.drain()}
    pool = dec.DecoderPool(model.speecht5.encoder, 4, 49, 17, torch.device("cuda", 0), return_logits=True, return_scores=True, sample=cfg)
    n_greedy = 2
    for r in range(n_greedy):
        pool.admit([r], [short[r]])  # the greedy admit
    mine = [h for h in hyps if h.utterance == short[2].key][:2]
    pool.admit_samples([2, 3], [mine])
    lib, args, ws = gu.lib(), (model.speecht5.encoder._handle, 4, 49, 17), C.c_void_p(pool.workspace.data_ptr())
    assert lib.loco_decoder_pool_step(*args, 0, 49, None, ws, pool.workspace.numel(), gu.stream()) == -2
    assert b"admitted to sample" in lib.loco_last_error()
    got = {k: (ids, lg.cpu(), sc.cpu()) for k, ids, lg, sc in pool.drain()}
    for it in short[:n_greedy]:
        assert all(torch.equal(x, y) for x, y in zip(got[it.key], want[it.key])), it.key
    for h in mine:
        assert all(torch.equal(x, y) for x, y in zip(got[h.key], base[h.key])), h.key
    gu.check(lib.loco_decoder_pool_init(*args, ws, pool.workspace.numel(), gu.stream()), "loco_decoder_pool_init")
    assert lib.loco_decoder_pool_step(*args, 0, 49, None, ws, pool.workspace.numel(), gu.stream()) == 0  # an empty greedy pool again
    with pytest.raises(ValueError, match="3 clips x 2 copies for a pool of 4 slots"):
        gu.check(lib.loco_decoder_pool_admit_samples(*args, 3, 2, None, None, 0, None, None, None, None, None, None, ws, pool.workspace.numel(),
                                                     gu.stream()), "loco_decoder_pool_admit_samples")
    torch.cuda.synchronize()


# ---- 4. sample ----------------------------------------------------------------------------------------------------------------------------
def test_sample_layout_and_scores(gu, dec):
    model = small_model(gu)
    clips = pc.oracle_clips(gu.la.synth)[:4]
    batch = batches_of(gu, clips, size=4)[0]
    B, n, S_max = 4, 3, 12
    kw = dict(num_return_sequences=n, temperature=TEMPERATURE, seed=SEED, max_length=S_max)
    out = model.sample(batch["input_values"], batch["attention_mask"], return_scores=True, **kw)
    hyps, logits = model.sample_many([batch], return_logits=True, **kw)
    assert isinstance(out, dec.SampleOutput) and out.seed == SEED and out.sequences.is_cuda and out.sequences.dtype == torch.long
    seqs = out.sequences.cpu()
    S = max(len(h) for per in hyps for h in per)
    assert seqs.shape == (B * n, S) and S <= S_max
    lp, total = out.token_logprobs.cpu(), out.sequence_logprobs.cpu()
    assert lp.shape == (B * n, S - 1) and total.shape == (B * n,)
    bare = model.sample(batch["input_values"], batch["attention_mask"], **kw)
    assert torch.equal(bare.sequences, out.sequences) and bare.token_logprobs is None and bare.sequence_logprobs is None
    labels = torch.full((B * n, S - 1), -100, dtype=torch.long)
    steps = torch.zeros((B * n, S - 1, 81))
    for b in range(B):
        for h in range(n):
            row, k = b * n + h, len(hyps[b][h])
            assert seqs[row, :k].tolist() == hyps[b][h].tolist() and bool((seqs[row, k:] == 1).all()), (b, h)  # <pad> after the row's end
            assert bool((lp[row, k - 1:] == 0).all()) and bool((lp[row, :k - 1] <= 0).all())
            labels[row, :k - 1] = hyps[b][h][1:]
            steps[row, :k - 1] = logits[b][h].cpu()
    # against score() of the sequences as labels: the teacher-forced logits differ from the steps' by delta, log_softmax moves by at
    # most twice that (tests/test_gpu_decoder_score.py's bar for forward(labels=)), the sums by the sum over their tokens
    x, m = batch["input_values"].repeat_interleave(n, 0), batch["attention_mask"].repeat_interleave(n, 0)
    sc = model.score(x, m, labels=labels)
    forced = model(x, m, labels=labels).logits.cpu()
    counted = labels != -100
    delta = (forced - steps).abs().amax(-1).double() * counted
    ref_lp = sc.token_logprobs.cpu().double()
    lim = (2 * delta + floor_of(ref_lp)) * counted
    err = (lp.double() - ref_lp).abs()
    assert bool((err <= lim).all()), float((err / lim.clamp(min=1e-300)).max())
    want = sc.sequence_logprob.cpu().double()
    lim_seq = lim.sum(1) + 2.0 ** -23 * want.abs()  # both sums are stored as fp32
    err_seq = (total.double() - want).abs()
    record_figure("decoder_sample_vs_score", delta_max=float(delta.max()), worst_error_over_bar=float((err_seq / lim_seq).max()))
    assert bool((err_seq <= lim_seq).all()), (err_seq, lim_seq)
    assert sc.tokens.cpu().tolist() == counted.sum(1).tolist()


# ---- 5. the CLI ---------------------------------------------------------------------------------------------------------------------------
def test_transcribe_nbest(gu, tmp_path, monkeypatch):
    tr = importlib.import_module("loco-asr_amd.transcribe")
    model = small_model(gu)
    monkeypatch.setattr(tr, "build_model", lambda args: model)  # the CLI's own path from the arguments on; 2-layer weights keep it quick
    common = ["--random-init", "--synthetic", "4", "--slots", "4"]
    nbest = ["--nbest", "3", "--greedy-first", "--seed", "7"]
    for extra in ([], ["--scores"]):
        a, b = tmp_path / "plain.jsonl", tmp_path / "nbest.jsonl"
        assert tr.main(common + extra + ["--out", str(a)]) == 0
        assert tr.main(common + extra + nbest + ["--out", str(b)]) == 0
        plain, lines = [json.loads(l) for l in a.read_text().splitlines()], [json.loads(l) for l in b.read_text().splitlines()]
        assert len(plain) == len(lines) == 4
        for p, l in zip(plain, lines):
            best = l.pop("nbest")
            assert l == p  # the line's own fields are the greedy transcript's
            assert len(best) == 3 and all(set(r) == {"ids", "logprob", "avg_logprob"} for r in best)
            assert [r["logprob"] for r in best] == sorted((r["logprob"] for r in best), reverse=True)
            assert all(r["ids"][0] == 2 and abs(r["avg_logprob"] - r["logprob"] / (len(r["ids"]) - 1)) < 1e-12 for r in best)
            greedy_ids = p["token_ids"][:tr.row_length(p["token_ids"])]
            assert greedy_ids in [r["ids"] for r in best]
            if extra:
                assert any(r["ids"] == greedy_ids and r["logprob"] == p["logprob"] for r in best)
    with pytest.raises(SystemExit, match="--nbest needs --slots"):
        tr.main(["--random-init", "--synthetic", "2", "--nbest", "3"])
